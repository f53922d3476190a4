"""Posterior histograms counted on the device (bisip_chain_range_dev, bisip_chain_histograms_dev,
bisip_chain_pair_histograms_dev), from the C entry points up to the model and SpectraBatch methods.  Every count is
compared with NumPy (np.histogram / np.histogram2d) on a host copy of the same samples: integer equality, no
tolerance."""
import warnings

import numpy as np
import pytest

from chain_harness import GuardedCall, used_window

pytestmark = pytest.mark.gpu


def numpy_histograms(flat, ranges, bins):
    """np.histogram of every column of flat (n, ndim) within ranges (ndim, 2): counts (ndim, bins), edges."""
    with np.errstate(invalid='ignore'):
        out = [np.histogram(flat[:, q], bins, tuple(ranges[q])) for q in range(flat.shape[1])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def numpy_pair_histograms(flat, ranges, bins):
    jj, kk = np.triu_indices(flat.shape[1], 1)
    out = np.empty((jj.size, bins, bins), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for q, (j, k) in enumerate(zip(jj, kk)):
            out[q] = np.histogram2d(flat[:, j], flat[:, k], bins, [tuple(ranges[j]), tuple(ranges[k])])[0]
    return out


def flat_of(host, e, Wp):
    """(n, E * Wp, ndim) host samples -> the flat chain (n * Wp, ndim) of ensemble e."""
    return host[:, e * Wp:(e + 1) * Wp].reshape(-1, host.shape[2])


def abi_counts(t, offset, n, stride, E, Wp, ndim, edges):
    """Both entry points on device tensor t: (counts (E, ndim, bins), pair counts (E, npairs, bins, bins)).  The counts
    start as -7 (the call must clear them) and are followed by guard values."""
    import torch
    from bisip_amd import _hip
    bins = edges.shape[2] - 1
    d_edges = torch.from_numpy(np.ascontiguousarray(edges)).cuda()
    call = GuardedCall()
    counts = call.out('the counts', (E, ndim, bins), torch.int64)
    _hip.chain_histograms_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, d_edges.data_ptr(), bins, counts,
                              call.stream)
    if ndim >= 2:
        pairs = call.out('the pair counts', (E, ndim * (ndim - 1) // 2, bins, bins), torch.int64)
        _hip.chain_pair_histograms_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, d_edges.data_ptr(), bins, pairs,
                                       call.stream)
    got = call.finish()
    return got[0], got[1] if ndim >= 2 else None


def abi_range(t, offset, n, stride, E, Wp, ndim):
    import torch
    from bisip_amd import _hip
    call = GuardedCall()
    out, bad = call.out('the range', (E, ndim, 2)), call.out('the count of non-finite values', (E, ndim), torch.int64)
    _hip.chain_range_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, out, bad, call.stream)
    return tuple(call.finish())


def hand_built_chain(E, Wp, ndim, bins, stored, seed):
    """A host chain (stored, E * Wp, ndim) and ranges (E, ndim, 2): columns of widths 1e-8 ... 1e2 around centres of
    any size, every edge planted and its floating-point neighbours, NaN, +-inf and rows outside the range; parameter 1
    has EVERY row of a sample range in one bin (the serialising case) and parameter 2 is constant."""
    rng = np.random.default_rng(seed)
    W = E * Wp
    lo = rng.normal(size=(E, ndim)) * 10.0 ** rng.integers(-3, 3, (E, ndim))
    width = 10.0 ** rng.integers(-8, 3, (E, ndim)).astype(np.float64)
    ranges = np.stack([lo, lo + width], axis=-1)
    u = rng.uniform(-0.05, 1.05, (stored, E, Wp, ndim))                    # ~10 % of the values outside
    x = ranges[None, :, None, :, 0] + u * width[None, :, None, :]
    if ndim > 1:
        x[..., 1] = (ranges[:, 1, 0] + 0.3 * width[:, 1])[None, :, None]   # one bin for every row
    if ndim > 2:
        x[..., 2] = 0.25
        ranges[:, 2] = [0.25, 0.25]                                        # lo == hi: widened by 0.5 either side
    from bisip_amd.histogram import edges_from_range
    edges = edges_from_range(ranges, bins)
    for e in range(E):
        for q in range(ndim):
            if q in (1, 2):
                continue
            ed = edges[e, q]
            plant = np.concatenate([ed, np.nextafter(ed, -np.inf), np.nextafter(ed, np.inf),
                                    [np.nan, np.inf, -np.inf, -np.nan]])
            s = rng.integers(0, stored, plant.size)
            w = rng.integers(0, Wp, plant.size)
            x[s, e, w, q] = plant
    return x.reshape(stored, W, ndim), ranges, edges


CASES = [  # E, Wp, ndim, bins, stored, discard, thin
    (1, 37, 3, 1, 40, 0, 1),
    (1, 37, 3, 25, 40, 5, 3),
    (3, 100, 7, 20, 30, 0, 1),
    (3, 100, 7, 25, 30, 7, 2),
    (3, 100, 7, 64, 30, 1, 4),
    (64, 10, 7, 20, 24, 3, 2),
    (3, 50, 12, 20, 20, 2, 3),        # 66 pairs in two groups
    (1, 70, 12, 64, 20, 0, 1),        # three pairs per group
    (3, 33, 16, 20, 16, 1, 2),        # 120 pairs in four groups
    (1, 65, 16, 64, 12, 0, 1),        # three pairs per group, 40 groups
    (64, 6, 16, 25, 9, 0, 2),
    (1, 1000, 2, 20, 13, 0, 1),       # walkers split over workgroups
]


@pytest.mark.parametrize('E,Wp,ndim,bins,stored,discard,thin', CASES)
def test_entry_points_equal_numpy(hip_lib, E, Wp, ndim, bins, stored, discard, thin):
    import torch
    host, ranges, edges = hand_built_chain(E, Wp, ndim, bins, stored, seed=E * 1000 + ndim * 10 + bins)
    W = E * Wp
    # the stored chain sits inside a larger tensor: pointer offset and a stride of `thin` samples
    pad = 5
    t = torch.full((pad + stored * W * ndim + pad,), float('nan'), dtype=torch.float64, device='cuda')
    t[pad:pad + stored * W * ndim] = torch.from_numpy(host.reshape(-1)).cuda()
    offset, stride, n = used_window(stored, W * ndim, discard, thin)
    offset += pad
    used = host[discard + thin - 1::thin]
    assert used.shape[0] == n >= 2
    counts, pairs = abi_counts(t, offset, n, stride, E, Wp, ndim, edges)
    minmax, bad = abi_range(t, offset, n, stride, E, Wp, ndim)
    r = np.stack([edges[..., 0], edges[..., -1]], axis=-1)
    for e in range(E):
        flat = flat_of(used, e, Wp)
        want, want_edges = numpy_histograms(flat, r[e], bins)
        np.testing.assert_array_equal(want_edges, edges[e])
        np.testing.assert_array_equal(counts[e], want)
        np.testing.assert_array_equal(pairs[e], numpy_pair_histograms(flat, r[e], bins))
        fin = np.isfinite(flat)
        np.testing.assert_array_equal(bad[e], (~fin).sum(axis=0))
        np.testing.assert_array_equal(minmax[e, :, 0], np.where(fin, flat, np.inf).min(axis=0))
        np.testing.assert_array_equal(minmax[e, :, 1], np.where(fin, flat, -np.inf).max(axis=0))
        if ndim > 1:
            assert counts[e, 1].max() == n * Wp              # every row in one bin
    assert counts.sum() < n * W * ndim                       # something was outside


@pytest.mark.parametrize('E,Wp,ndim,n', [(1, 37, 3, 40), (3, 100, 7, 21), (64, 10, 12, 9), (2, 3000, 16, 5)])
def test_range_equals_np_min_max(hip_lib, E, Wp, ndim, n):
    import torch
    g = torch.Generator(device='cuda').manual_seed(n)
    t = torch.randn((n, E * Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
    t[..., 0] *= 1e-300
    t[..., ndim - 1] += 1e9
    minmax, bad = abi_range(t, 0, n, E * Wp * ndim, E, Wp, ndim)
    host = t.cpu().numpy()
    assert not bad.any()
    for e in range(E):
        flat = flat_of(host, e, Wp)
        np.testing.assert_array_equal(minmax[e, :, 0], np.min(flat, axis=0))
        np.testing.assert_array_equal(minmax[e, :, 1], np.max(flat, axis=0))
    # a column without a finite value: (+inf, -inf) and all of it counted
    t[:, :Wp, 1] = float('nan')
    minmax, bad = abi_range(t, 0, n, E * Wp * ndim, E, Wp, ndim)
    assert minmax[0, 1, 0] == np.inf and minmax[0, 1, 1] == -np.inf and bad[0, 1] == n * Wp
    assert bad.sum() == n * Wp


def check_public(obj, host_chain, E, Wp, bounds, kw, bins1=25, bins2=20, batch=True):
    """get_param_histogram / get_corner_histograms of a fitted object against NumPy on its get_chain, for every kind of
    range.  host_chain (n, E * Wp, ndim)."""
    ndim = host_chain.shape[2]
    n = host_chain.shape[0]
    flats = [flat_of(host_chain, e, Wp) for e in range(E)]
    own = np.stack([np.stack([f.min(axis=0), f.max(axis=0)], axis=1) for f in flats])        # (E, ndim, 2)
    mid = own.mean(axis=2, keepdims=True)
    explicit_each = np.concatenate([mid - 0.3 * (mid - own[..., :1]), mid + 0.3 * (own[..., 1:] - mid)], axis=2)
    kinds = [(None, own), ('bounds', np.broadcast_to(bounds.T, (E, ndim, 2))), (explicit_each[0], None)]
    if batch:
        kinds.append((explicit_each, explicit_each))
    for arg, r in kinds:
        if r is None:
            r = np.broadcast_to(arg, (E, ndim, 2))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)
            counts, edges = obj.get_param_histogram(bins=bins1, range=arg, **kw)
            pc, pe, (jj, kk) = obj.get_corner_histograms(bins=bins2, range=arg, **kw)
        if not batch:
            counts, edges, pc, pe = counts[None], edges[None], pc[None], pe[None]
        assert counts.shape == (E, ndim, bins1) and counts.dtype == np.int64
        assert pc.shape == (E, ndim * (ndim - 1) // 2, bins2, bins2) and pc.dtype == np.int64
        np.testing.assert_array_equal(jj, np.triu_indices(ndim, 1)[0])
        np.testing.assert_array_equal(kk, np.triu_indices(ndim, 1)[1])
        for e in range(E):
            want, want_edges = numpy_histograms(flats[e], r[e], bins1)
            np.testing.assert_array_equal(counts[e], want)
            np.testing.assert_array_equal(edges[e], want_edges)
            np.testing.assert_array_equal(pc[e], numpy_pair_histograms(flats[e], r[e], bins2))
            np.testing.assert_array_equal(pe[e], numpy_histograms(flats[e], r[e], bins2)[1])
        if arg is None:
            assert (counts.sum(axis=2) == n * Wp).all()
            assert (pc.sum(axis=(2, 3)) == n * Wp).all()
        elif not isinstance(arg, str):
            assert (counts.sum(axis=2) < n * Wp).all()


DISCARD_THIN = [dict(discard=0, thin=1), dict(discard=40, thin=1), dict(discard=31, thin=7)]


def test_model_fitted_on_the_device():
    import bisip_amd
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=3, nwalkers=32, nsteps=120)
    np.random.seed(2)
    m.fit(chain='device')
    assert m._sampler.chain_on_device
    for kw in DISCARD_THIN:
        host = m.get_chain(**kw)
        check_public(m, host, 1, 32, m.param_bounds, kw, batch=False)
    # an explicit chain takes the NumPy definition: the same integers
    flat = m.get_chain(flat=True, discard=40)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        a = m.get_param_histogram(discard=40)
        b = m.get_param_histogram(chain=flat)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(ValueError, match='no samples'):
        m.get_param_histogram(discard=120)
    with pytest.raises(ValueError, match='range must'):
        m.get_corner_histograms(range=np.zeros((2, 2)), discard=1)
    mm, bad = m._sampler.param_range(discard=40)
    np.testing.assert_array_equal(mm[0, :, 0], flat.min(axis=0))
    np.testing.assert_array_equal(mm[0, :, 1], flat.max(axis=0))
    assert not bad.any()


def test_model_with_a_host_chain_on_the_device_sampler():
    import bisip_amd
    m = bisip_amd.PeltonColeCole(bisip_amd.DataFiles()['SIP-K389175'], n_modes=1, nwalkers=32, nsteps=100)
    np.random.seed(3)
    m.fit()
    assert not m._sampler.chain_on_device
    kw = dict(discard=20, thin=3)
    check_public(m, m.get_chain(**kw), 1, 32, m.param_bounds, kw, batch=False)


def batch_spectra():
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    files = bisip_amd.DataFiles()
    return [files[k] for k in ('SIP-K389175', 'SIP-K389176')] + [synthetic_columns(20, i) for i in range(7)]


@pytest.mark.parametrize('where', ['device', 'host'])
@pytest.mark.parametrize('model,opts', [('PolynomialDecomposition', dict(poly_deg=4)),
                                        ('PeltonColeCole', dict(n_modes=2))])
def test_spectra_batch(model, opts, where):
    import bisip_amd
    spectra = batch_spectra()
    E, Wp = len(spectra), 32
    assert E >= 8
    b = bisip_amd.SpectraBatch(model, spectra, nwalkers=Wp, nsteps=150, **opts)
    np.random.seed(5)
    b.fit(seed=11, chain=where)
    assert b._sampler.chain_on_device == (where == 'device')
    for kw in DISCARD_THIN:
        host = b.get_chain(**kw).reshape(-1, E * Wp, b.ndim)
        check_public(b, host, E, Wp, b.param_bounds, kw)
    with pytest.raises(ValueError, match='no samples'):
        b.get_corner_histograms(discard=150)
    with pytest.raises(ValueError, match='range must'):
        b.get_param_histogram(range=np.zeros((E + 1, b.ndim, 2)))
    with pytest.raises((TypeError, ValueError), match='bins'):
        b.get_param_histogram(bins=0)
    b.close()


def test_range_none_refuses_a_non_finite_sample():
    import torch
    from bisip_amd import histogram as hg
    from bisip_amd.chainview import ChainView
    t = torch.rand((6, 2 * 10, 3), dtype=torch.float64, device='cuda')
    t[4, 13, 2] = float('nan')
    view = ChainView(t, 6, 2, 10, 3)
    minmax, bad = hg.device_param_range(view)
    assert bad.sum() == 1 and bad[1, 2] == 1
    with pytest.raises(ValueError, match='not finite'):
        hg.resolve_range(None, 2, 3, data_range=lambda: (minmax, bad))
    # an explicit range counts the rest
    edges = hg.edges_from_range(hg.resolve_range([[0, 1]] * 3, 2, 3), 10)
    counts = hg.device_histograms(view, edges)
    assert counts[1, 2].sum() == 59 and counts[0].sum() == 180
    pc = hg.device_pair_histograms(view, edges)
    np.testing.assert_array_equal(pc.sum(axis=(2, 3)), [[60, 60, 60], [60, 59, 59]])


def test_full_size_cfg5_slice():
    """512 spectra x 256 walkers, 500 used samples of 1000 stored, 7 parameters: a synthetic chain made on the device."""
    import torch
    from bisip_amd import histogram as hg
    from bisip_amd.chainview import ChainView
    E, Wp, ndim, stored, discard = 512, 256, 7, 1000, 500
    W, n = E * Wp, stored - discard
    g = torch.Generator(device='cuda').manual_seed(2024)
    t = torch.empty((stored, W, ndim), dtype=torch.float64, device='cuda')
    centre = torch.rand((1, W // Wp, 1, ndim), generator=g, dtype=torch.float64, device='cuda')
    for s0 in range(0, stored, 100):
        blk = torch.randn((100, E, Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
        t[s0:s0 + 100] = (centre + 0.05 * blk).reshape(100, W, ndim)
        del blk
    view = ChainView(t, n, E, Wp, ndim, offset=discard * W * ndim, stride=W * ndim)
    minmax, bad = hg.device_param_range(view)
    assert not bad.any()
    edges1 = hg.edges_from_range(minmax, 25)
    counts = hg.device_histograms(view, edges1)
    assert counts.shape == (E, ndim, 25)
    assert (counts.sum(axis=2) == n * Wp).all()
    edges2 = hg.edges_from_range(minmax, 20)
    pc = hg.device_pair_histograms(view, edges2)
    assert pc.shape == (E, 21, 20, 20)
    assert (pc.sum(axis=(2, 3)) == n * Wp).all()
    # the prior box of the survey: the same edges for every spectrum, a narrow posterior inside them
    box = np.broadcast_to(np.array([[-1.0, 2.0]] * ndim), (E, ndim, 2))
    eb1, eb2 = hg.edges_from_range(box, 25), hg.edges_from_range(box, 20)
    cb = hg.device_histograms(view, eb1)
    pb = hg.device_pair_histograms(view, eb2)
    assert (cb.sum(axis=2) == n * Wp).all() and (pb.sum(axis=(2, 3)) == n * Wp).all()
    for e in (0, 1, 63, 200, 255, 256, 400, 511):
        flat = t[discard:, e * Wp:(e + 1) * Wp].reshape(-1, ndim).cpu().numpy()
        np.testing.assert_array_equal(minmax[e, :, 0], flat.min(axis=0))
        np.testing.assert_array_equal(minmax[e, :, 1], flat.max(axis=0))
        want, want_edges = numpy_histograms(flat, minmax[e], 25)
        np.testing.assert_array_equal(edges1[e], want_edges)
        np.testing.assert_array_equal(counts[e], want)
        np.testing.assert_array_equal(pc[e], numpy_pair_histograms(flat, minmax[e], 20))
        np.testing.assert_array_equal(cb[e], numpy_histograms(flat, box[e], 25)[0])
        np.testing.assert_array_equal(pb[e], numpy_pair_histograms(flat, box[e], 20))
