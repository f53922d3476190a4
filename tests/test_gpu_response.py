"""Amplitude / phase bands and response moments on the device (bisip_forward_columns_kind_dev,
bisip_forward_percentiles_kind, bisip_response_moments_dev), from the C entry points up to the model and SpectraBatch
methods.  The reference of every comparison is the library's own forward (the entry point that existed before) over the
host copy of the same samples, then NumPy.  RI through the new entries is held to the bits of the old ones; the RI moments
to the bits of the summation order include/bisip_hip.h states (bisip_amd.response.ordered_response_moments) and, against
the long-double definitions, to the bound of tests/response_bounds.py; the PA percentiles to K ulp of the largest value of
the column, the PA moments to the bound with its K u |x| term."""
import functools

import numpy as np
import pytest

from chain_harness import assert_same_bits, used_window
from response_bounds import assert_within, reference_and_bounds

pytestmark = pytest.mark.gpu

# ulp of the device's double hypot / atan2: the HIP math documentation installed with this ROCm states none, so OpenCL full
# profile's (OpenCL C specification, "Relative error as ULPs", double precision: hypot <= 4 ulp, atan2 <= 6 ulp)
HYPOT_ULP, ATAN2_ULP = 4, 6
GLIBC_ULP = 1             # NumPy's hypot / arctan2 on the reference side
INTERPOLATION_ULP = 3     # the two roundings of lo + t * (hi - lo) and that of t
K_AMP = HYPOT_ULP + GLIBC_ULP + INTERPOLATION_ULP          # 8
K_PHA = ATAN2_ULP + GLIBC_ULP + INTERPOLATION_ULP          # 10
K = (K_AMP, K_PHA)
ULP = 2.0 ** -52

P = np.array([2.5, 50.0, 97.5])
MODEL_ID = {'PolynomialDecomposition': 0, 'PeltonColeCole': 1, 'Dias2000': 2, 'Shin2015': 3}
E = 5


def spectra(n_freq, count):
    """N = 20: the bundled spectra; N = 32: synthetic ones."""
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    if n_freq == 20:
        files = bisip_amd.DataFiles()
        return [files[k] for k in sorted(files)[:count]]
    return [synthetic_columns(n_freq, i) for i in range(count)]


def inside(model, lo, hi, shape, seed):
    """Uniform draws strictly inside the prior box, from the part of it where Re Z > 0 for every model (asserted by the
    tests on the responses themselves): the chargeabilities of a multi-mode Cole-Cole model must not add up to 1, the
    polynomial of a decomposition stays a small correction."""
    rng = np.random.RandomState(seed)
    a, b = lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)
    ndim = lo.size
    if model == 'PolynomialDecomposition':
        a, b = a.copy(), b.copy()
        scale = 0.005 * 6.0 ** -np.arange(ndim - 1)        # log_tau reaches -6: a_p log_tau^p stays small
        a[1:], b[1:] = np.maximum(a[1:], -scale), np.minimum(b[1:], scale)
    elif model == 'PeltonColeCole':
        D = (ndim - 1) // 3
        a, b = a.copy(), b.copy()
        b[1:1 + D] = 0.9 / D
    elif model == 'Dias2000':
        c = np.array([1.0, 0.5, -8.0, 10.0, 0.5])
        a, b = np.maximum(a, c - 0.1 * (hi - lo)), np.minimum(b, c + 0.1 * (hi - lo))
    assert (a > lo).all() and (b < hi).all() and (a < b).all()
    return np.ascontiguousarray(rng.uniform(a, b, tuple(shape) + (ndim,)))


def make_batch(model, kw, n_freq, Wp, count=E):
    import bisip_amd
    return bisip_amd.SpectraBatch(model, spectra(n_freq, count), nwalkers=Wp, nsteps=8, **kw)


def single_context(b, e):
    from bisip_amd import _hip
    kw = {}
    if b.model == 'PolynomialDecomposition':
        kw = dict(poly_deg=b.poly_deg, c_exp=b.c_exp, taus=b.taus, log_taus=b.log_taus)
    if b.model == 'PeltonColeCole':
        kw = dict(n_modes=b.n_modes)
    return _hip.HipContext(MODEL_ID[b.model], b.w[e], b.zn[e], b.zn_err[e], b.param_bounds, **kw)


def forward_rows(b, used, first=0, count=None):
    """Z (count, R, 2, N): forward of every spectrum's rows (k * Wp + w) of the used samples (n, E * Wp, ndim), by a
    single-spectrum context of each spectrum through the entry point that existed before."""
    n, W, ndim = used.shape
    count = b.n_spectra - first if count is None else count
    Wp = W // b.n_spectra
    out = []
    for e in range(first, first + count):
        ctx = single_context(b, e)
        out.append(ctx.forward(np.ascontiguousarray(used[:, e * Wp:(e + 1) * Wp].reshape(n * Wp, ndim))))
        ctx.close()
    return np.stack(out)


def view_of(stored, discard, thin, n_ensembles, Wp, first=0, count=None):
    """The ChainView of the used samples of `count` ensembles starting with `first` of a stored chain tensor."""
    from bisip_amd.chainview import ChainView
    total, W, ndim = stored.shape
    offset, stride, n = used_window(total, W * ndim, discard, thin)
    count = n_ensembles - first if count is None else count
    return ChainView(stored, n, count, Wp, ndim, offset + first * Wp * ndim, stride)


def assert_pa_percentiles(got, Z, what):
    """got (len(P), 2, N) against np.percentile(response_pa(Z), P, axis=0), Z (R, 2, N): K ulp of the column's largest."""
    from bisip_amd import response as rs
    assert (Z[:, 0, :] > 0).all(), f'{what}: Re Z > 0 is a precondition of the inputs'
    pa = rs.response_pa(Z)
    want = np.percentile(pa, P, axis=0)
    N = Z.shape[-1]
    tol = np.repeat(np.asarray(K, dtype=np.float64), N).reshape(2, N) * ULP * np.abs(pa).max(axis=0)
    err = np.abs(got - want)
    worst = float((err / tol).max())
    print(f'{what}: PA percentiles at most {worst:.3f} of K ulp = ({K_AMP}, {K_PHA}) of the largest value')
    assert (err <= tol).all(), (what, worst)


def check_moments(view, ctx, Z, what, first=0, n_spectra=None):
    """Both kinds of the moments of a view against Z (E', R, 2, N): RI the bits of the stated order and the bound, PA the
    bound with its K u |x| term; twice the same bits."""
    from bisip_amd import response as rs
    assert (Z[:, :, 0, :] > 0).all(), f'{what}: Re Z > 0 is a precondition of the inputs'
    m, s = rs.device_model_moments(view, ctx, 'ri', first)
    om, os_ = rs.ordered_response_moments(Z, 'ri', n_spectra)
    assert_same_bits(m, om, f'{what}: mean, ri')
    assert_same_bits(s, os_, f'{what}: std, ri')
    ref = reference_and_bounds(Z, 'ri')
    worst = max(assert_within(m, ref, 'mean', what), assert_within(s, ref, 'std', what))
    mp, sp = rs.device_model_moments(view, ctx, 'pa', first)
    refp = reference_and_bounds(Z, 'pa', K)
    worstp = max(assert_within(mp, refp, 'mean', what + ' pa'), assert_within(sp, refp, 'std', what + ' pa'))
    print(f'{what}: RI moments at most {worst:.3f} of their bound, PA {worstp:.3f}')
    mp2, sp2 = rs.device_model_moments(view, ctx, 'pa', first)
    np.testing.assert_array_equal(mp2.view(np.uint64), mp.view(np.uint64))
    np.testing.assert_array_equal(sp2.view(np.uint64), sp.view(np.uint64))
    m2, s2 = rs.device_model_moments(view, ctx, 'ri', first)
    np.testing.assert_array_equal(m2.view(np.uint64), m.view(np.uint64))
    np.testing.assert_array_equal(s2.view(np.uint64), s.view(np.uint64))
    return (m, s), (mp, sp)


# model, options, N, Wp, stored samples: every Wp with both N; Wp = 8 and 50 take the per-lane branch of the column kernel
# with the rows of a wave straddling spectra, 64 and 192 the whole-wave branch; rows per spectrum 88 ... 11520, never a
# multiple of 256, a multiple of 64 only where Wp is
CASES = [('PolynomialDecomposition', dict(poly_deg=0), 20, 8, 40),
         ('PolynomialDecomposition', dict(poly_deg=5), 32, 50, 45),
         ('PolynomialDecomposition', dict(poly_deg=10), 20, 64, 41),
         ('PeltonColeCole', dict(n_modes=1), 32, 192, 60),
         ('PeltonColeCole', dict(n_modes=3), 20, 50, 52),
         ('Dias2000', {}, 32, 64, 47),
         ('Shin2015', {}, 20, 8, 55),
         ('PeltonColeCole', dict(n_modes=2), 32, 8, 43)]
# the other shapes a context can have, at the smallest sizes above: each of the 18 takes a kernel of its own
CASES += [('PolynomialDecomposition', dict(poly_deg=p), 20, 8, 36 + p) for p in (1, 2, 3, 4, 6, 7, 8, 9)]
CASES += [('PeltonColeCole', dict(n_modes=d), 20, 8, 38 + d) for d in (4, 5)]


@pytest.mark.parametrize('model,kw,n_freq,Wp,stored', CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_bands_and_moments_of_uniform_draws(model, kw, n_freq, Wp, stored):
    import torch
    from bisip_amd.summaries import device_model_percentiles
    b = make_batch(model, kw, n_freq, Wp)
    lo, hi = b.param_bounds
    chain = inside(model, lo, hi, (stored, E * Wp), seed=stored + Wp)
    t = torch.from_numpy(chain).cuda()
    for discard, thin in ((0, 1), (7, 3)):
        used = chain[discard + thin - 1::thin]
        what = f'{model} {kw} N={n_freq} Wp={Wp} discard={discard} thin={thin}'
        # every spectrum of the context
        view = view_of(t, discard, thin, E, Wp)
        assert view.n == used.shape[0]
        Z = forward_rows(b, used)
        got = device_model_percentiles(view, b.ctx, P, 'pa').reshape(3, E, 2, n_freq)
        old = device_model_percentiles(view, b.ctx, P).reshape(3, E, 2, n_freq)
        for e in range(E):
            assert_pa_percentiles(got[:, e], Z[e], f'{what} spectrum {e}')
            np.testing.assert_array_equal(old[:, e], np.percentile(Z[e], P, axis=0))
        (m, s), (mp, sp) = check_moments(view, b.ctx, Z, what)
        # spectra 1, 2, 3 of the five: first_spectrum > 0, n_spectra < E
        sub = view_of(t, discard, thin, E, Wp, 1, 3)
        (m3, s3), (mp3, sp3) = check_moments(sub, b.ctx, Z[1:4], what + ' spectra 1-3', first=1)
        for a3, a5 in ((m3, m), (s3, s), (mp3, mp), (sp3, sp)):       # the plan of 3 spectra is that of 5 here or not:
            if _same_plan(view.n, Wp, 3, E):
                np.testing.assert_array_equal(a3.view(np.uint64), a5[1:4].view(np.uint64))
    b.close()


def _same_plan(n, Wp, E1, E2):
    from bisip_amd import response as rs
    return rs.plan(n, E1, Wp) == rs.plan(n, E2, Wp)


def test_ri_through_the_new_entries_has_the_bits_of_the_old_ones():
    import torch
    b = make_batch('PeltonColeCole', dict(n_modes=2), 32, 64)
    lo, hi = b.param_bounds
    st = torch.cuda.current_stream().cuda_stream
    for rows in (128, 77):                                           # the whole-wave branch and the per-lane one
        th = torch.from_numpy(inside(b.model, lo, hi, (3, rows), seed=rows)).cuda()
        old = torch.full((3, 64, rows), -7.25, dtype=torch.float64, device='cuda')
        new = torch.full((3, 64, rows), -7.25, dtype=torch.float64, device='cuda')
        pa = torch.full((3, 64, rows), -7.25, dtype=torch.float64, device='cuda')
        b.ctx.forward_columns_dev(1, 3, th.data_ptr(), 3 * rows, old.data_ptr(), st)
        b.ctx.forward_columns_kind_dev(1, 3, th.data_ptr(), 3 * rows, new.data_ptr(), 'ri', st)
        b.ctx.forward_columns_kind_dev(1, 3, th.data_ptr(), 3 * rows, pa.data_ptr(), 'pa', st)
        torch.cuda.synchronize()
        assert torch.equal(old, new) and not (old == -7.25).any()
        # the PA columns themselves: the device's hypot / atan2 and glibc's on the same doubles
        from bisip_amd import response as rs
        Z = old.cpu().numpy().reshape(3, 2, 32, rows)                  # column part * N + j of every spectrum
        assert (Z[:, 0] > 0).all()
        want = rs.response_pa(Z.transpose(0, 3, 1, 2)).transpose(0, 2, 3, 1)
        got = pa.cpu().numpy().reshape(3, 2, 32, rows)
        assert (np.abs(got[:, 0] - want[:, 0]) <= (HYPOT_ULP + GLIBC_ULP) * ULP * np.abs(want[:, 0])).all()
        assert (np.abs(got[:, 1] - want[:, 1]) <= (ATAN2_ULP + GLIBC_ULP) * ULP * np.abs(want[:, 1])).all()
        with pytest.raises(ValueError, match='kind'):
            b.ctx.forward_columns_kind_dev(1, 3, th.data_ptr(), 3 * rows, new.data_ptr(), 2, st)
    single = single_context(b, 2)
    theta = inside(b.model, lo, hi, (333,), seed=5)
    np.testing.assert_array_equal(single.forward_percentiles_kind(theta, P, 'ri'), single.forward_percentiles(theta, P))
    assert_pa_percentiles(single.forward_percentiles_kind(theta, P, 'pa'), single.forward(theta), 'forward_percentiles_kind')
    with pytest.raises(ValueError, match='kind'):
        single.forward_percentiles_kind(theta, P, 5)
    with pytest.raises(NotImplementedError):
        b.ctx.forward_percentiles_kind(theta, P, 'pa')
    single.close()
    b.close()


def test_fewer_rows_than_a_wave():
    """40 rows per spectrum: one partial wave of slots, most of them empty."""
    import torch
    b = make_batch('PeltonColeCole', dict(n_modes=1), 20, 8, count=3)
    chain = inside(b.model, *b.param_bounds, (5, 3 * 8), seed=1)
    t = torch.from_numpy(chain).cuda()
    check_moments(view_of(t, 0, 1, 3, 8), b.ctx, forward_rows(b, chain), '5 x 8 rows')
    b.close()


@pytest.mark.parametrize('model,kw,n_freq', [('PeltonColeCole', dict(n_modes=2), 32), ('PolynomialDecomposition', dict(poly_deg=5), 20)],
                         ids=['ColeCole2', 'PD5'])
def test_one_spectrum_in_segments(model, kw, n_freq):
    """E = 1, 50 x 50 = 2500 rows: two whole segments of 1024 and a ragged third; the workspace and the NULL outputs."""
    import torch
    from bisip_amd import response as rs
    b = make_batch(model, kw, n_freq, 50, count=2)
    ctx = single_context(b, 1)                                        # a single-spectrum context
    n, Wp = 50, 50
    assert rs.plan(n, 1, Wp) == (1024, 3, 256)
    chain = inside(model, *b.param_bounds, (n, Wp), seed=n_freq)
    t = torch.from_numpy(chain).cuda()
    view = view_of(t, 0, 1, 1, Wp)
    Z = ctx.forward(chain.reshape(n * Wp, -1))[None]
    (m, s), (mp, sp) = check_moments(view, ctx, Z, f'{model} in three segments')
    nbytes = ctx.response_moments_workspace(n, 1, Wp)
    assert nbytes == 8 * (3 * 4 + 2) * n_freq
    assert ctx.response_moments_workspace(20, 1, Wp) == 0               # 1000 rows: one segment, no workspace
    st = torch.cuda.current_stream().cuda_stream
    work = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.full((2, 2 * n_freq + 8), -7.25, dtype=torch.float64, device='cuda')

    def call(mean, std, work_ptr=work.data_ptr(), work_bytes=nbytes, kind='ri'):
        ctx.response_moments_dev(0, 1, view.ptr, n, view.stride, Wp, kind, mean, std, work_ptr, work_bytes, st)
        torch.cuda.synchronize()

    for bad in (dict(work_bytes=nbytes - 8), dict(work_ptr=0), dict(mean=0, std=0)):
        with pytest.raises(ValueError, match='workspace|neither'):
            call(**dict(dict(mean=out[0].data_ptr(), std=out[1].data_ptr()), **bad))
    assert (out == -7.25).all() and (work == 0xA5).all()                 # refused on the host: nothing launched
    call(out[0].data_ptr(), 0)
    assert (out[1] == -7.25).all() and (out[0, 2 * n_freq:] == -7.25).all()
    np.testing.assert_array_equal(out[0, :2 * n_freq].cpu().numpy().view(np.uint64), m.reshape(-1).view(np.uint64))
    out.fill_(-7.25)
    call(0, out[1].data_ptr())
    assert (out[0] == -7.25).all() and (out[1, 2 * n_freq:] == -7.25).all()
    np.testing.assert_array_equal(out[1, :2 * n_freq].cpu().numpy().view(np.uint64), s.reshape(-1).view(np.uint64))
    assert (work[nbytes:] == 0xA5).all(), 'bytes after the workspace were written'
    ctx.close()
    b.close()


def test_a_parameter_that_is_not_finite_stays_in_its_spectrum():
    import torch
    from bisip_amd import response as rs
    from bisip_amd.summaries import device_model_percentiles
    Wp, n = 50, 30
    b = make_batch('PeltonColeCole', dict(n_modes=2), 32, Wp, count=3)
    chain = inside(b.model, *b.param_bounds, (n, 3 * Wp), seed=9)
    clean = torch.from_numpy(chain).cuda()
    view = view_of(clean, 0, 1, 3, Wp)
    pct = device_model_percentiles(view, b.ctx, P, 'pa').reshape(3, 3, 2, 32)
    mom = {k: rs.device_model_moments(view, b.ctx, k) for k in rs.KINDS}
    for value, column in ((np.nan, 4), (np.inf, 3), (-np.inf, 0)):
        dirty = chain.copy()
        dirty[17, Wp + 23, column] = value                            # sample 17, walker 23 of spectrum 1
        v = view_of(torch.from_numpy(dirty).cuda(), 0, 1, 3, Wp)
        for k in rs.KINDS:
            m, s = rs.device_model_moments(v, b.ctx, k)
            assert not np.isfinite(m[1]).any() and not np.isfinite(s[1]).any()
            for e in (0, 2):
                np.testing.assert_array_equal(m[e].view(np.uint64), mom[k][0][e].view(np.uint64))
                np.testing.assert_array_equal(s[e].view(np.uint64), mom[k][1][e].view(np.uint64))
        if np.isnan(value):
            got = device_model_percentiles(v, b.ctx, P, 'pa').reshape(3, 3, 2, 32)
            assert np.isnan(got[:, 1]).all()
            np.testing.assert_array_equal(got[:, [0, 2]], pct[:, [0, 2]])
    b.close()


# -- through the layers ---------------------------------------------------------------------------------------------
KW = dict(discard=10, thin=3)


@functools.lru_cache(maxsize=None)
def fitted_batch(where):
    import bisip_amd
    files = bisip_amd.DataFiles()
    names = sorted(files)[:3]
    b = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in names], nwalkers=64, nsteps=40, n_modes=1)
    centre = np.array([1.0, 0.3, -6.0, 0.5])
    p0 = centre + 1e-4 * np.random.RandomState(1).randn(3, 64, 4)
    b.fit(p0, seed=6, chain=where)
    return b, names


@pytest.mark.parametrize('where', ['device', 'host'])
def test_model_sampler_and_batch_agree(where):
    import bisip_amd
    from bisip_amd import response as rs
    b, names = fitted_batch(where)
    Eb, Wp, N = 3, 64, b.N
    flat = b.get_chain(flat=True, **KW)                                # (E, n * Wp, ndim)
    n = flat.shape[1] // Wp
    pct = b.get_model_percentile_pa(P, **KW)
    assert pct.shape == (3, Eb, 2, N) and b.get_model_percentile_pa(50, **KW).shape == (1, Eb, 2, N)
    mom = {k: (b.get_model_mean(k, **KW), b.get_model_std(k, **KW)) for k in rs.KINDS}
    assert mom['ri'][0].shape == mom['pa'][1].shape == (Eb, 2, N)
    used = b.get_chain(**KW).reshape(n, Eb * Wp, -1)
    Z = forward_rows(b, used)
    for k in rs.KINDS:
        ref = reference_and_bounds(Z, k, K if k == 'pa' else (0, 0))
        assert_within(mom[k][0], ref, 'mean', f'batch {k}')
        assert_within(mom[k][1], ref, 'std', f'batch {k}')
    assert_same_bits(mom['ri'][0], rs.ordered_response_moments(Z, 'ri')[0], 'batch mean')
    files = bisip_amd.DataFiles()
    for e, name in enumerate(names):
        assert_pa_percentiles(pct[:, e], Z[e], f'batch spectrum {e}')
        m = bisip_amd.PeltonColeCole(files[name], n_modes=1, nwalkers=Wp, nsteps=40)
        np.testing.assert_array_equal(m.get_model_percentile_pa(list(P), chain=flat[e]), pct[:, e])
        assert m.get_model_percentile_pa(50, chain=flat[e]).shape == (2, N)
        for k in rs.KINDS:
            mean, std = m.get_model_mean(chain=flat[e], kind=k), m.get_model_std(chain=flat[e], kind=k)
            assert mean.shape == std.shape == (2, N)
            if rs.plan(n, 1, Wp) == rs.plan(n, Eb, Wp):              # (one segment each here)
                np.testing.assert_array_equal(mean.view(np.uint64), mom[k][0][e].view(np.uint64))
                np.testing.assert_array_equal(std.view(np.uint64), mom[k][1][e].view(np.uint64))
            ref = reference_and_bounds(Z[e:e + 1], k, K if k == 'pa' else (0, 0))
            assert_within(mean[None], ref, 'mean', f'model {k}')
            assert_within(std[None], ref, 'std', f'model {k}')
    assert rs.plan(n, 1, Wp)[1] == 1
    with pytest.raises(ValueError):
        b.get_model_mean('ri', discard=40)
    with pytest.raises(ValueError, match="'ri' or 'pa'"):
        b.get_model_std('amp')


@pytest.mark.parametrize('where', ['device', 'host'])
def test_fitted_model_methods(where):
    import bisip_amd
    from bisip_amd import response as rs
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=32, nsteps=60)
    np.random.seed(4)
    p0 = np.array([1.0, 0.005, -0.003, -0.001]) + 1e-4 * np.random.RandomState(2).randn(32, 4)      # Re Z > 0 from the start
    m.fit(p0=p0, chain=where)
    flat = m.get_chain(flat=True, **KW)
    Z = m._context().forward(np.ascontiguousarray(flat))
    with pytest.warns(UserWarning, match='No samples were discarded'):
        assert m.get_model_percentile_pa().shape == (3, 2, m._context().N)
    pct = m.get_model_percentile_pa(list(P), **KW)
    assert_pa_percentiles(pct, Z, f'model, chain={where}')
    np.testing.assert_array_equal(pct, m.get_model_percentile_pa(list(P), chain=flat))
    np.testing.assert_array_equal(m.get_model_percentile_pa(50, **KW), m.get_model_percentile_pa([50], **KW)[0])
    for k in rs.KINDS:
        mean, std = m.get_model_mean(kind=k, **KW), m.get_model_std(kind=k, **KW)
        np.testing.assert_array_equal(mean.view(np.uint64), m.get_model_mean(chain=flat, kind=k).view(np.uint64))
        np.testing.assert_array_equal(std.view(np.uint64), m.get_model_std(chain=flat, kind=k).view(np.uint64))
        ref = reference_and_bounds(Z[None], k, K if k == 'pa' else (0, 0))
        assert_within(mean[None], ref, 'mean', f'model {k} {where}')
        assert_within(std[None], ref, 'std', f'model {k} {where}')
    assert_same_bits(m.get_model_mean(**KW)[None], rs.ordered_response_moments(Z, 'ri')[0], 'model mean')
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_model_std(chain=flat, discard=3)
    with pytest.raises(NotImplementedError, match='plotting'):
        m.plot_fit()


def test_unfitted_batch_and_argument_checks():
    """Every refused call below is refused on the host before anything is launched: the pointers are never dereferenced."""
    b = make_batch('PeltonColeCole', dict(n_modes=1), 20, 8, count=2)
    for call in (b.get_model_percentile_pa, b.get_model_mean, b.get_model_std):
        with pytest.raises(AssertionError, match='not fitted'):
            call()
    ctx = b.ctx
    ok = dict(first=0, count=1, chain=4096, n=8, stride=2 * 8 * 4, Wp=8, kind='ri', mean=4096, std=4096, work=4096, nbytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        ctx.response_moments_dev(a['first'], a['count'], a['chain'], a['n'], a['stride'], a['Wp'], a['kind'], a['mean'],
                                 a['std'], a['work'], a['nbytes'], 0)

    with pytest.raises(ValueError, match='kind'):
        call(kind=2)
    with pytest.raises(ValueError, match='neither'):
        call(mean=0, std=0)
    with pytest.raises(ValueError, match='null'):
        call(chain=0)
    with pytest.raises(ValueError, match='spectra'):
        call(first=2)
    with pytest.raises(ValueError, match='bad chain shape'):
        call(count=3)
    with pytest.raises(ValueError, match='sample_stride'):
        call(stride=31)
    with pytest.raises(ValueError, match='workspace'):
        call(n=300, work=0)                                   # 2400 rows: three segments
    with pytest.raises(ValueError, match='workspace'):
        call(n=300, nbytes=8)
    assert ctx.response_moments_workspace(8, 1, 8) == 0
    assert ctx.response_moments_workspace(300, 1, 8) == 8 * (3 * 4 + 2) * ctx.N
    assert ctx.response_moments_workspace(0, 1, 8) < 0 and ctx.response_moments_workspace(8, 3, 8) < 0
    b.close()
