"""The ordering of Cole-Cole modes and the per-mode descriptors of device-resident chains (bisip_mode_order_dev;
bisip_amd.modes).  Two claims are kept apart: that the row function does what the definition says is tests/test_modes.py's, on
the CPU, for the host entry point; that the kernel runs that row function is checked here, bit for bit against the host entry
point on ``ordered``, ``moved`` and ``m_total`` (the two relaxation times pass through the device's log1p: they are held to the
long-double yardstick within the bound of tests/mode_bounds.py).  The model and SpectraBatch methods are then held to the NumPy
definitions on a get_chain copy: the ordered chain is a permutation, so its percentiles and HDI are those of the same doubles
uploaded; means and stds with the allowances tests/test_gpu_relaxation.py uses (MOMENT_TOL relative to max(1, |value|), rtol
STD_RTOL, each plus the largest bound of the column)."""
import functools
import itertools
import math

import numpy as np
import pytest

import mode_bounds as mb
from chain_harness import GuardedCall, store
from test_modes import BYS, KS, bits, hostile_rows, same_bits_or_nan, tied_rows

pytestmark = pytest.mark.gpu

MOMENT_TOL = 1e-12
STD_RTOL = 1e-9
COMBOS = [c for c in itertools.product((False, True), repeat=3) if any(c)]


def device_rows(t, off, stride, n, E, Wp, K, by, asked=(True, True, True)):
    """bisip_mode_order_dev on the samples of a device tensor, guards behind every output, the ones not asked for untouched:
    (ordered, desc, moved), None where not asked for."""
    import torch
    from bisip_amd import _hip, modes
    call = GuardedCall()
    o = call.out('the ordered rows', (n, E * Wp, 1 + 3 * K), asked=asked[0])
    d = call.out('the descriptors', (n, E * Wp, 1 + 2 * K), asked=asked[1])
    mv = call.out('moved', (n, E * Wp), dtype=torch.uint8, fill=9, asked=asked[2])
    _hip.mode_order_dev(t.data_ptr() + 8 * off, n, stride, E, Wp, K, modes.KEY_GROUPS[by], o, d, mv, call.stream)
    return [r if a else None for r, a in zip(call.finish(), asked)]


@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (1, 257)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('K', KS)
def test_device_equals_the_host_entry_point(K, shape):
    """Rows per sample 1, 15 (3 ensembles of 5 walkers) and 257 (one row into a second workgroup), 3 and 9 samples, behind an
    offset, a stride and padding, hostile keys among the rows, every key group and every combination of asked outputs."""
    import torch
    from bisip_amd import _hip, modes
    E, Wp = shape
    for n in (3, 9):
        for by in BYS:
            g = modes.KEY_GROUPS[by]
            total = n * E * Wp
            x = np.concatenate([hostile_rows(K, by), tied_rows(np.random.default_rng([K, g, n]), total, K)])[:total]
            x = x.reshape(n, E * Wp, 1 + 3 * K)
            stored, off, stride = store(x, filler=np.nan)
            t = torch.from_numpy(stored).cuda()
            wo, wd, wm = _hip.mode_order_host(stored, n, stride, E, Wp, K, g, offset=off)
            for asked in COMBOS:
                o, d, mv = device_rows(t, off, stride, n, E, Wp, K, by, asked)
                what = f'K={K} {E}x{Wp} n={n} by {by} asked {asked}'
                if o is not None:
                    np.testing.assert_array_equal(bits(o), bits(wo), err_msg=what)
                if mv is not None:
                    np.testing.assert_array_equal(mv, wm.astype(np.uint8), err_msg=what)
                if d is not None:
                    same_bits_or_nan(d[..., 0], wd[..., 0])
                    np.testing.assert_array_equal(np.isnan(d), np.isnan(wd), err_msg=what)
                    np.testing.assert_array_equal(np.isfinite(d), np.isfinite(wd), err_msg=what)
            assert K == 1 or total < 8 or (wm.any() and not wm.all())


@pytest.mark.parametrize('K', KS)
def test_relaxation_times_within_the_bound(K):
    """log_tau_cc and log_tau_peak of the device against the long-double yardstick, rows of the box and rows at its edges."""
    import torch
    for name, rows in mb.families(K, 20000 // K, seed=1).items():
        t = torch.from_numpy(rows[None]).cuda()
        for by in BYS:
            o, d, mv = device_rows(t, 0, rows.size, 1, 1, rows.shape[0], K, by)
            worst = mb.assert_within(d[0], rows, K, by, f'device K={K} {name} by {by}')
        print(f'K={K} {name}: the device uses {worst:.3f} of the bound')


def test_more_samples_than_one_grid_column():
    """65,537 samples of 3 rows, K = 1: the kernel's sample loop goes beyond the 65,535 blocks of the grid's y."""
    import torch
    from bisip_amd.chainview import ChainView
    from bisip_amd.modes import device_mode_order, host_mode_order
    n = 65537
    chain = mb.box_rows(np.random.default_rng(65), n * 3, 1).reshape(n, 3, 4)
    o, d, mv = device_mode_order(ChainView(torch.from_numpy(chain).cuda(), n, 3, 1, 4), 1, moved=True)
    wo, wd, wm = host_mode_order(chain, 1, n_ensembles=3)
    np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(wo))
    np.testing.assert_array_equal(bits(d.cpu().numpy()[..., 0]), bits(wd[..., 0]))
    assert not mv.cpu().numpy().any() and not wm.any()
    mb.assert_within(d.cpu().numpy().reshape(-1, 3), chain.reshape(-1, 4), 1)


def test_box_edges_propagate_into_the_summaries():
    """A used sample with m = 1 (or c = 0) gives -inf (or NaN) in its descriptors: the mean of its ensemble is that, as NumPy's
    is, and no other ensemble's."""
    import torch
    from bisip_amd.chainview import ChainView, device_moments, device_percentiles
    from bisip_amd.modes import device_mode_order, mode_descriptors
    n, Wp = 20, 16
    chain = mb.box_rows(np.random.default_rng(9), n * 3 * Wp, 2).reshape(n, 3 * Wp, 7)
    chain[3, Wp + 2, 1] = 1.0                 # ensemble 1: m_1 = 1
    chain[4, 2 * Wp + 1, [1, 5]] = 0.0        # ensemble 2: m_1 = 0 and c_1 = 0
    view = ChainView(torch.from_numpy(chain).cuda(), n, 3, Wp, 7)
    d = view.derived(device_mode_order(view, 2, 'm', ordered=False)[1])
    want = mode_descriptors(chain, 2, 'm')
    np.testing.assert_array_equal(np.isnan(d.tensor.cpu().numpy()), np.isnan(want))
    np.testing.assert_array_equal(np.isneginf(d.tensor.cpu().numpy()), np.isneginf(want))
    mean, std = device_moments(d)
    pct = device_percentiles(d, [50.0])[0]
    assert np.isfinite(mean[0]).all() and np.isfinite(std[0]).all() and np.isfinite(pct[0]).all()
    with np.errstate(invalid='ignore'):
        wmean = want.reshape(n, 3, Wp, 5).transpose(1, 0, 2, 3).reshape(3, -1, 5).mean(axis=1)
    assert np.isneginf(wmean[1]).any() and np.isnan(wmean[2]).any()
    np.testing.assert_array_equal(np.isneginf(mean), np.isneginf(wmean))
    np.testing.assert_array_equal(np.isnan(mean), np.isnan(wmean))


# -- a real label-switching run, the methods and the evidence -------------------------------------------------------------------
TRUTH = np.array([1.0, 0.15, 0.5, -1.5, -12.0, 0.45, 0.6])
SWAP = [0, 2, 1, 4, 3, 6, 5]
STEPS, DISCARD, WP = 600, 300, 32


def starts(rng, shape):
    """Walkers near the truth of bisip_amd.synthetic, the odd ones with the two modes exchanged."""
    p0 = TRUTH + 1e-3 * rng.standard_normal(shape + (7,))
    p0[..., 1::2, :] = p0[..., 1::2, :][..., SWAP]
    return p0


@functools.lru_cache(maxsize=None)
def spectrum_files():
    import tempfile
    from bisip_amd.synthetic import write_spectrum_file
    spectrum_files.directory = tempfile.TemporaryDirectory(prefix='bisip_modes_')      # removed when the interpreter ends
    return tuple(write_spectrum_file(f'{spectrum_files.directory.name}/two_modes_{i}.csv', 20, i) for i in range(3))


@functools.lru_cache(maxsize=None)
def fitted_model(where):
    import bisip_amd
    m = bisip_amd.PeltonColeCole(spectrum_files()[0], n_modes=2, nwalkers=WP, nsteps=STEPS)
    np.random.seed(31)
    m.fit(p0=starts(np.random.default_rng(4), (WP,)), chain=where)
    return m


@functools.lru_cache(maxsize=None)
def fitted_batch(where):
    import bisip_amd
    b = bisip_amd.SpectraBatch('PeltonColeCole', list(spectrum_files()), nwalkers=WP, nsteps=STEPS, n_modes=2)
    b.fit(starts(np.random.default_rng(5), (3, WP)), seed=6, chain=where)
    return b


def check_against_definitions(flat, ordered, desc, mean_o, std_o, mean_d, std_d, by):
    """Per-ensemble rows ``flat (R, 7)``: the device's ordered rows and descriptors and their means and stds."""
    from bisip_amd import modes
    wo = modes.order_modes(flat, 2, by)
    np.testing.assert_array_equal(bits(ordered), bits(wo))
    mb.assert_within(desc, flat, 2, by)
    values, bound = mb.yardstick(flat, 2, by)
    for got_m, got_s, want, b in ((mean_o, std_o, wo, 0.0), (mean_d, std_d, values.astype(np.float64), bound.max(axis=0).astype(np.float64))):
        m_np, s_np = want.mean(axis=0), want.std(axis=0)
        assert np.all(np.abs(got_m - m_np) <= MOMENT_TOL * np.maximum(1.0, np.abs(m_np)) + b), (got_m, m_np)
        assert np.all(np.abs(got_s - s_np) <= STD_RTOL * np.abs(s_np) + b), (got_s, s_np)


def uploaded(chain3, E):
    import torch
    from bisip_amd.chainview import ChainView
    n, rows, ndim = chain3.shape
    return ChainView(torch.from_numpy(np.ascontiguousarray(chain3)).cuda(), n, E, rows // E, ndim)


def test_model_methods_on_a_label_switching_run():
    from bisip_amd import modes
    from bisip_amd.chainview import device_percentiles
    from bisip_amd.interval import device_hdi
    out = {}
    for where in ('device', 'host'):
        m = fitted_model(where)
        kw = dict(discard=DISCARD, thin=2)
        out[where] = [m.get_chain(**kw), m.get_ordered_chain(**kw), m.get_ordered_chain(flat=True, **kw), m.get_mode_chain(**kw),
                      m.get_ordered_mean(**kw), m.get_ordered_std(**kw), m.get_ordered_percentile(**kw), m.get_ordered_hdi(0.9, **kw),
                      m.get_mode_mean(**kw), m.get_mode_std(**kw), m.get_mode_percentile(50, **kw), m.get_mode_hdi([0.5, 0.9], **kw),
                      m.get_mode_switch_rate(**kw), m.get_ordered_std(by='m', **kw)]
    for a, c in zip(out['device'], out['host']):
        np.testing.assert_array_equal(bits(a), bits(c))
    ch, oc, oflat, dc, omean, ostd, opct, ohdi, dmean, dstd, dp50, dhdi, rate, _ = out['device']
    n = (STEPS - DISCARD) // 2
    assert ch.shape == oc.shape == (n, WP, 7) and oflat.shape == (n * WP, 7) and dc.shape == (n, WP, 5)
    assert omean.shape == ostd.shape == (7,) and opct.shape == (3, 7) and ohdi.shape == (2, 7)
    assert dmean.shape == dstd.shape == dp50.shape == (5,) and dhdi.shape == (2, 2, 5) and rate.shape == (WP,)
    flat = ch.reshape(-1, 7)
    check_against_definitions(flat, oflat, dc.reshape(-1, 5), omean, ostd, dmean, dstd, 'log_tau')
    # the same doubles uploaded: the same percentiles and the same interval
    v = uploaded(modes.order_modes(ch, 2), 1)
    np.testing.assert_array_equal(bits(opct), bits(device_percentiles(v, [2.5, 50, 97.5])[:, 0]))
    np.testing.assert_array_equal(bits(ohdi), bits(device_hdi(v, 0.9)[..., 0, :]))
    np.testing.assert_allclose(opct, np.percentile(modes.order_modes(flat, 2), [2.5, 50, 97.5], axis=0), rtol=1e-14, atol=0)
    # the walkers keep the labelling they started in, half of them each: the rate is strictly between 0 and 1
    want_rate = modes.modes_moved(ch, 2).mean(axis=0)
    np.testing.assert_array_equal(rate, want_rate)
    assert 0 < rate.mean() < 1 and np.all((rate >= 0) & (rate <= 1))
    assert np.all(oflat[:, 3] <= oflat[:, 4])                                     # every ordered sample
    m = fitted_model('device')
    unordered = m.get_param_std(**kw)
    assert ostd[3] < unordered[3] and ostd[4] < unordered[4], (ostd, unordered)
    print('switch rate', rate.mean(), 'ordered log_tau std', ostd[3:5], 'unordered', unordered[3:5], 'descriptors', dmean)
    # a chain= array of whole samples is summarised as the fitted chain is; discard beside it is refused
    np.testing.assert_array_equal(bits(m.get_ordered_mean(chain=flat)), bits(omean))
    np.testing.assert_array_equal(bits(m.get_mode_chain(chain=flat)), bits(dc.reshape(-1, 5)))
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_mode_mean(chain=flat, thin=2)
    np.testing.assert_array_equal(bits(m.mode_descriptors(flat)), bits(modes.mode_descriptors(flat, 2)))


def test_batch_methods():
    from bisip_amd import modes
    from bisip_amd.chainview import device_percentiles
    from bisip_amd.interval import device_hdi
    out = {}
    for where in ('device', 'host'):
        b = fitted_batch(where)
        a = (DISCARD, 2)
        out[where] = [b.get_chain(*a), b.get_ordered_chain(*a), b.get_ordered_chain(*a, flat=True), b.get_mode_chain(*a, flat=True),
                      b.get_ordered_mean(*a), b.get_ordered_std(*a), b.get_ordered_percentile((2.5, 50, 97.5), *a),
                      b.get_ordered_hdi(0.9, *a), b.get_mode_mean(*a), b.get_mode_std(*a), b.get_mode_percentile(50, *a),
                      b.get_mode_hdi(0.9, *a), b.get_mode_switch_rate('log_tau', *a), b.get_mode_mean(*a, by='c')]
    for x, y in zip(out['device'], out['host']):
        np.testing.assert_array_equal(bits(x), bits(y))
    ch, oc, oflat, dflat, omean, ostd, opct, ohdi, dmean, dstd, dp50, dhdi, rate, _ = out['device']
    n, E = (STEPS - DISCARD) // 2, 3
    assert ch.shape == oc.shape == (n, E, WP, 7) and oflat.shape == (E, n * WP, 7) and dflat.shape == (E, n * WP, 5)
    assert omean.shape == ostd.shape == (E, 7) and opct.shape == (3, E, 7) and ohdi.shape == (2, E, 7)
    assert dmean.shape == dstd.shape == dp50.shape == (E, 5) and dhdi.shape == (2, E, 5) and rate.shape == (E, WP)
    flat = ch.transpose(1, 0, 2, 3).reshape(E, n * WP, 7)
    for e in range(E):
        check_against_definitions(flat[e], oflat[e], dflat[e], omean[e], ostd[e], dmean[e], dstd[e], 'log_tau')
    v = uploaded(modes.order_modes(ch, 2).reshape(n, E * WP, 7), E)
    np.testing.assert_array_equal(bits(opct), bits(device_percentiles(v, [2.5, 50, 97.5])))
    np.testing.assert_array_equal(bits(ohdi), bits(device_hdi(v, 0.9)))
    np.testing.assert_array_equal(rate, modes.modes_moved(ch, 2).mean(axis=0))
    assert np.all((0 < rate.mean(axis=1)) & (rate.mean(axis=1) < 1)) and np.all(oflat[..., 3] <= oflat[..., 4])
    b = fitted_batch('device')
    np.testing.assert_array_equal(b.mode_descriptors(flat[:, :40]), modes.mode_descriptors(flat[:, :40], 2))


def ordered_check(res, raw, chain, logp, log_prob_fn, bounds, what):
    """The device's estimate over one labelling against bridge_evidence(order=...) on the copied chain with the kept draws,
    within the first-order bound of tests/test_gpu_evidence.py (check_against_numpy: it restates the estimate from the samples
    and a log-probability, so it gets the samples in order and the log-probability that refuses the draws that are not -- what
    ``order=`` does, tests/test_modes.py)."""
    from bisip_amd import evidence as ev, modes
    from test_gpu_evidence import check_against_numpy
    assert res['log_symmetry'] == math.log(2) == raw['log_symmetry']
    kept = {k: raw[k] for k in ('theta2', 'logg2', 'logp2')}
    one = dict(raw, log_ml=raw['log_ml'] - raw['log_symmetry'])
    refused = lambda t: np.where(modes.modes_moved(t, 2), -np.inf, log_prob_fn(t))
    host = check_against_numpy(one, kept, modes.order_modes(chain, 2), logp, refused, bounds, what)
    direct = ev.bridge_evidence(chain, logp, log_prob_fn, bounds, neff=raw['neff'], use_all=False, order=(2, 'log_tau'),
                                proposal=(raw['proposal_mean'], raw['proposal_cov']), draws=(raw['theta2'], raw['logg2']))
    assert direct['log_ml'] == host['log_ml'] + math.log(2) and direct['log_symmetry'] == math.log(2)
    assert direct['frac_outside'] == raw['frac_outside'] and raw['iterations'] < ev.MAXITER
    assert np.mean(modes.modes_moved(raw['theta2'], 2)) <= raw['frac_outside']


def test_get_evidence_over_one_labelling():
    from bisip_amd import evidence as ev
    m = fitted_model('device')
    s = m._sampler
    KW = dict(discard=DISCARD, thin=1)
    res = m.get_evidence(seed=5, order_modes='log_tau', **KW)
    assert list(res)[-1] == 'log_symmetry' and len(res) == 13 and res['iterations'] < ev.MAXITER
    lo, hi = m.param_bounds
    assert res['log_evidence'] == res['log_ml'] - float(np.log(hi - lo).sum())
    raw = ev.device_evidence(s.used_samples_dev(**KW), s.log_prob_samples_dev(**KW), s.backend.ctx, seed=5, keep_draws=True,
                             order=(2, 'log_tau'))
    assert raw['log_ml'][0] == res['log_ml']
    one = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
    ordered_check(res, one, m.get_chain(**KW), s.get_log_prob(**KW), m.log_prob, m.param_bounds, 'two modes, one labelling')
    plain = m.get_evidence(seed=5, **KW)
    assert 'log_symmetry' not in plain and len(plain) == 12
    print(f'ordered {res["log_ml"]:.4f} +- {res["se"]:.1e} in {res["iterations"]} passes; mixed labellings {plain["log_ml"]:.4f} +- '
          f'{plain["se"]:.1e} in {plain["iterations"]} passes')


def test_batch_evidence_over_one_labelling():
    import bisip_amd
    from bisip_amd import evidence as ev
    b = fitted_batch('device')
    KW = dict(discard=DISCARD, thin=1)
    res = b.get_evidence(seed=9, order_modes='log_tau', **KW)
    assert res['log_symmetry'] == math.log(2) and res['log_ml'].shape == (3,) and np.all(res['iterations'] < ev.MAXITER)
    raw = b._fitted().evidence(seed=9, keep_draws=True, order=(2, 'log_tau'), **KW)
    np.testing.assert_array_equal(raw['log_ml'], res['log_ml'])
    chain, logp = b.get_chain(**KW), b.get_log_prob(**KW)
    for e in range(3):
        one = {k: (v[e] if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
        lone = bisip_amd.PeltonColeCole(spectrum_files()[e], n_modes=2, nwalkers=WP, nsteps=5)
        ordered_check(dict(log_symmetry=res['log_symmetry']), one, np.ascontiguousarray(chain[:, e]),
                      np.ascontiguousarray(logp[:, e]), lone.log_prob, b.param_bounds, f'spectrum {e}')
