"""The relaxation descriptors of device-resident chains (bisip_rtd_descriptors_dev: the RTD's peak and the cumulative
relaxation times; bisip_amd.decomposition, "Relaxation descriptors").  Two claims are kept apart: that the arithmetic
meets its bound is tests/test_relaxation.py's, on the CPU, for the host entry point; that the kernel does that arithmetic
is checked here, bit for bit against the host entry point.  The model and SpectraBatch methods are then held to NumPy on
the long-double yardstick (tests/relaxation_bounds.py) with the allowances tests/test_gpu_decomposition.py uses for the
integrating parameters, restated: MOMENT_TOL relative to max(1, |value|) for the mean, rtol STD_RTOL for the std, each
plus the largest bound of the column; a percentile is 1-Lipschitz in the max-norm of its column, so it may move by the
largest bound of the column plus 4u of its value.  The bound of a fragile entry (relaxation_bounds) is the width of the
grid, which holds because it lies inside; of a fragile m_peak the largest bound of the row's m_l."""

import functools

import numpy as np
import pytest

from chain_harness import GuardedCall, store
from relaxation_bounds import descriptor_bounds, descriptors_yardstick
from test_decomposition import DEBYE_TUTORIAL, U, bounds, grid, prior_rows, tutorial_rows

pytestmark = pytest.mark.gpu

MOMENT_TOL = 1e-12
STD_RTOL = 1e-9
Q_SETS = {1: [1.0], 3: [0.1, 0.5, 0.9], 8: [0.01, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0]}
P_MANY = [0, 1, 2.5, 10, 25, 37.5, 50, 62.5, 75, 90, 97.5, 99, 100]      # more than 8: the sort path
GRIDS = {1: np.array([-2.5]), 2: np.array([-6.0, 2.0]), 40: grid(40), 64: grid(64, -7.0, 3.0)}
E, WP, N = 3, 100, 5               # 300 rows a sample: a whole 256-thread block and a part of a second


def same_bits(got, want, what=''):
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64), err_msg=what)


def device_rows(t, off, stride, n, n_ensembles, Wp, ndim, lt, q):
    """bisip_rtd_descriptors_dev on the samples of a device tensor, guards behind the output: (n, E * Wp, 2 + J)."""
    import torch
    from bisip_amd import _hip
    d_lt = torch.from_numpy(np.ascontiguousarray(lt, dtype=np.float64)).cuda()
    d_q = torch.from_numpy(np.asarray(q, dtype=np.float64)).cuda()
    call = GuardedCall()
    out = call.out('the descriptors', (n, n_ensembles * Wp, 2 + len(q)))
    _hip.rtd_descriptors_dev(t.data_ptr() + 8 * off, n, stride, n_ensembles, Wp, ndim, d_lt.data_ptr(), len(lt),
                             d_q.data_ptr(), len(q), out, call.stream)
    return call.finish()[0]


def stored_chain(rows, ndim):
    """Rows as a chain (N, E * WP, ndim) behind an offset, a stride of two samples and padding, on both sides."""
    import torch
    stored, off, stride = store(rows.reshape(N, E * WP, ndim))
    return stored, torch.from_numpy(stored).cuda(), off, stride


def hostile(rows, P):
    """Prior-box rows with a NaN coefficient, a row that overflows and a row with no positive RTD among them."""
    rows = rows.copy()
    rows[7, 1 + P // 2] = np.nan
    rows[11, 1 + P] = 1e308 if P else np.inf
    rows[13, 1:] = -np.abs(rows[13, 1:])
    rows[13, 2::2] = 0.0                                  # even powers only, all <= 0: m_l <= 0
    return rows


@pytest.mark.parametrize('L', sorted(GRIDS))
@pytest.mark.parametrize('P', [0, 1, 4, 5, 14])
def test_device_equals_the_host_entry_point(P, L):
    from bisip_amd import _hip
    ndim, lt = P + 2, GRIDS[L]
    rows = hostile(prior_rows(np.random.default_rng(100 * P + L), N * E * WP, P), P)
    stored, t, off, stride = stored_chain(rows, ndim)
    nan_rows = 0
    for J, q in Q_SETS.items():
        want = _hip.rtd_descriptors_host(stored, N, stride, E, WP, ndim, lt, q, offset=off)
        got = device_rows(t, off, stride, N, E, WP, ndim, lt, q)
        assert got.shape == (N, E * WP, 2 + J)
        same_bits(got, want, f'P={P} L={L} J={J}')
        nan = np.isnan(got)
        assert np.all(nan.all(axis=-1) == nan.any(axis=-1))          # a row is NaN throughout or nowhere
        nan_rows = int(nan[..., 0].sum())
    assert 3 <= nan_rows < N * E * WP                                  # real NaN rows, and not only those


def test_device_equals_the_host_entry_point_on_tutorial_rows():
    from bisip_amd import _hip
    rows = tutorial_rows(np.random.default_rng(6), N * E * WP)
    stored, t, off, stride = stored_chain(rows, 6)
    for L in (40, 64):
        for J, q in Q_SETS.items():
            want = _hip.rtd_descriptors_host(stored, N, stride, E, WP, 6, GRIDS[L], q, offset=off)
            same_bits(device_rows(t, off, stride, N, E, WP, 6, GRIDS[L], q), want, f'L={L} J={J}')
            assert np.isfinite(want).all()


@pytest.mark.parametrize('P', [1, 4, 5])
def test_peak_is_the_largest_of_the_rtd_columns(P):
    """m_peak and log_tau_peak are the max and x[argmax] (the first) of bisip_rtd_columns_dev's m_l, bit for bit."""
    from test_gpu_decomposition import chain_columns
    lt = GRIDS[40]
    rows = prior_rows(np.random.default_rng(P), N * E * WP, P)
    _, t, off, stride = stored_chain(rows, P + 2)
    got = device_rows(t, off, stride, N, E, WP, P + 2, lt, Q_SETS[3])          # (N, E * WP, 5)
    cols = chain_columns(t, N, off, stride, E, WP, P + 2, lt)                   # (E, L, N * WP), rows s * WP + w
    m = cols.reshape(E, 40, N, WP).transpose(2, 0, 3, 1).reshape(N, E * WP, 40)
    ok = ~np.isnan(got[..., 0])
    np.testing.assert_array_equal(ok, np.any(m > 0, axis=-1))
    same_bits(got[..., 1][ok], m.max(axis=-1)[ok])
    same_bits(got[..., 0][ok], lt[m.argmax(axis=-1)][ok])


def test_more_samples_than_one_grid_column():
    """70,000 samples of 2 x 1 walkers: the kernel's sample loop goes beyond the 65,535 blocks of the grid's y."""
    import torch
    from bisip_amd.chainview import ChainView
    from bisip_amd.decomposition import device_rtd_descriptors, host_rtd_descriptors
    n, P = 70000, 4
    chain = prior_rows(np.random.default_rng(70), n * 2, P).reshape(n, 2, P + 2)
    t = torch.from_numpy(chain).cuda()
    got = device_rtd_descriptors(ChainView(t, n, 2, 1, P + 2), GRIDS[40], Q_SETS[3]).cpu().numpy()
    same_bits(got, host_rtd_descriptors(chain, GRIDS[40], Q_SETS[3], n_ensembles=2))


def test_nan_rows_make_nan_summaries():
    """A used sample with no positive RTD is a NaN row of the derived chain: mean, std, percentiles and HDI of its
    ensemble are NaN, as NumPy's are, and no other ensemble's."""
    import torch
    from bisip_amd.chainview import ChainView, device_moments, device_percentiles
    from bisip_amd.decomposition import device_rtd_descriptors
    from bisip_amd.interval import device_hdi
    n, Wp = 20, 16
    chain = tutorial_rows(np.random.default_rng(9), n * 2 * Wp).reshape(n, 2 * Wp, 6)
    chain[3, Wp + 2, 1:] = [-1.0, 0.0, 0.0, 0.0, 0.0]                # ensemble 1 only
    view = ChainView(torch.from_numpy(chain).cuda(), n, 2, Wp, 6)
    d = view.derived(device_rtd_descriptors(view, GRIDS[40], Q_SETS[3]))
    mean, std = device_moments(d)
    for out in (mean, std, device_percentiles(d, [2.5, 50, 97.5]), device_percentiles(d, P_MANY), device_hdi(d, 0.9)):
        assert np.isfinite(out[..., 0, :]).all() and np.isnan(out[..., 1, :]).all()


# -- the methods of the model and of SpectraBatch ------------------------------------------------------------------------
def yardstick_of(chain, lt, q):
    """Long-double values (..., K) of a chain (..., ndim) and the bound of every entry (module docstring)."""
    flat = chain.reshape(-1, chain.shape[-1])
    ys = descriptors_yardstick(flat, lt, q)
    bound, fragile = descriptor_bounds(flat, lt, q, ys)
    bound = bound.copy()
    times = np.ones(bound.shape[1], dtype=bool)
    times[1] = False
    bound[:, times] = np.where(fragile[:, times], lt[-1] - lt[0], bound[:, times])
    bound[:, 1] = np.where(fragile[:, 1], bounds(flat, lt, 1.0)[1].max(axis=1), bound[:, 1])
    K = bound.shape[1]
    return ys['values'].reshape(chain.shape[:-1] + (K,)), bound.reshape(chain.shape[:-1] + (K,)), fragile


def check_rows(got, want, bound, fragile, lt):
    """Per-sample values: the yardstick's NaN pattern, held entries within their bound, fragile ones inside the grid."""
    K = got.shape[-1]
    g, w, b = got.reshape(-1, K), want.reshape(-1, K), bound.reshape(-1, K)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert np.all(np.abs(g.astype(np.longdouble) - w)[ok] <= b[ok])
    assert fragile.mean() <= 0.01


def check_summaries(flat_want, flat_bound, mean, std, pct, p):
    """Device mean / std / percentiles of a derived chain against NumPy's on the long-double yardstick rounded to
    float64; flat_* (rows, K).  A column with a NaN row is NaN in both."""
    want = flat_want.astype(np.float64)
    bmax = np.max(flat_bound, axis=0).astype(np.float64)
    with np.errstate(invalid='ignore'):
        m_np, s_np, pw = want.mean(axis=0), want.std(axis=0), np.percentile(want, p, axis=0)
    for got, ref in ((mean, m_np), (std, s_np), (pct, pw)):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(m_np)
    assert np.all(np.abs(mean - m_np)[ok] <= (MOMENT_TOL * np.maximum(1.0, np.abs(m_np)) + bmax)[ok]), (mean, m_np)
    assert np.all(np.abs(std - s_np)[ok] <= (STD_RTOL * np.abs(s_np) + bmax)[ok]), (std, s_np)
    assert np.all(np.abs(pct - pw)[:, ok] <= (bmax + 4 * U * np.abs(pw))[:, ok]), (pct, pw)


def batch_spectra():
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    files = bisip_amd.DataFiles()
    return [files[k] for k in sorted(DEBYE_TUTORIAL)] + [synthetic_columns(20, i) for i in range(4)]


def batch_outputs(b, discard, thin, q):
    return [b.get_relaxation_chain(discard, thin, q=q), b.get_relaxation_chain(discard, thin, flat=True, q=q),
            b.get_relaxation_mean(discard, thin, q=q), b.get_relaxation_std(discard, thin, q=q),
            b.get_relaxation_percentile([2.5, 50, 97.5], discard, thin, q=q), b.get_relaxation_percentile(50, discard, thin, q=q),
            b.get_relaxation_hdi(0.9, discard, thin, q=q), b.get_relaxation_hdi([0.5, 0.9], discard, thin, q=q)]


def test_batch_methods():
    """Ten spectra (the six bundled ones and four synthetic), 32 walkers, 300 steps: shapes, device chain and host chain
    bit for bit, the chain against the host entry point and the yardstick, the summaries against device_moments /
    device_percentiles / device_hdi of the derived chain and against NumPy on the yardstick."""
    import torch
    import bisip_amd
    from bisip_amd.chainview import ChainView, device_moments, device_percentiles
    from bisip_amd.decomposition import device_rtd_descriptors, host_rtd_descriptors, rtd_descriptors
    from bisip_amd.interval import device_hdi
    spectra = batch_spectra()
    n_spectra, Wp, discard, thin, q = len(spectra), 32, 100, 2, Q_SETS[3]
    out = {}
    for where in ('device', 'host'):
        b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=Wp, nsteps=300, poly_deg=4)
        np.random.seed(8)
        b.fit(seed=9, chain=where)
        out[where] = (b.get_chain(discard, thin), batch_outputs(b, discard, thin, q), b.log_tau.copy())
        if where == 'device':
            many = b.get_relaxation_percentile(P_MANY, discard, thin)
            eight = b.get_relaxation_chain(discard, thin, q=Q_SETS[8])
            # the host method: the module's definition on the shared grid
            theta = b.get_chain(discard, thin, flat=True)[:, :50]
            host = b.relaxation_descriptors(theta, q=q)
            assert host.shape == (n_spectra, 50, 5)
            np.testing.assert_array_equal(host[3], rtd_descriptors(theta[3], b.log_tau, q))
        b.close()
    np.testing.assert_array_equal(out['device'][0], out['host'][0])
    for a, c in zip(out['device'][1], out['host'][1]):
        same_bits(a, c)
    ch, (rc, rflat, mean, std, pct, p50, hdi, hdi2), lt = out['device']
    n = ch.shape[0]
    assert n == 100 and ch.shape == (n, n_spectra, Wp, 6)
    assert rc.shape == (n, n_spectra, Wp, 5) and rflat.shape == (n_spectra, n * Wp, 5)
    assert mean.shape == std.shape == p50.shape == (n_spectra, 5) and pct.shape == (3, n_spectra, 5)
    assert hdi.shape == (2, n_spectra, 5) and hdi2.shape == (2, 2, n_spectra, 5) and many.shape == (len(P_MANY), n_spectra, 5)
    assert eight.shape == (n, n_spectra, Wp, 10)
    np.testing.assert_array_equal(rflat, rc.transpose(1, 0, 2, 3).reshape(n_spectra, n * Wp, 5))
    np.testing.assert_array_equal(p50, pct[1])
    # the chain is the host entry point's, row for row: every spectrum with the shared grid, in its own place
    rows = ch.reshape(n, n_spectra * Wp, 6)
    same_bits(rc.reshape(n, n_spectra * Wp, 5), host_rtd_descriptors(rows, lt, q, n_ensembles=n_spectra))
    same_bits(eight.reshape(n, n_spectra * Wp, 10), host_rtd_descriptors(rows, lt, Q_SETS[8], n_ensembles=n_spectra))
    assert len({tuple(r) for r in mean.round(3).tolist()}) > 1        # the spectra differ: the ensemble index is exercised
    # the summaries are those of the derived chain
    view = ChainView(torch.from_numpy(rows).cuda(), n, n_spectra, Wp, 6)
    d = view.derived(device_rtd_descriptors(view, lt, q))
    for got, want in zip((mean, std), device_moments(d)):
        same_bits(got, want)
    same_bits(pct, device_percentiles(d, [2.5, 50, 97.5]))
    same_bits(many, device_percentiles(d, P_MANY))
    same_bits(hdi, device_hdi(d, 0.9))
    same_bits(hdi2, device_hdi(d, [0.5, 0.9]))
    # against NumPy on the yardstick
    want, bound, fragile = yardstick_of(ch, lt, q)
    check_rows(rc, want, bound, fragile, lt)
    wf = want.transpose(1, 0, 2, 3).reshape(n_spectra, n * Wp, 5)
    bf = bound.transpose(1, 0, 2, 3).reshape(n_spectra, n * Wp, 5)
    for e in range(n_spectra):
        check_summaries(wf[e], bf[e], mean[e], std[e], many[:, e], P_MANY)


def model_outputs(m, **kw):
    return [m.get_relaxation_chain(**kw), m.get_relaxation_chain(flat=True, **kw), m.get_relaxation_mean(**kw),
            m.get_relaxation_std(**kw), m.get_relaxation_percentile(**kw), m.get_relaxation_percentile(50, **kw),
            m.get_relaxation_hdi(**kw), m.get_relaxation_hdi([0.5, 0.9], **kw)]


def test_model_methods():
    import bisip_amd
    from bisip_amd.decomposition import host_rtd_descriptors, rtd_descriptors
    out = {}
    for where in ('device', 'host'):
        np.random.seed(12)
        m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389174'], nwalkers=32, nsteps=500, poly_deg=5)
        m.fit(chain=where)
        out[where] = (m.get_chain(), model_outputs(m, discard=200, thin=2))
        flat = m.get_chain(discard=200, thin=2, flat=True)
        # a chain= array of whole samples is summarised as the fitted chain is
        for a, c in zip(model_outputs(m, chain=flat)[2:], out[where][1][2:]):
            same_bits(a, c)
        with pytest.raises(ValueError, match='Do not pass both'):
            m.get_relaxation_mean(chain=flat, thin=2)
    np.testing.assert_array_equal(out['device'][0], out['host'][0])
    for a, c in zip(out['device'][1], out['host'][1]):
        same_bits(a, c)
    rc, rflat, mean, std, pct, p50, hdi, hdi2 = out['device'][1]
    assert rc.shape == (150, 32, 5) and rflat.shape == (150 * 32, 5) and mean.shape == std.shape == p50.shape == (5,)
    assert pct.shape == (3, 5) and hdi.shape == (2, 5) and hdi2.shape == (2, 2, 5)
    ch = m.get_chain(discard=200, thin=2)
    same_bits(rc, host_rtd_descriptors(ch, m.log_tau))
    want, bound, fragile = yardstick_of(ch, m.log_tau, Q_SETS[3])
    check_rows(rc, want, bound, fragile, m.log_tau)
    check_rows(m.relaxation_descriptors(flat), want, bound, fragile, m.log_tau)
    np.testing.assert_array_equal(m.relaxation_descriptors(flat), rtd_descriptors(flat, m.log_tau))
    many = m.get_relaxation_percentile(P_MANY, discard=200, thin=2)
    check_summaries(want.reshape(-1, 5), bound.reshape(-1, 5), mean, std, many, P_MANY)
    # other fractions: one, and eight with q = 1
    assert m.get_relaxation_mean(discard=200, thin=2, q=[0.6]).shape == (3,)
    same_bits(m.get_relaxation_chain(discard=200, thin=2, q=Q_SETS[8]), host_rtd_descriptors(ch, m.log_tau, Q_SETS[8]))


def test_flat_chain_of_prior_box_rows():
    """5000 rows of the prior box as chain=: one sample of 5000 walkers, NaN rows among them."""
    import bisip_amd
    from bisip_amd.decomposition import host_rtd_descriptors
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389173'], poly_deg=4, nwalkers=32)
    rows = prior_rows(np.random.default_rng(14), 5000, 4)
    got = m.get_relaxation_chain(chain=rows)
    assert got.shape == (5000, 5)
    same_bits(got, host_rtd_descriptors(rows[None], m.log_tau)[0])
    want, bound, fragile = yardstick_of(rows, m.log_tau, Q_SETS[3])
    check_rows(got, want, bound, fragile, m.log_tau)
    assert np.isnan(got[:, 0]).any() and np.isnan(m.get_relaxation_mean(chain=rows)).all()
    ok = rows[~np.isnan(got[:, 0])]
    ok = ok[:ok.shape[0] // 32 * 32]                      # whole samples of 32 walkers
    mean, std = m.get_relaxation_mean(chain=ok), m.get_relaxation_std(chain=ok)
    pct = m.get_relaxation_percentile(P_MANY, chain=ok)
    want, bound, _ = yardstick_of(ok, m.log_tau, Q_SETS[3])
    check_summaries(want, bound, mean, std, pct, P_MANY)


@functools.lru_cache(maxsize=None)
def tutorial_fit():
    import bisip_amd
    np.random.seed(42)
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], nwalkers=32, poly_deg=4, c_exp=1, nsteps=1000)
    m.fit(chain='device')
    return m


def test_cumulative_times_are_ordered_on_real_data():
    """A bundled spectrum fitted as in the tutorial (degree 4, c_exp = 1): log_tau_10 < log_tau_50 < log_tau_90 for every
    used sample.  No value is recorded anywhere to compare with; none is asserted."""
    m = tutorial_fit()
    rc = m.get_relaxation_chain(discard=500, flat=True)
    assert rc.shape == (500 * 32, 5) and np.isfinite(rc).all()
    assert np.all(rc[:, 2] < rc[:, 3]) and np.all(rc[:, 3] < rc[:, 4])
    assert np.all(rc[:, [0, 2, 3, 4]] >= m.log_tau[0]) and np.all(rc[:, [0, 2, 3]] <= m.log_tau[-1])
    med = m.get_relaxation_percentile(50, discard=500)
    print('median (log_tau_peak, m_peak, log_tau_10, log_tau_50, log_tau_90):', med,
          'mean log_tau_mean:', m.get_integrating_mean(discard=500)[1])
