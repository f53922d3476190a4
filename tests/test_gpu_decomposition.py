"""PolynomialDecomposition's RTD and integrating parameters on the device (bisip_rtd_integrals_dev,
bisip_rtd_columns_dev) against the long-double yardstick, from the C entry points up to the model and
SpectraBatch methods.  Bounds: tests/test_decomposition.py.  Summaries add the tolerance the existing
device-summary tests hold the same kernels to: MOMENT_TOL relative to max(1, |value|) for the mean
(tests/test_gpu_batch.py), rtol 1e-9 for the std (tests/test_gpu_parity.py) -- loose figures kept as they were; what
the moments kernel itself is held to is the derived bound of tests/moments_bounds.py; a percentile is 1-Lipschitz in
the max-norm of its column, so it may move by the largest bound of the column plus 4u of its value."""

import warnings

import numpy as np
import pytest

from chain_harness import GuardedCall
from test_decomposition import (DEBYE_TUTORIAL, TOTAL_M_RECORDED, U, assert_within, bounds, prior_rows,
                                yardstick)

pytestmark = pytest.mark.gpu

MOMENT_TOL = 1e-12
STD_RTOL = 1e-9
P_MANY = [0, 1, 2.5, 10, 25, 37.5, 50, 62.5, 75, 90, 97.5, 99, 100]      # more than 8: the sort path


def derived_yardstick(chain, log_tau, nf):
    """(n, ..., ndim) chain -> long-double (m_total, log_tau_mean, m_norm) (n, ..., 3), their bounds, and the
    long-double RTD (n, ..., L) with its bounds."""
    m, total, _, mean, norm = yardstick(chain, log_tau, nf)
    b3, bm = bounds(chain, log_tau, nf)
    return np.stack([total, mean, norm], axis=-1), b3, m, bm


def check_summaries(flat_dev, flat_want, b3, mean, std, pct, p):
    """Device mean / std / percentiles of a derived chain against NumPy's on the long-double yardstick rounded
    to float64; flat_* (rows, 3), b3 the per-row bounds."""
    want = flat_want.astype(np.float64)
    bmax = np.max(b3, axis=0).astype(np.float64)
    m_np, s_np = want.mean(axis=0), want.std(axis=0)
    assert np.all(np.abs(mean - m_np) <= MOMENT_TOL * np.maximum(1.0, np.abs(m_np)) + bmax), (mean, m_np)
    assert np.all(np.abs(std - s_np) <= STD_RTOL * np.abs(s_np) + bmax), (std, s_np)
    pw = np.percentile(want, p, axis=0)
    assert np.all(np.abs(pct - pw) <= bmax + 4 * U * np.abs(pw)), (pct, pw)


def chain_columns(t, n, off, stride, E, Wp, ndim, log_tau):
    """Every m_l of every sample of a device chain, from the C entry point: (E, L, n * Wp), rows s * Wp + w."""
    import torch
    from bisip_amd import _hip
    L = len(log_tau)
    lt = torch.from_numpy(np.ascontiguousarray(log_tau)).cuda()
    call = GuardedCall()
    cols = call.out('the columns', (E, L, n * Wp))
    _hip.rtd_columns_dev(t.data_ptr() + 8 * off, n, stride, E, Wp, ndim, 0, E, lt.data_ptr(), L, cols, call.stream)
    return call.finish()[0]


def rtd_columns(s, log_tau, discard, thin):
    """Every m_l of every used sample of a sampler: (E, L, n * Wp)."""
    v = s.used_samples_dev(discard, thin)
    return chain_columns(v.tensor, v.n, v.offset, v.stride, s.n_ensembles, s.walkers_per_ensemble, s.ndim, log_tau)


def batch_spectra():
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    files = bisip_amd.DataFiles()
    return [files[k] for k in sorted(DEBYE_TUTORIAL)] + [synthetic_columns(20, i) for i in range(4)]


@pytest.mark.parametrize('P', [4, 5])
def test_batch_per_sample_values_and_summaries(P):
    import bisip_amd
    spectra = batch_spectra()
    E, Wp, discard, thin = len(spectra), 32, 150, 3
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=Wp, nsteps=400, poly_deg=P)
    np.random.seed(P)
    b.fit(seed=3, chain='device')
    ch = b.get_chain(discard=discard, thin=thin)                          # (n, E, Wp, ndim)
    n, L = ch.shape[0], b.log_tau.size
    assert n == len(range(discard + thin - 1, 400, thin))
    nf = np.asarray(b.norm_factor)[None, :, None]
    want, b3, m_want, bm = derived_yardstick(ch, b.log_tau, nf)
    got = b.get_integrating_chain(discard=discard, thin=thin)
    assert got.shape == (n, E, Wp, 3)
    for j, name in enumerate(('m_total', 'log_tau_mean', 'm_norm')):
        assert_within(got[..., j], want[..., j], b3[..., j], name)
    cols = rtd_columns(b._sampler, b.log_tau, discard, thin)                  # (E, L, n * Wp), rows s * Wp + w
    m_cols = m_want.transpose(1, 3, 0, 2).reshape(E, L, n * Wp)
    bm_cols = bm.transpose(1, 3, 0, 2).reshape(E, L, n * Wp)
    assert_within(cols, m_cols, bm_cols, 'm_l')
    # the host methods: each spectrum with its own norm_factor, as the module's definitions one spectrum at a time
    from bisip_amd import decomposition
    theta = ch.transpose(1, 0, 2, 3).reshape(E, -1, P + 2)
    host_rtd, host_ip = b.rtd(theta), b.integrating_params(theta)
    assert host_rtd.shape == (E, n * Wp, L) and host_ip.shape == (E, n * Wp, 3)
    for e in range(E):
        np.testing.assert_array_equal(host_rtd[e], decomposition.rtd(theta[e], b.log_tau))
        np.testing.assert_array_equal(host_ip[e], decomposition.integrating_params(theta[e], b.log_tau,
                                                                                  b.norm_factor[e]))
    assert len(set(np.asarray(b.norm_factor).tolist())) > 1      # the per-spectrum factor is exercised
    # summaries
    flat = b.get_integrating_chain(discard=discard, thin=thin, flat=True)
    np.testing.assert_array_equal(flat, got.transpose(1, 0, 2, 3).reshape(E, n * Wp, 3))
    mean, std = b.get_integrating_mean(discard, thin), b.get_integrating_std(discard, thin)
    pct = b.get_integrating_percentile(P_MANY, discard, thin)
    assert mean.shape == std.shape == (E, 3) and pct.shape == (len(P_MANY), E, 3)
    one = b.get_integrating_percentile(50, discard, thin)
    np.testing.assert_array_equal(one, b.get_integrating_percentile([50], discard, thin)[0])
    wf = want.transpose(1, 0, 2, 3).reshape(E, n * Wp, 3)
    bf = b3.transpose(1, 0, 2, 3).reshape(E, n * Wp, 3)
    for e in range(E):
        check_summaries(flat[e], wf[e], bf[e], mean[e], std[e], pct[:, e], P_MANY)
    rp = b.get_rtd_percentile([2.5, 50, 97.5], discard, thin)
    assert rp.shape == (3, E, L)
    pw = np.percentile(m_cols.astype(np.float64), [2.5, 50, 97.5], axis=2)          # (3, E, L)
    bmax = bm_cols.max(axis=2).astype(np.float64)
    assert np.all(np.abs(rp - pw) <= bmax + 4 * U * np.abs(pw))
    np.testing.assert_array_equal(b.gather(np.moveaxis(rp, 1, 0)), np.moveaxis(rp, 1, 0))
    b.close()


def test_many_percentiles_of_many_ensembles_take_the_sort_path():
    """24 ensembles x 3 = 72 columns and 13 percentiles: bisip_chain_percentiles_dev sorts."""
    import torch
    from bisip_amd import decomposition
    from bisip_amd.chainview import ChainView, device_moments, device_percentiles
    E, Wp, n, P = 24, 16, 40, 5
    rng = np.random.default_rng(5)
    chain = prior_rows(rng, n * E * Wp, P).reshape(n, E * Wp, P + 2)
    lt = np.linspace(-7.0, 3.0, 64)
    nf = rng.uniform(0.5, 3.0, E)
    t = torch.from_numpy(chain).cuda()
    view = ChainView(t, n, E, Wp, P + 2)
    d = decomposition.device_integrating_chain(view, lt, nf)
    got = d.cpu().numpy().reshape(n, E, Wp, 3)
    want, b3, _, _ = derived_yardstick(chain.reshape(n, E, Wp, P + 2), lt, nf[None, :, None])
    for j in range(3):
        assert_within(got[..., j], want[..., j], b3[..., j])
    mean, std = device_moments(view.derived(d))
    pct = device_percentiles(view.derived(d), P_MANY)
    gf = got.transpose(1, 0, 2, 3).reshape(E, -1, 3)
    wf = want.transpose(1, 0, 2, 3).reshape(E, -1, 3)
    bf = b3.transpose(1, 0, 2, 3).reshape(E, -1, 3)
    for e in range(E):
        check_summaries(gf[e], wf[e], bf[e], mean[e], std[e], pct[:, e], P_MANY)


@pytest.mark.parametrize('P', [4, 5])
def test_flat_chain_of_prior_box_rows(P):
    import bisip_amd
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389173'], poly_deg=P, nwalkers=32)
    rows = prior_rows(np.random.default_rng(P + 10), 5000, P)
    nf = m.data['norm_factor']
    want, b3, m_want, bm = derived_yardstick(rows, m.log_tau, nf)
    got = m.get_integrating_chain(chain=rows)
    assert got.shape == (5000, 3)
    for j in range(3):
        assert_within(got[:, j], want[:, j], b3[:, j])
    mean, std = m.get_integrating_mean(chain=rows), m.get_integrating_std(chain=rows)
    pct = m.get_integrating_percentile(P_MANY, chain=rows)
    assert mean.shape == std.shape == (3,) and pct.shape == (len(P_MANY), 3)
    check_summaries(got, want, b3, mean, std, pct, P_MANY)
    assert m.get_integrating_percentile(97.5, chain=rows).shape == (3,)
    # every m_l of every row, on the layout the chain= path uploads (5000 rows: one sample of 5000 walkers)
    v = m._decomposition_samples(rows, {})
    assert (v.n, v.walkers_per_ensemble) == (1, 5000)
    cols = chain_columns(v.tensor, v.n, v.offset, v.stride, 1, v.walkers_per_ensemble, P + 2, m.log_tau)[0]          # (L, 5000)
    assert_within(cols.T, m_want, bm, 'm_l')
    rp = m.get_rtd_percentile(chain=rows)
    assert rp.shape == (3, m.log_tau.size)
    pw = np.percentile(m_want.astype(np.float64), [2.5, 50, 97.5], axis=0)
    assert np.all(np.abs(rp - pw) <= bm.max(axis=0).astype(np.float64) + 4 * U * np.abs(pw))
    np.testing.assert_array_equal(m.get_rtd_percentile(50, chain=rows), m.get_rtd_percentile([50], chain=rows)[0])


def batch_outputs(b, discard, thin):
    return [b.get_integrating_chain(discard, thin), b.get_integrating_chain(discard, thin, flat=True),
            b.get_integrating_mean(discard, thin), b.get_integrating_std(discard, thin),
            b.get_integrating_percentile([2.5, 50, 97.5], discard, thin), b.get_integrating_percentile(50, discard, thin),
            b.get_rtd_percentile([2.5, 50, 97.5], discard, thin), b.get_rtd_percentile(16, discard, thin)]


def test_batch_device_and_host_chains_give_the_same_bits():
    import bisip_amd
    spectra = batch_spectra()
    out = {}
    for chain in ('device', 'host'):
        b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=32, nsteps=300, poly_deg=4)
        np.random.seed(8)
        b.fit(seed=9, chain=chain)
        out[chain] = (b.get_chain(), batch_outputs(b, 100, 2))
        b.close()
    np.testing.assert_array_equal(out['device'][0], out['host'][0])
    for a, c in zip(out['device'][1], out['host'][1]):
        np.testing.assert_array_equal(a.view(np.int64), c.view(np.int64))


def model_outputs(m, **kw):
    return [m.get_integrating_chain(**kw), m.get_integrating_chain(flat=True, **kw), m.get_integrating_mean(**kw),
            m.get_integrating_std(**kw), m.get_integrating_percentile(**kw), m.get_integrating_percentile(50, **kw),
            m.get_rtd_percentile(**kw), m.get_rtd_percentile(84, **kw)]


def test_model_device_and_host_chains_give_the_same_bits():
    import bisip_amd
    out = {}
    for chain in ('device', 'host'):
        np.random.seed(12)
        m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389174'], nwalkers=32, nsteps=800,
                                              poly_deg=5)
        m.fit(chain=chain)
        out[chain] = (m.get_chain(), model_outputs(m, discard=300, thin=2))
        flat = m.get_chain(discard=300, thin=2, flat=True)
        # a chain= array of whole samples is summarised as the fitted chain is
        for a, c in zip(model_outputs(m, chain=flat)[2:], out[chain][1][2:]):
            np.testing.assert_array_equal(a, c)
        with pytest.warns(UserWarning, match='No samples were discarded'):
            m.get_integrating_mean()
        with pytest.raises(ValueError, match='Do not pass both'):
            m.get_integrating_mean(chain=flat, thin=2)
    np.testing.assert_array_equal(out['device'][0], out['host'][0])
    for a, c in zip(out['device'][1], out['host'][1]):
        np.testing.assert_array_equal(a.view(np.int64), c.view(np.int64))
    assert out['device'][1][0].shape == (250, 32, 3) and out['device'][1][1].shape == (250 * 32, 3)


def test_rtd_passes_give_the_same_bits(monkeypatch):
    import bisip_amd
    from bisip_amd import decomposition
    spectra = batch_spectra()
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=32, nsteps=200, poly_deg=5)
    np.random.seed(4)
    b.fit(seed=4, chain='device')
    p = [2.5, 16, 50, 84, 97.5]
    one = b.get_rtd_percentile(p, discard=50)
    n, L = 150, b.log_tau.size
    per_spectrum = n * 32 * L * 8
    monkeypatch.setattr(decomposition, 'RTD_PASS_BYTES', 3 * per_spectrum)      # 10 spectra: 4 passes
    assert -(-b.n_spectra // 3) >= 3
    np.testing.assert_array_equal(b.get_rtd_percentile(p, discard=50).view(np.int64), one.view(np.int64))
    monkeypatch.setattr(decomposition, 'RTD_PASS_BYTES', 1)                     # one spectrum per pass
    np.testing.assert_array_equal(b.get_rtd_percentile(p, discard=50).view(np.int64), one.view(np.int64))
    b.close()


def test_batch_of_another_model_refuses():
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    b = bisip_amd.SpectraBatch('PeltonColeCole', [synthetic_columns(20, i) for i in range(2)], nwalkers=16,
                               nsteps=20)
    b.fit(seed=1, chain='device')
    for f in (b.get_integrating_mean, b.get_integrating_std, b.get_integrating_percentile, b.get_rtd_percentile,
              b.get_integrating_chain):
        with pytest.raises(ValueError, match='PolynomialDecomposition'):
            f()
    b.close()


@pytest.mark.parametrize('name', sorted(DEBYE_TUTORIAL))
def test_tutorial_total_chargeability_on_the_gpu(name):
    """The setting of test_debye_decomposition_tutorial_means, chain kept on the device.  m_total is linear in
    a_p, so the 0.35-sigma condition that test asserts on every a_p bounds the posterior mean of m_total:
    0.35 sum_p |S_p| std(a_p), plus the printing error of the tutorial's table, plus the summary allowance."""
    import bisip_amd
    from bisip_amd.decomposition import power_sums
    np.random.seed(42)
    model = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()[name], nwalkers=32, poly_deg=4, c_exp=1,
                                              nsteps=3000)
    model.fit(chain='device')
    got = model.get_integrating_mean(discard=1500)[0]
    std = model.get_param_std(discard=1500)[1:]
    S = np.abs(power_sums(model.log_tau, 5))
    chain = model.get_chain(discard=1500, flat=True)
    _, b3, _, _ = derived_yardstick(chain, model.log_tau, model.data['norm_factor'])
    allowance = MOMENT_TOL * max(1.0, abs(got)) + float(np.max(b3[:, 0]))
    tol = 0.35 * np.sum(S * std) + 0.5e-6 * np.sum(S) + 0.5e-6 + allowance
    assert abs(got - TOTAL_M_RECORDED[name]) <= tol, (name, got, TOTAL_M_RECORDED[name], tol)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        model.get_integrating_std(discard=1500)


def test_more_samples_than_one_grid_column():
    """70,000 samples of 2 x 1 walkers: the kernels' sample loop goes beyond the 65,535 blocks of the grid's y."""
    import torch
    from bisip_amd import decomposition
    from bisip_amd.chainview import ChainView
    E, Wp, n, P = 2, 1, 70000, 4
    rng = np.random.default_rng(70)
    chain = prior_rows(rng, n * E * Wp, P).reshape(n, E * Wp, P + 2)
    lt = np.linspace(-6.0, 2.0, 40)
    nf = np.array([0.7, 2.5])
    t = torch.from_numpy(chain).cuda()
    got = decomposition.device_integrating_chain(ChainView(t, n, E, Wp, P + 2), lt, nf).cpu().numpy()
    got = got.reshape(n, E, Wp, 3)
    want, b3, m_want, bm = derived_yardstick(chain.reshape(n, E, Wp, P + 2), lt, nf[None, :, None])
    for j in range(3):
        assert_within(got[..., j], want[..., j], b3[..., j])
    cols = chain_columns(t, n, 0, E * Wp * (P + 2), E, Wp, P + 2, lt)              # (E, L, n * Wp)
    assert_within(cols, m_want.transpose(1, 3, 0, 2).reshape(E, len(lt), n * Wp),
                  bm.transpose(1, 3, 0, 2).reshape(E, len(lt), n * Wp), 'm_l')
