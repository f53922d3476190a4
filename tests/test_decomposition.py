"""PolynomialDecomposition's relaxation time distribution (RTD) and integrating parameters on the host
(bisip_amd.decomposition): the tutorial's formula, error bounds against a long-double yardstick, the known
answers of the decomposition tutorial, and the checks the public methods make before any device work.

Error bounds (u = 2**-53, C_k(theta) = sum_p |a_p| * sum_l |log_tau_l|**(p+k)):
  * m_total and sum_l m_l log_tau_l: 2 (L + P + 2) u C_0 and 2 (L + P + 2) u C_1;
  * a quotient q = num / den: (|d_num| + |q| |d_den|) / |den| + u |q| -- for log_tau_mean d_num, d_den are the
    two bounds above; for m_norm d_num is the bound of m_total and d_den = u |r0 * norm_factor| (the one rounding
    of that product in float64);
  * m_l: 2 (P + 2) u sum_p |a_p| |log_tau_l|**p.
"""

import numpy as np
import pytest

from bisip_amd.decomposition import INTEGRATING_NAMES, integrating_params, power_sums, rtd
from fitted import fitted_on_host
from test_gpu_known_answers import DEBYE_TUTORIAL

U = 2.0 ** -53

# docs/tutorials/decomposition.ipynb: total_m of the Debye fits (poly_deg=4) the get_m cell records
TOTAL_M_RECORDED = {'SIP-K389170': 1.342871, 'SIP-K389172': 1.210898, 'SIP-K389173': 0.786556,
                    'SIP-K389174': 0.930805, 'SIP-K389175': 0.655028, 'SIP-K389176': 0.545386}


def yardstick(theta, log_tau, norm_factor):
    """The definitions in long double: m (..., L), m_total, sum_l m_l log_tau_l, log_tau_mean, m_norm."""
    th = np.asarray(theta, dtype=np.float64).astype(np.longdouble)
    lt = np.asarray(log_tau, dtype=np.float64).astype(np.longdouble)
    m = np.zeros(th.shape[:-1] + lt.shape, dtype=np.longdouble)
    for p in range(th.shape[-1] - 1):
        m = m + th[..., 1 + p, None] * lt ** p
    total = m.sum(axis=-1)
    num = (m * lt).sum(axis=-1)
    den = th[..., 0] * np.asarray(norm_factor, dtype=np.float64).astype(np.longdouble)
    with np.errstate(divide='ignore', invalid='ignore'):
        return m, total, num, num / total, total / den


def bounds(theta, log_tau, norm_factor):
    """Bounds of (m_total, log_tau_mean, m_norm) (..., 3) and of m (..., L), as the module docstring derives."""
    th = np.asarray(theta, dtype=np.float64)
    lt = np.abs(np.asarray(log_tau, dtype=np.float64))
    L, P = lt.size, th.shape[-1] - 2
    a = np.abs(th[..., 1:]).astype(np.longdouble)
    powers = np.array([lt.astype(np.longdouble) ** k for k in range(P + 2)])     # (P + 2, L)
    C0 = (a * powers[:P + 1].sum(axis=1)).sum(axis=-1)
    C1 = (a * powers[1:].sum(axis=1)).sum(axis=-1)
    d_tot, d_num = 2 * (L + P + 2) * U * C0, 2 * (L + P + 2) * U * C1
    _, total, num, mean, norm = yardstick(theta, log_tau, norm_factor)
    den = np.abs(th[..., 0].astype(np.longdouble) * np.asarray(norm_factor, dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        b_mean = (d_num + np.abs(mean) * d_tot) / np.abs(total) + U * np.abs(mean)
        b_norm = (d_tot + np.abs(norm) * U * den) / den + U * np.abs(norm)
    b_m = 2 * (P + 2) * U * np.einsum('...p,pl->...l', a, powers[:P + 1])
    return np.stack([d_tot, b_mean, b_norm], axis=-1), b_m


def assert_within(got, want, bound, what=''):
    """|got - want| <= bound elementwise, in long double; NaN / inf where the yardstick has them."""
    got = np.asarray(got, dtype=np.float64).astype(np.longdouble)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= bound[fin]), (what, float(np.max(err / bound[fin])))
    return float(np.max(err / bound[fin])) if err.size else 0.0


def tutorial_m(row, log_tau):
    """The get_m cell of the tutorial, restated: m += coeff * log_tau**p; total_m = np.sum(m)."""
    m = 0
    for p in range(len(row) - 1):
        m += row[1 + p] * log_tau ** p
    return m, np.sum(m)


def prior_rows(rng, n, P):
    lo = np.array([0.9] + [-1.0] * (P + 1))
    hi = np.array([1.1] + [1.0] * (P + 1))
    return rng.uniform(lo, hi, (n, P + 2))


def tutorial_rows(rng, n):
    """Rows around the tutorial's posterior means (poly_deg=4), a few percent of their size apart."""
    means = np.array(list(DEBYE_TUTORIAL.values()))
    pick = means[rng.integers(0, len(means), n)]
    return pick * (1.0 + 0.05 * rng.standard_normal(pick.shape))


def grid(L, lo=-6.0, hi=2.0):
    return np.linspace(lo, hi, L)


def test_names():
    assert INTEGRATING_NAMES == ('m_total', 'log_tau_mean', 'm_norm')
    import bisip_amd
    assert bisip_amd.INTEGRATING_NAMES is INTEGRATING_NAMES
    assert bisip_amd.rtd is rtd and bisip_amd.integrating_params is integrating_params


@pytest.mark.parametrize('P', [0, 4, 5])
def test_host_definitions_are_the_tutorial_formula(P):
    rng = np.random.default_rng(P)
    lt = grid(40)
    rows = prior_rows(rng, 50, P)
    m_all, ip = rtd(rows, lt), integrating_params(rows, lt, 1.7)
    assert m_all.shape == (50, 40) and ip.shape == (50, 3)
    for i, row in enumerate(rows):
        m, total = tutorial_m(row, lt)
        np.testing.assert_array_equal(rtd(row, lt), m)
        np.testing.assert_array_equal(m_all[i], m)
        np.testing.assert_array_equal(integrating_params(row, lt, 1.7)[0], total)
        np.testing.assert_array_equal(ip[i, 0], total)
        np.testing.assert_array_equal(ip[i, 1], np.sum(m * lt) / total)
        np.testing.assert_array_equal(ip[i, 2], total / (row[0] * 1.7))


@pytest.mark.parametrize('L', [40, 64])
@pytest.mark.parametrize('P', [4, 5, 8])
def test_float64_definitions_meet_the_bounds(L, P):
    rng = np.random.default_rng(L * 10 + P)
    lt = grid(L, -7.0, 3.0) if L == 64 else grid(L)
    rows = prior_rows(rng, 4000, P)
    if P == 4:
        rows = np.concatenate([rows, tutorial_rows(rng, 2000)])
    nf = 3.5
    b3, bm = bounds(rows, lt, nf)
    m, total, num, mean, norm = yardstick(rows, lt, nf)
    ip = integrating_params(rows, lt, nf)
    assert_within(ip[:, 0], total, b3[:, 0], 'm_total')
    assert_within(ip[:, 1], mean, b3[:, 1], 'log_tau_mean')
    assert_within(ip[:, 2], norm, b3[:, 2], 'm_norm')
    assert_within(rtd(rows, lt), m, bm, 'm_l')


def test_power_sums():
    """S_p of the tutorial's grid (-6 ... 2, 40 points): 40, -80, 384.27, -1665.64, 8284.11."""
    lt = grid(40)
    S = power_sums(lt, 5)
    np.testing.assert_allclose(S, [40, -80, 384.27, -1665.64, 8284.11], rtol=0, atol=5e-3)
    want = [np.sum(lt.astype(np.longdouble) ** k) for k in range(5)]
    assert np.all(np.abs(S - np.array(want, dtype=np.float64)) <= U * np.abs(S))


def test_tutorial_total_chargeability():
    """decomposition.ipynb: the six bundled spectra share one grid; the tutorial's printed means give its
    recorded total_m within the printing error 0.5e-6 * sum_p |S_p| + 0.5e-6."""
    import bisip_amd
    files = bisip_amd.DataFiles()
    models = {name: bisip_amd.PolynomialDecomposition(files[name], poly_deg=4, c_exp=1) for name in TOTAL_M_RECORDED}
    grids = [m.log_tau for m in models.values()]
    for g in grids[1:]:
        np.testing.assert_array_equal(g, grids[0])
    lt = grids[0]
    assert lt.size == 40 and lt[0] == -6.0 and lt[-1] == 2.0
    S = power_sums(lt, 5)
    tol = 0.5e-6 * np.sum(np.abs(S)) + 0.5e-6
    for name, model in models.items():
        theta = np.array(DEBYE_TUTORIAL[name])
        got = model.integrating_params(theta)
        assert got.shape == (3,)
        np.testing.assert_array_equal(got, integrating_params(theta, lt, model.data['norm_factor']))
        np.testing.assert_array_equal(model.rtd(theta), rtd(theta, lt))
        assert abs(got[0] - TOTAL_M_RECORDED[name]) <= tol, (name, got[0], TOTAL_M_RECORDED[name], tol)


def test_abi_version_and_symbols(hip_lib):
    assert hip_lib.bisip_abi_version() == 6
    for name in ('bisip_rtd_integrals_dev', 'bisip_rtd_columns_dev'):
        assert hasattr(hip_lib, name)


@pytest.mark.parametrize('method', ['get_integrating_chain', 'get_integrating_mean', 'get_integrating_std',
                                    'get_integrating_percentile', 'get_rtd_percentile'])
def test_argument_checks(method):
    m = fitted_on_host()
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=20)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=5, thin=0)
    with pytest.raises(ValueError, match='Do not pass both'):
        f(chain=m.get_chain(flat=True), discard=5)
    with pytest.raises(ValueError, match='Flatten'):
        f(chain=m.get_chain())


@pytest.mark.parametrize('method', ['rtd', 'integrating_params', 'get_integrating_chain', 'get_integrating_mean',
                                    'get_integrating_std', 'get_integrating_percentile', 'get_rtd_percentile'])
def test_spectra_batch_of_another_model_refuses(method):
    from bisip_amd import SpectraBatch
    b = SpectraBatch.__new__(SpectraBatch)       # the check comes before the device context is touched
    b.model, b._sampler = 'PeltonColeCole', None
    with pytest.raises(ValueError, match='PolynomialDecomposition'):
        f = getattr(b, method)
        f(np.zeros((1, 2, 7))) if method in ('rtd', 'integrating_params') else f()
