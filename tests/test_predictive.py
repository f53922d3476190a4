"""bisip_amd.predictive on the host: the closed-form functions against mpmath at 50 digits, hand cases, the calibration of
the definitions on data drawn from the model itself (every probability uniform), the NumPy restatement of the
predictive-check kernel's order against the long-double yardstick within the bounds of tests/predictive_bounds.py, glibc's
erfc -- the one function the yardstick does not take in long double -- against mpmath, the new entry points and the
surface of the models and of SpectraBatch."""
import inspect
import math
import os
import re

import mpmath
import numpy as np
import pytest

import predictive_bounds as pb
from bisip_amd import predictive as pp
from convergence_bounds import LD, U
from fit_quality_bounds import data_for, inverse_variance
from response_bounds import responses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = float(pb.TINY)


def mp(x):
    """A double or long double as an mpmath number, exactly."""
    x = LD(x)
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


@pytest.fixture(autouse=True)
def fifty_digits():
    with mpmath.workdps(50):
        yield


# -- the yardstick's erfc -----------------------------------------------------------------------------------------------
def test_erfc_of_glibc_and_of_the_yardstick_against_mpmath():
    rng = np.random.default_rng(0)
    z = np.concatenate([np.linspace(-40.0, 40.0, 4001), rng.uniform(-40.0, 40.0, 4000), 3.0 * rng.normal(size=1999)])
    a = -z / math.sqrt(2.0)
    worst = 0.0
    for v in a:
        want = mpmath.erfc(mpmath.mpf(float(v)))
        if want >= mpmath.mpf(2) ** -1022:                             # (below: no relative error to speak of)
            worst = max(worst, float(abs(mpmath.mpf(math.erfc(v)) - want) / want) / U)
        else:
            assert abs(mpmath.mpf(math.erfc(v)) - want) <= TINY
    print(f'math.erfc: at most {worst:.2f} u over {a.size} arguments')
    assert worst <= pb.ERFC_GLIBC
    # the yardstick's erfc of long-double arguments that are no doubles: the same bound, no rounding of the argument
    a_ld = (a[::7].astype(LD) * (1 + LD(2.0) ** -55)) / np.sqrt(LD(2)) * np.sqrt(LD(2))
    got = pb.erfc_ld(a_ld)
    for v, g in zip(a_ld, got):
        want = mpmath.erfc(mp(v))
        if want >= mpmath.mpf(2) ** -1022:
            assert abs(mp(g) - want) <= (pb.ERFC_GLIBC + 0.01) * U * want, float(v)


# -- the functions against mpmath -----------------------------------------------------------------------------------
X_GRID = (1e-3, 0.03, 0.5, 1.0, 2.5, 7.0, 19.0, 63.5, 64.0, 150.0, 700.0, 1e4)


@pytest.mark.parametrize('N', range(1, 65))
def test_chi2_sf_even_against_mpmath(N):
    x = np.array(sorted(set(X_GRID + (float(N), np.nextafter(float(N), 0.0), N + 0.5, max(N - 0.5, 0.25)))))
    assert (x < N).any() and (x >= N).any() and (x == N).any()          # both branches and the switch point
    got = pp.chi2_sf_even(N, x)
    rel = pb.chi2_sf_rel_bound(N, x.astype(LD), pb.K_NUMPY).astype(np.float64)
    for xv, g, r in zip(x, got, rel):
        want = mpmath.gammainc(N, mpmath.mpf(float(xv)), mpmath.inf, regularized=True)
        assert abs(mpmath.mpf(float(g)) - want) <= r * want + TINY, (N, xv, g)
        assert 0.0 <= g <= 1.0
    assert pp.chi2_sf_even(N, 0.0) == 1.0 and pp.chi2_sf_even(N, np.inf) == 0.0 and np.isnan(pp.chi2_sf_even(N, np.nan))


def test_chi2_sf_even_refuses_what_it_cannot_be():
    with pytest.raises(ValueError, match='at least 1'):
        pp.chi2_sf_even(0, 1.0)
    with pytest.raises(ValueError, match='negative'):
        pp.chi2_sf_even(3, -1.0)
    assert pp.chi2_sf_even(3, np.ones((2, 5))).shape == (2, 5)


def test_normal_cdf_against_mpmath():
    rng = np.random.default_rng(1)
    z = np.concatenate([np.linspace(-38.0, 9.0, 300), rng.normal(size=300), [0.0, -0.0, np.inf, -np.inf]])
    got = pp.normal_cdf(z)
    assert got[-4] == got[-3] == 0.5 and got[-2] == 1.0 and got[-1] == 0.0
    for zv, g in zip(z[:-2], got[:-2]):
        want = mpmath.ncdf(mpmath.mpf(float(zv)))
        # erfc: ERFC_GLIBC u; the quotient by a rounded sqrt 2: 2 u of the argument
        bound = U * (pb.ERFC_GLIBC * want + 2 * mpmath.npdf(mpmath.mpf(float(zv))) * abs(float(zv))) + TINY
        assert abs(mpmath.mpf(float(g)) - want) <= bound, zv
    assert np.isnan(pp.normal_cdf(np.nan))


@pytest.mark.parametrize('n', (2, 6, 40, 64))
def test_max_abs_sf_against_mpmath(n):
    q = np.array([0.0, 1e-300, 1e-12, 1e-3, 0.5, 1.0, 4.0, 9.0, 25.0, 80.0, 400.0, 1500.0, 3000.0])
    got = pp.max_abs_sf(n, q)
    _, bound = pb.max_abs_sf_ld(n, q, pb.K_NUMPY, 1)
    assert got[0] == 1.0 and got[-1] == 0.0
    for qv, g, b in zip(q, got, bound.astype(np.float64)):
        e = mpmath.erfc(mpmath.sqrt(mpmath.mpf(float(qv)) / 2))
        want = -mpmath.expm1(n * mpmath.log1p(-e)) if e < 1 else mpmath.mpf(1)
        assert abs(mpmath.mpf(float(g)) - want) <= b + TINY, (n, qv, g)
    assert (np.diff(got) <= 0).all()


@pytest.mark.parametrize('m', (0, 1, 4, 38, 126))
def test_binomial_half_cdf_against_mpmath(m):
    got = pp.binomial_half_cdf(m)
    assert got.shape == (m + 1,) and got[-1] == 1.0
    total = mpmath.mpf(0)
    for c in range(m + 1):
        total += mpmath.binomial(m, c)
        assert got[c] == float(total / mpmath.mpf(2) ** m)              # an integer ratio: correctly rounded
    assert got[0] == 2.0 ** -m
    with pytest.raises(ValueError, match='negative'):
        pp.binomial_half_cdf(-1)


def test_sign_changes_by_hand():
    d = np.array([[1.0, -1.0, -2.0, 0.0, 3.0], [-1.0, -1.0, -0.0, 1.0, -1.0]])
    # Re: + - - + +: 2 changes (0.0 is not < 0); Im: - - + + -: 2 changes (-0.0 is not < 0)
    assert pp.sign_changes(d) == 4
    assert list(pp.sign_changes(np.stack([d, -d, np.abs(d)]))) == [4, 4, 0]
    with pytest.raises(ValueError, match='2, N'):
        pp.sign_changes(np.zeros((3, 4)))


# -- hand cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', (1, 2, 7, 32))
def test_a_row_on_the_data(N):
    y = responses(1, 1, N)[0, 0]
    err = 0.01 * np.abs(y) + 1e-3
    c = pp.predictive_check(y[None], y, err)
    assert (c['pit'] == 0.5).all() and c['n_extreme'] == 0
    assert c['chi2_mean'] == 0.0 and c['chi2_reduced'] == 0.0 and c['p_chi2'] == 1.0 and c['p_max'] == 1.0
    assert c['sign_changes'].shape == (2 * N - 1,) and c['sign_changes'].dtype == np.int64
    assert c['sign_changes'][0] == 1 and c['sign_changes'].sum() == 1 == c['n_rows']
    assert c['p_runs'] == 2.0 ** -(2 * N - 2)                           # (N = 1, the smallest a context accepts: one bin, 1.0)
    ordered = pp.ordered_predictive_sums(y[None], y, inverse_variance(err))
    assert (ordered[0] == 0.5).all() and list(ordered[1][0]) == [0.0, 1.0, 1.0] and ordered[2][0, 0] == 1


@pytest.mark.parametrize('N', (2, 7, 32))
def test_residuals_of_one_sigma_alternating_in_sign(N):
    y = responses(1, 1, N)[0, 0]
    err = 2.0 ** -7 * np.ones((2, N))                                   # (a power of two: iv and every q are exact)
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    Z = (y - err * sign)[None]
    y = Z[0] + err * sign                                               # (so that y - Z is err to the bit)
    c = pp.predictive_check(Z, y, err)
    assert c['sign_changes'][2 * N - 2] == 1 and c['sign_changes'].sum() == 1
    assert c['p_runs'] == 1.0 and c['chi2_mean'] == 2 * N and c['chi2_reduced'] == 1.0
    np.testing.assert_allclose(c['pit'], np.broadcast_to(np.where(sign > 0, 0.8413447460685429, 0.15865525393145705), (2, N)),
                               rtol=1e-15)
    with mpmath.workdps(50):
        want = mpmath.gammainc(N, N, mpmath.inf, regularized=True)
        assert float(want) == pytest.approx(c['p_chi2'], rel=1e-13)
        assert float(1 - mpmath.erf(1 / mpmath.sqrt(2)) ** (2 * N)) == pytest.approx(c['p_max'], rel=1e-13)


def test_definitions_against_loops():
    rng = np.random.default_rng(5)
    R, N = 9, 4
    Z = rng.normal(size=(R, 2, N))
    y = rng.normal(size=(2, N))
    err = rng.uniform(0.5, 2.0, size=(2, N))
    pit, row, hist = pp.predictive_sums(Z, y, inverse_variance(err))
    c = pp.predictive_check(Z, y, err)
    F = pp.binomial_half_cdf(2 * N - 2)
    T, Q, pm, Cs = [], [], [], []
    for r in range(R):
        z = (y - Z[r]) / err
        T.append(float(np.sum(z ** 2)))
        Q.append(float(mpmath.gammainc(N, T[-1] / 2, mpmath.inf, regularized=True)))
        pm.append(1 - math.erf(np.abs(z).max() / math.sqrt(2)) ** (2 * N))
        Cs.append(sum(int((z[p, j] < 0) != (z[p, j + 1] < 0)) for p in range(2) for j in range(N - 1)))
    np.testing.assert_allclose(row, [np.mean(T), np.mean(Q), np.mean(pm)], rtol=1e-12)
    np.testing.assert_array_equal(hist, np.bincount(Cs, minlength=2 * N - 1))
    for p in range(2):
        for j in range(N):
            want = np.mean([0.5 * math.erfc(-(y[p, j] - Z[r, p, j]) / err[p, j] / math.sqrt(2)) for r in range(R)])
            assert pit[p, j] == pytest.approx(want, rel=1e-13)
    assert c['p_runs'] == pytest.approx(np.mean([F[k] for k in Cs]), rel=1e-14) and c['n_rows'] == R
    assert c['chi2_reduced'] == c['chi2_mean'] / (2 * N) and c['n_extreme'] == ((pit < 0.025) | (pit > 0.975)).sum()
    assert set(c) == {'pit', 'n_extreme', 'chi2_mean', 'chi2_reduced', 'p_chi2', 'p_max', 'sign_changes', 'p_runs', 'n_rows'}
    with pytest.raises(ValueError, match='R, 2, N'):
        pp.predictive_sums(np.zeros((4, 3, 5)), 0.0, 1.0)


# -- calibration ----------------------------------------------------------------------------------------------------
def kolmogorov_distance(p):
    p = np.sort(np.asarray(p))
    n = p.size
    return max(np.max(np.arange(1, n + 1) / n - p), np.max(p - np.arange(n) / n))


@pytest.mark.parametrize('N', (3, 8, 20))
def test_calibration_on_data_drawn_from_the_model(N):
    """y = Z0 + sigma eps, the chain sitting on the truth: p_chi2, p_max and the pit of a point are uniform, and the sign
    changes are 2N - 2 fair coins.  400 seeds: the 1 % point of Kolmogorov's distance is 1.63 / sqrt(400)."""
    Z0 = responses(1, 1, N)[0]                                           # (1, 2, N): one row
    sigma = 0.01 * np.abs(Z0[0]) + 1e-3
    p_chi2, p_max, pit00, C = [], [], [], []
    for seed in range(1000, 1400):
        eps = np.random.default_rng(seed).standard_normal((2, N))
        c = pp.predictive_check(Z0, Z0[0] + sigma * eps, sigma)
        p_chi2.append(c['p_chi2'])
        p_max.append(c['p_max'])
        pit00.append(c['pit'][0, 0])
        C.append(int(np.argmax(c['sign_changes'])))
        assert c['sign_changes'].sum() == 1
    dist = [kolmogorov_distance(v) for v in (p_chi2, p_max, pit00)]
    print(f'N = {N}: Kolmogorov distances {dist[0]:.3f}, {dist[1]:.3f}, {dist[2]:.3f}; mean C {np.mean(C):.3f}')
    assert max(dist) < 1.63 / math.sqrt(400)
    assert abs(np.mean(C) - (N - 1)) <= 4 * math.sqrt((2 * N - 2) / 4 / 400)


# -- the device's order, restated -----------------------------------------------------------------------------------
# (E, rows, N): the plans of tests/test_gpu_predictive.py -- rows on both sides of a run of 64 slots and of the 256 slots,
# one row, one above the segment minimum, ragged segments; E = 256 is the first count that takes one segment; N = 1 and
# N on both sides of the point pass's tile of 8
SHAPES = [(1, 1, 3), (1, 1, 1), (1, 63, 4), (1, 64, 9), (1, 65, 8), (3, 65, 5), (1, 255, 2), (1, 256, 2), (1, 257, 3),
          (1, 1024, 2), (1, 1025, 3), (3, 1025, 2), (1, 2500, 6), (1, 500, 32), (256, 27, 2), (256, 1, 1)]


def check_ordered(Z, y, err, what, n_spectra=None):
    """ordered_predictive_sums within the bounds of the yardstick, and the definition on every spectrum within its own:
    equal counts, and chi2_mean, p_chi2, p_max, pit of the two within the sum of the bounds."""
    iv = inverse_variance(err)
    pit, row, hist = pp.ordered_predictive_sums(Z, y, iv, n_spectra)
    ref = pb.reference_and_bounds(Z, y, iv, pb.K_NUMPY)
    worst = pb.assert_all_within(pit, row, ref, what)
    print(f'{what}: pit, chi2_mean, p_chi2, p_max at most {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f}, {worst[3]:.3f} of their bounds')
    np.testing.assert_array_equal(hist.sum(axis=1), ref['good'].sum(axis=1))
    ref_d = pb.reference_and_bounds(Z, y, iv, pb.K_NUMPY, pb.K_ARG_DEFINITION)
    d = [pp.predictive_sums(Z[e], y[e], iv[e]) for e in range(Z.shape[0])]
    pb.assert_all_within(np.stack([a[0] for a in d]), np.stack([a[1] for a in d]), ref_d, what + ' (definition)')
    np.testing.assert_array_equal(np.stack([a[2] for a in d]), hist)
    return (pit, row, hist), ref


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ordered_sums_against_the_yardstick(shape):
    E, R, N = shape
    Z = responses(E, R, N)
    y, err = data_for(Z)
    (pit, row, hist), ref = check_ordered(Z, y, err, str(shape))
    assert pit.shape == (E, 2, N) and row.shape == (E, 3) and hist.shape == (E, 2 * N - 1) and hist.dtype == np.int64
    assert np.isfinite(pit).all() and np.isfinite(row).all() and (hist.sum(axis=1) == R).all()
    assert ((pit >= 0) & (pit <= 1)).all() and ((row[:, 1:] >= 0) & (row[:, 1:] <= 1)).all()
    if E == 1:
        for a, b in zip(pp.ordered_predictive_sums(Z[0], y[0], inverse_variance(err[0])), (pit, row, hist)):
            np.testing.assert_array_equal(a, b)


def test_ordered_sums_take_both_branches_of_q():
    Z = responses(1, 700, 6, seed=3)
    y, err = data_for(Z, seed=3)
    _, ref = check_ordered(Z, y, err, 'both branches')
    assert ref['x_min'][0] < 6 <= ref['x_max'][0]


def test_phi_and_q_underflow_to_zero():
    """The error of one point shrunk until the measurement lies some 50 sigma below every row's response: Phi of that point
    and Q of every row underflow to exactly 0, and p_max too."""
    Z = responses(1, 300, 3, seed=5)
    y, err = data_for(Z, seed=5)
    err[0, 0, 1] = 1e-4
    y[0, 0, 1] = Z[0, :, 0, 1].min() - 50 * err[0, 0, 1]
    (pit, row, hist), ref = check_ordered(Z, y, err, 'underflow')
    assert pit[0, 0, 1] == 0.0 and row[0, 1] == 0.0 and row[0, 2] == 0.0 and ref['x_min'][0] > 1200
    assert np.isfinite(row).all() and hist.sum() == 300


def test_a_residual_of_exactly_zero():
    Z = responses(1, 70, 4, seed=2)
    y, err = data_for(Z, seed=2)
    Z[0, 5] = y[0]                                                       # a row on the data: T = 0, Q = p_max = 1, C = 0
    Z[0, 9:20, 1, 2] = y[0, 1, 2]
    (pit, row, hist), _ = check_ordered(Z, y, err, 'd = 0')
    assert hist[0, 0] >= 1


def test_all_rows_equal():
    Z = responses(1, 700, 3, seed=5)
    Z[0, :] = Z[0, 0]
    y, err = data_for(Z, seed=5)
    (pit, row, hist), ref = check_ordered(Z, y, err, 'all rows equal')
    one = pp.ordered_predictive_sums(Z[:, :1], y, inverse_variance(err))
    assert hist.max() == 700 and (hist > 0).sum() == 1
    tol = (ref['dpit'] + pb.reference_and_bounds(Z[:, :1], y, inverse_variance(err), pb.K_NUMPY)['dpit']).astype(np.float64)
    assert (np.abs(pit - one[0]) <= tol).all()


def test_a_nan_row_stays_in_its_spectrum():
    Z = responses(3, 300, 4)
    y, err = data_for(Z)
    iv = inverse_variance(err)
    clean = pp.ordered_predictive_sums(Z, y, iv)
    Z[1, 17] = np.nan
    pit, row, hist = pp.ordered_predictive_sums(Z, y, iv)
    assert np.isnan(pit[1]).all() and np.isnan(row[1]).all() and hist[1].sum() == 299
    for a, b in zip((pit, row, hist), clean):
        np.testing.assert_array_equal(a[[0, 2]], b[[0, 2]])
    d = pp.predictive_check(Z[1], y[1], err[1])
    assert np.isnan(d['pit']).all() and np.isnan(d['p_chi2']) and d['n_rows'] == 299 and np.isfinite(d['p_runs'])
    np.testing.assert_array_equal(d['sign_changes'], hist[1])
    Z[1, 17, 0, 2] = np.inf                                              # a row whose T is not finite
    assert pp.ordered_predictive_sums(Z, y, iv)[2][1].sum() == 299


# -- plumbing -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ('bisip_predictive_check_workspace', 'bisip_predictive_check_dev')


def test_entry_points_exist(hip_lib):
    import __graft_entry__ as entry
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    for name in NEW_ENTRIES:
        assert hasattr(hip_lib, name) and name in _hip.SYMBOLS
        assert re.search(r'\b%s\(' % name, header) and name in exports
    assert _hip.SYMBOLS['bisip_predictive_check_dev'] == _hip.SYMBOLS['bisip_fit_quality_dev']      # the same shape of call
    assert _hip.SYMBOLS['bisip_predictive_check_workspace'] == _hip.SYMBOLS['bisip_fit_quality_workspace']
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6      # an addition under the same number
    for method in ('predictive_check_workspace', 'predictive_check_dev'):
        assert callable(getattr(_hip.HipContext, method))
    unit = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'dispatch_predictive.hip')).read()
    assert 'with_model(' in unit and 'rm_plan(' in unit and 'check_response_shape(' in unit and 'eval_const<M>' in unit


def test_signatures():
    import bisip_amd
    from bisip_amd.summaries import DeviceChainSummaries
    sig = lambda f: str(inspect.signature(f))
    assert sig(DeviceChainSummaries.predictive_check) == '(self, discard=0, thin=1)'
    assert sig(pp.device_predictive_check) == '(view, ctx, first_spectrum=0)'
    assert sig(pp.ordered_predictive_sums) == '(Z, y, iv, n_spectra=None)'
    assert sig(pp.predictive_sums) == '(Z, y, iv)'
    for cls in (bisip_amd.PolynomialDecomposition, bisip_amd.PeltonColeCole, bisip_amd.Dias2000, bisip_amd.Shin2015):
        assert issubclass(cls, pp.ModelPredictive)
        for name in ('get_predictive_check', 'get_pit'):
            assert sig(getattr(cls, name)) == '(self, chain=None, **kwargs)'
            assert name not in vars(cls) and name not in vars(bisip_amd.utils.utils)
    B = bisip_amd.SpectraBatch
    assert issubclass(B, pp.BatchPredictive)
    for name in ('get_predictive_check', 'get_pit'):
        assert sig(getattr(B, name)) == '(self, discard=0, thin=1)' and name not in vars(B)
    for name in ('normal_cdf', 'chi2_sf_even', 'max_abs_sf', 'sign_changes', 'binomial_half_cdf', 'predictive_sums',
                 'predictive_check', 'ordered_predictive_sums', 'device_predictive_check', 'ModelPredictive', 'BatchPredictive'):
        assert name in pp.__all__ and hasattr(pp, name)


def test_errors_of_an_unfitted_model_and_of_chain_with_discard():
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389175']
    m = bisip_amd.PeltonColeCole(path, n_modes=1, nwalkers=8, nsteps=5)
    calls = (m.get_predictive_check, m.get_pit)
    for call in calls:
        with pytest.raises(AssertionError, match='not fitted'):
            call()
    chain = np.tile(0.5 * (m.param_bounds[0] + m.param_bounds[1]), (6, 1))
    for call in calls:
        with pytest.raises(ValueError, match='Do not pass both'):
            call(chain=chain, discard=2)
        with pytest.raises(ValueError, match='Flatten chain'):
            call(chain=chain.reshape(3, 2, -1))
