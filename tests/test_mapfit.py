"""bisip_amd.mapfit on the CPU: lm_fit over the CPU oracle's forward against scipy's trust-region least squares from the same
starts on the five bundled cases, the bound handling, the dense step of the host entry point (bisip_lm_step_host, the functions
the kernel shares) against the NumPy definition bit for bit, the normal equations against the long-double yardstick of
tests/map_bounds.py (and that against mpmath.diff), the ball of walkers, the Laplace evidence against its formula, the plumbing,
and the dense step under AddressSanitizer + UBSan in a program of its own."""
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_bounds as mb
from bisip_amd import mapfit as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def fitted(case_id):
    """lm_fit over the oracle's forward from the 32 starts of the case, at most 60 iterations, pred_tol = 0 (a start runs until
    no candidate lowers chi2: stopping at a predicted decrease of 1e-8, the default, cannot promise the 1e-9 that the comparison
    with scipy asks for -- Dias2000's valley is descended linearly and ends 2.3e-8 above the optimum then):
    (model, problem, starts, result)."""
    import oracle
    case = mb.CASES[mb.CASE_IDS.index(case_id)]
    m = mb.model_of(case)
    prob = mb.oracle_problem(m)
    starts = mb.starts_of(m)
    res = mf.lm_fit(lambda th: oracle.forward(prob, th), m.data['zn'], mb.inverse_variance(m.data['zn_err']), m.param_bounds, starts,
                     max_iter=60, pred_tol=0.0)
    return m, prob, starts, res


# -- the algorithm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id', mb.CASE_IDS)
def test_lm_fit_against_scipy(case_id):
    """The best chi2 within 1e-9 of scipy's trf best from the same starts on the inner box; at least 20 of 32 starts within
    1e-6 of the best."""
    optimize = pytest.importorskip('scipy.optimize')
    import oracle
    m, prob, starts, res = fitted(case_id)
    d = m.data
    sw = np.sqrt(mb.inverse_variance(d['zn_err']))
    _, lo_in, hi_in = mf.inner_box(m.param_bounds)
    resid = lambda th: ((d['zn'] - oracle.forward(prob, th[None])[0]) * sw).ravel()
    best = np.inf
    for s in mf.clip(starts, lo_in, hi_in):
        r = optimize.least_squares(resid, s, bounds=(lo_in, hi_in), method='trf', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
        best = min(best, 2.0 * r.cost)
    ours = res['chi2'].min()
    agree = int(np.sum(res['chi2'] <= ours + 1e-6))
    print(f'{case_id}: chi2 {ours:.12g}, scipy {best:.12g}, difference {ours - best:.2e}; {agree} of 32 starts agree; '
          f'median iterations {np.median(res["iterations"])}; status counts {np.bincount(res["status"], minlength=3)}')
    assert abs(ours - best) <= 1e-9
    assert agree >= 20
    assert (res['iterations'] <= 60).all() and set(res['status']) <= {0, 1, 2}
    assert ((res['theta'] >= lo_in) & (res['theta'] <= hi_in)).all()


def test_one_mode_cole_cole_ends_on_the_bound():
    m, _, _, res = fitted('cc1')
    b = m.param_bounds
    _, lo_in, _ = mf.inner_box(b)
    best = res['theta'][np.argmin(res['chi2'])]
    j = m.param_names.index('log_tau1')
    assert best[j] == lo_in[j]
    raw = dict(res, logp=-0.5 * res['chi2'])
    out = mf.summarize(raw, b)
    assert out['at_bound'][j] and out['at_bound'].sum() == 1
    assert np.isnan(out['cov'][j]).all() and np.isnan(out['cov'][:, j]).all() and np.isnan(out['log_evidence_laplace'])
    free = ~out['at_bound']
    np.testing.assert_allclose(out['cov'][np.ix_(free, free)] @ out['hessian'][np.ix_(free, free)], np.eye(3), atol=1e-8)
    assert out['n_agree'] == int(np.sum(res['chi2'] <= res['chi2'].min() + 1e-6)) and out['status'] in mf.STATUS.values()


def test_max_iter_and_cap():
    import oracle
    m, prob, starts, _ = fitted('cc2')
    fwd = lambda th: oracle.forward(prob, th)
    y, iv = m.data['zn'], mb.inverse_variance(m.data['zn_err'])
    res = mf.lm_fit(fwd, y, iv, m.param_bounds, starts[:4], max_iter=3, pred_tol=0.0)
    assert (res['iterations'] <= 3).all() and (res['status'][res['iterations'] == 3] == 2).all()
    zero = mf.lm_fit(fwd, y, iv, m.param_bounds, starts[:4], max_iter=0)
    _, lo_in, hi_in = mf.inner_box(m.param_bounds)
    np.testing.assert_array_equal(zero['theta'], mf.clip(starts[:4], lo_in, hi_in))
    assert (zero['status'] == 2).all() and (zero['iterations'] == 0).all()
    assert (res['chi2'] <= zero['chi2']).all()
    with pytest.raises(ValueError):
        mf.lm_fit(fwd, y, iv, m.param_bounds, starts[:1], max_iter=1001)
    with pytest.raises(ValueError, match='not finite'):
        mf.lm_fit(fwd, y, iv, np.array([np.full(7, -np.inf), np.full(7, np.inf)]), starts[:1])


# -- the dense step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id', mb.CASE_IDS)
def test_host_step_is_the_numpy_definition(case_id):
    """bisip_lm_step_host (lm_step.h, what the kernel calls) against mapfit's NumPy step at the results of every start: the
    fixed set, pred, delta and the trial bit for bit, for a damping that works, a huge one and none."""
    from bisip_amd import _hip
    m, _, _, res = fitted(case_id)
    b = m.param_bounds
    _, lo_in, hi_in = mf.inner_box(b)
    for s in range(0, 32, 3):
        A, g, th = res['hessian'][s], res['g'][s], res['theta'][s]
        fixed = mf.fixed_mask(th, g, A, lo_in, hi_in)
        for lam in (0.0, 1e-3, 10.0, 1e8):
            got = _hip.lm_step_host(A, g, th, b, lam)
            np.testing.assert_array_equal(got['fixed'], fixed)
            assert bits(got['pred']) == bits(mf.lm_pred(A, g, fixed))
            want = mf.lm_candidate(A, g, th, fixed, lam, lo_in, hi_in)
            assert got['ok'] == (want is not None)
            if want is not None:
                np.testing.assert_array_equal(bits(got['delta']), bits(want[0]))
                np.testing.assert_array_equal(bits(got['trial']), bits(want[1]))
            else:
                assert np.isnan(got['delta']).all() and np.isnan(got['trial']).all()


def test_dense_step_in_words():
    from bisip_amd import _hip
    A = np.array([[4.0, 2.0], [2.0, 3.0]])
    g = np.array([-2.0, 1.0])
    b = np.array([[0.0, 0.0], [1.0, 1.0]])
    h, lo_in, hi_in = mf.inner_box(b)
    np.testing.assert_array_equal(h, [1e-6, 1e-6])
    th = np.array([0.5, 0.5])
    got = _hip.lm_step_host(A, g, th, b, 0.0)
    np.testing.assert_allclose(got['delta'], np.linalg.solve(A, -g), rtol=1e-14)
    assert got['pred'] == pytest.approx(0.5 * g @ np.linalg.solve(A, g), rel=1e-14) and not got['fixed'].any() and got['ok']
    # on the lower bound with the gradient pushing out: fixed; pushing in: free; a zero diagonal: left out
    on = np.array([lo_in[0], 0.5])
    assert list(_hip.lm_step_host(A, np.array([2.0, 1.0]), on, b, 0.0)['fixed']) == [True, False]
    assert list(_hip.lm_step_host(A, g, on, b, 0.0)['fixed']) == [False, False]
    assert list(_hip.lm_step_host(np.array([[4.0, 0.0], [0.0, 0.0]]), np.array([1.0, -0.0]), th, b, 0.0)['fixed']) == [False, True]
    # a huge step is clipped onto the inner box
    far = _hip.lm_step_host(A, 1e3 * g, th, b, 0.0)
    assert far['trial'][0] == hi_in[0] and far['trial'][1] == lo_in[1]
    # not positive definite: pred = +inf, no candidate without damping, one with
    S = np.array([[1.0, 2.0], [2.0, 4.0]])
    bad = _hip.lm_step_host(S, g, th, b, 0.0)
    assert bad['pred'] == np.inf and not bad['ok'] and mf.lm_pred(S, g, np.zeros(2, bool)) == np.inf
    assert _hip.lm_step_host(S, g, th, b, 1.0)['ok']
    with pytest.raises(ValueError):
        _hip.lm_step_host(np.eye(17), np.zeros(17), np.zeros(17), np.zeros((2, 17)), 0.0)


# -- the normal equations ---------------------------------------------------------------------------------------------------
def colecole_points(K, n=64):
    import oracle
    m = mb.model_of(mb.CASES[2 if K == 1 else 1])
    theta, bounds = mb.points(K, n)
    d = m.data
    prob = oracle.OracleProblem('PeltonColeCole', d['w'], d['zn'], d['zn_err'], bounds, n_modes=K)
    h, _, _ = mf.inner_box(bounds)
    Z = oracle.forward(prob, mf.stencil(theta, h).reshape(-1, theta.shape[1])).reshape(n, 2 * theta.shape[1] + 1, 2, -1)
    return m, theta, bounds, h, Z


@pytest.mark.parametrize('K', (1, 2))
def test_normal_equations_against_the_long_double_yardstick(K):
    m, theta, bounds, h, Z = colecole_points(K)
    y, iv = m.data['zn'], mb.inverse_variance(m.data['zn_err'])
    ref = mb.yardstick(theta, m.data['w'], K, y, iv, bounds)
    own = mb.scaled_errors(mf.normal_equations(Z, y, iv, h), ref)
    ordered = mb.scaled_errors(mf.ordered_normal_equations(Z, y, iv, h), ref)
    print(f'K = {K}: the definition {own:.3e}, the ordered restatement {ordered:.3e} of the scale')
    assert own <= mb.OWN, f'the definition\'s own error {own:.3e} is above the figure written down'
    assert ordered <= mb.FACTOR * mb.OWN
    # one point alone gives the bits of the batch, and symmetric A
    c1, g1, A1 = mf.ordered_normal_equations(Z[3], y, iv, h)
    c, g, A = mf.ordered_normal_equations(Z, y, iv, h)
    assert bits(c1) == bits(c[3]) and (bits(g1) == bits(g[3])).all() and (bits(A1) == bits(A[3])).all()
    np.testing.assert_array_equal(bits(A), bits(np.swapaxes(A, -1, -2)))
    np.testing.assert_array_equal(bits(c), bits(mf.ordered_chi2(Z[:, 0], y, iv)))


def test_the_yardstick_against_mpmath():
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 40
    K = 2
    m, theta, bounds, h, _ = colecole_points(K, 4)
    w = m.data['w']
    J = mb.yardstick(theta, w, K, m.data['zn'], mb.inverse_variance(m.data['zn_err']), bounds)[3]

    def response(t, wf):
        z = sum(t[1 + k] * (1 - 1 / (1 + (mp.mpc(0, 1) * wf * mp.exp(t[1 + K + k])) ** t[1 + 2 * K + k])) for k in range(K))
        return t[0] * (1 - z)

    worst = 0.0
    for i in range(theta.shape[0]):
        t0 = [mp.mpf(float(x)) for x in theta[i]]
        for j in range(theta.shape[1]):
            exact = np.array([complex(mp.diff(lambda x: response(t0[:j] + [x] + t0[j + 1:], mp.mpf(float(wf))), t0[j])) for wf in w])
            got = J[i, j, 0].astype(np.float64) + 1j * J[i, j, 1].astype(np.float64)
            worst = max(worst, float(np.max(np.abs(got - exact)) / np.max(np.abs(exact))))
    print(f'the central difference in long double against mpmath.diff: {worst:.2e} of max |dZ_j|')
    assert worst <= mb.DIFF_RTOL


def test_a_point_that_is_not_finite():
    m, theta, bounds, h, Z = colecole_points(1, 4)
    y, iv = m.data['zn'], mb.inverse_variance(m.data['zn_err'])
    clean = mf.ordered_normal_equations(Z, y, iv, h)
    Z[1] = np.nan
    c, g, A = mf.ordered_normal_equations(Z, y, iv, h)
    assert np.isnan(c[1]) and np.isnan(g[1]).all() and np.isnan(A[1]).all()
    for a, b in zip((c, g, A), clean):
        np.testing.assert_array_equal(bits(a[[0, 2, 3]]), bits(b[[0, 2, 3]]))


# -- the ball, the Laplace evidence -------------------------------------------------------------------------------------------
def test_ball():
    from bisip_amd.sampler import walkers_independent
    m, _, _, res = fitted('cc1')
    b = m.param_bounds
    out = mf.summarize(dict(res, logp=-0.5 * res['chi2']), b)
    for nwalkers in (8, 32, 500):
        p0 = mf.ball(out['theta'], out['cov'], out['at_bound'], b, nwalkers, np.random.RandomState(3))
        assert p0.shape == (nwalkers, 4) and ((p0 > b[0]) & (p0 < b[1])).all() and walkers_independent(p0)
    p0 = mf.ball(out['theta'], out['cov'], out['at_bound'], b, 4000, np.random.RandomState(4))
    j = int(np.flatnonzero(out['at_bound'])[0])
    free = ~out['at_bound']
    # the free parameters have the Laplace covariance; the one on the bound (half its draws fall outside and are redrawn)
    # stays within a few times 1e-3 of its range
    np.testing.assert_allclose(np.cov(p0[:, free].T), out['cov'][np.ix_(free, free)], rtol=0.15, atol=0.15 * np.sqrt(
        np.outer(np.diag(out['cov'])[free], np.diag(out['cov'])[free])).max())
    assert np.abs(p0[:, j] - out['theta'][j]).max() < 6e-3 * (b[1, j] - b[0, j])
    same = mf.ball(out['theta'], out['cov'], out['at_bound'], b, 4000, np.random.RandomState(4))
    np.testing.assert_array_equal(p0, same)
    # a covariance that is no use: every parameter takes 1e-3 of its range; a box the ball misses: uniform draws
    p0 = mf.ball(out['theta'], np.full((4, 4), np.nan), np.zeros(4, bool), b, 64, np.random.RandomState(5))
    assert ((p0 > b[0]) & (p0 < b[1])).all() and walkers_independent(p0)
    assert (np.abs(p0 - out['theta']) < 6e-3 * (b[1] - b[0])).all()
    tiny = np.array([b[0], b[0] + 1e-9 * (b[1] - b[0])])
    p0 = mf.ball(out['theta'], 1e-4 * np.eye(4), np.zeros(4, bool), tiny, 16, np.random.RandomState(6))
    assert ((p0 > tiny[0]) & (p0 < tiny[1])).all()


def test_uniform_starts_leave_the_global_state_alone():
    b = np.array([[0.0, -1.0], [1.0, 1.0]])
    np.random.seed(11)
    before = np.random.get_state()
    a = mf.uniform_starts(b, (5,), seed=3)
    c = mf.uniform_starts(b, (2, 5), seed=None)
    after = np.random.get_state()
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]
    np.testing.assert_array_equal(a, np.random.RandomState(3).uniform(b[0], b[1], (5, 2)))
    assert c.shape == (2, 5, 2) and ((c >= b[0]) & (c <= b[1])).all()


def test_log_evidence_laplace_against_its_formula():
    rng = np.random.default_rng(2)
    n = 5
    J = rng.standard_normal((12, n))
    A = J.T @ J
    b = np.array([np.full(n, -2.0), np.linspace(1.0, 3.0, n)])
    logp = -3.25
    cov, lz = mf.laplace(logp, A, np.zeros(n, bool), b)
    want = logp + 0.5 * n * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(A)[1] - np.sum(np.log(b[1] - b[0]))
    assert lz == pytest.approx(want, rel=1e-13)
    np.testing.assert_allclose(cov, np.linalg.inv(A), rtol=1e-10)
    # a Gaussian likelihood inside a wide box: the Laplace evidence is the integral itself
    at = np.array([False, True, False, False, False])
    cov, lz = mf.laplace(logp, A, at, b)
    assert np.isnan(lz) and np.isnan(cov[1]).all() and np.isnan(cov[:, 1]).all()
    np.testing.assert_allclose(cov[np.ix_(~at, ~at)], np.linalg.inv(A[np.ix_(~at, ~at)]), rtol=1e-10)
    cov, lz = mf.laplace(logp, np.ones((n, n)), np.zeros(n, bool), b)           # not positive definite
    assert np.isnan(cov).all() and np.isnan(lz)


# -- plumbing ------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ('bisip_gauss_newton_dev', 'bisip_map_fit_dev', 'bisip_lm_step_host')


def test_entry_points_exist(hip_lib):
    import __graft_entry__ as entry
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    for name in NEW_ENTRIES:
        assert hasattr(hip_lib, name) and name in _hip.SYMBOLS
        assert re.search(r'\b%s\(' % name, header) and name in exports
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6      # an addition under the same number
    for method in ('gauss_newton_dev', 'map_fit_dev'):
        assert callable(getattr(_hip.HipContext, method))
    unit = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'dispatch_map.hip')).read()
    assert 'with_model(' in unit and 'eval_const<M>' in unit and 'lm_step.h' in unit and 'lm_candidate(' in unit
    step = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'lm_step.h')).read()
    assert 'fma(' not in step.replace('no fma', '')
    assert f'LM_CANDIDATES = {mf.CANDIDATES};' in step and f'LM_MAX_ITER = {mf.MAX_ITER};' in step


def test_signatures():
    import bisip_amd
    sig = lambda f: str(inspect.signature(f))
    want = '(self, n_starts=32, starts=None, seed=None, max_iter=60, pred_tol=1e-08)'
    for cls in (bisip_amd.PolynomialDecomposition, bisip_amd.PeltonColeCole, bisip_amd.Dias2000, bisip_amd.Shin2015):
        assert issubclass(cls, mf.ModelMapFit) and sig(cls.fit_map) == want and sig(cls.get_map) == '(self)'
    assert issubclass(bisip_amd.SpectraBatch, mf.BatchMapFit) and sig(bisip_amd.SpectraBatch.fit_map) == want
    assert sig(mf.lm_fit) == '(forward, y, iv, bounds, starts, max_iter=60, pred_tol=1e-08)'
    assert sig(mf.device_map_fit) == '(ctx, starts, max_iter=60, pred_tol=1e-08, first_spectrum=0)'
    assert sig(mf.ball) == '(theta, cov, at_bound, bounds, nwalkers, rng)'
    assert sig(mf.ordered_normal_equations) == sig(mf.normal_equations) == '(Z, y, iv, h)'
    for name in mf.__all__:
        assert hasattr(mf, name)
    m = mb.model_of(mb.CASES[2])
    with pytest.raises(AssertionError, match='No MAP fit yet'):
        m.get_map()
    with pytest.raises(ValueError, match="'map'"):
        m.fit(p0='mode')


def test_refusals_before_any_launch(hip_lib):
    """Null contexts and pointers are refused on the host."""
    assert hip_lib.bisip_gauss_newton_dev(None, 0, 1, None, 1, None, None, None, None) == -1
    assert hip_lib.bisip_map_fit_dev(None, 0, 1, None, 1, 60, 1e-8, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.bisip_lm_step_host(0, None, None, None, None, None, 0.0, None, None, None, None, None) == -1
    assert hip_lib.bisip_lm_step_host(2, None, None, None, None, None, 0.0, None, None, None, None, None) == -1


# -- sanitizers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_dense_step_under_asan_ubsan(tmp_path):
    """lm_step.h is plain C++: a stand-alone program of its own runs it for ndim 1, 2 and 16, a singular A, an empty free set,
    a parameter of zero sensitivity and a NaN, on buffers of the exact size, under AddressSanitizer + UBSan."""
    exe = tmp_path / 'sanitize_lm_step'
    build = subprocess.run(['g++', '-std=gnu++17', '-O1', '-g', '-fno-omit-frame-pointer', '-ffp-contract=off',
                            '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe),
                            os.path.join(ROOT, 'tests', 'native', 'sanitize_lm_step.cpp')],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'sanitize_lm_step: ok' in run.stdout
