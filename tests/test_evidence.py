"""bisip_amd.evidence on the CPU: the bridge-sampling estimate against targets of known evidence, its standard error against
the scatter over seeds, the overflow ends of the iteration, the NumPy restatements of the device's order, and the plumbing.
The bounds are tests/evidence_bounds.py's."""
import os
import re

import numpy as np
import pytest

import evidence_bounds as eb
from bisip_amd import evidence as ev
from conftest import ROOT

SEEDS = range(24)
DIMS = (1, 7, 16)
N_HALF, WP = 4000, 8               # 4,000 + 4,000 rows arranged as (n, Wp) = (1000, 8)


# -- the targets ------------------------------------------------------------------------------------------------------------
def precision(d):
    """A fixed precision matrix A (d, d) of condition number near 20, and the log evidence of exp(-0.5 x' A x)."""
    rng = np.random.default_rng([d, 99])
    Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    A = (Q * np.linspace(0.5, 10.0, d)) @ Q.T
    A = (A + A.T) / 2
    return A, 0.5 * d * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(A)[1]


def gauss_logp(A):
    return lambda t: -0.5 * np.einsum('...i,ij,...j->...', t, A, t)


def box_logp(t):
    return np.where(((t > 0) & (t < 1)).all(axis=-1), 0.0, -np.inf)


def gauss_rows(A, rng, shape):
    """iid rows of N(0, inv(A))."""
    C = np.linalg.cholesky(np.linalg.inv(A))
    return rng.normal(size=shape + (A.shape[0],)) @ C.T


def ar1_rows(A, rng, n, Wp, rho):
    """Wp independent AR(1) walkers, n steps, stationary in N(0, inv(A))."""
    d = A.shape[0]
    C = np.linalg.cholesky(np.linalg.inv(A))
    z = np.empty((n, Wp, d))
    z[0] = rng.normal(size=(Wp, d))
    eps = rng.normal(size=(n, Wp, d)) * np.sqrt(1 - rho * rho)
    for k in range(1, n):
        z[k] = rho * z[k - 1] + eps[k]
    return z @ C.T


def conditions(errors, ses, what):
    errors, ses = np.asarray(errors), np.asarray(ses)
    worst = (np.abs(errors) / ses).max()
    ratio = np.sqrt(np.mean(errors ** 2)) / ses.mean()
    print(f'{what}: worst |error| / se {worst:.2f}, rms error / mean se {ratio:.2f}, mean se {ses.mean():.3e}')
    return worst, ratio


# -- exact proposal, exact answer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', DIMS)
def test_the_exact_proposal_gives_the_exact_answer(d):
    """q = exp(-0.5 x' A x) with the proposal N(0, inv(A)): l1 and l2 are the constant log_ml up to rounding, F(r) does not
    depend on r but for it, so the first pass lands on the fixed point.  Every l is off by at most logg_bound (the stored
    logp is the exact one rounded, u |logp|) plus the rounding of its own subtraction, and the estimate moves by no more
    than its entries do (evidence_bounds); exp, the sums of one pass and log r add (K_exp + K_log |log r|) u and eta."""
    A, truth = precision(d)
    cov = np.linalg.inv(A)
    rng = np.random.default_rng([d, 1])
    x = gauss_rows(A, rng, (200, 4))
    exact_logp = lambda t: (-(np.einsum('...i,ij,...j->...', t.astype(eb.LD), A.astype(eb.LD), t.astype(eb.LD))) / 2
                            ).astype(np.float64)
    res = ev.bridge_evidence(x, exact_logp(x), exact_logp, neff=None, proposal=(np.zeros(d), cov), seed=3)
    assert res['iterations'] <= 2 and res['n1'] == 800 == res['n2'] and res['frac_outside'] == 0.0
    mu, L, c = ev.proposal_factor(np.zeros(d), cov)
    theta2, _ = ev.host_draws(mu[0], L[0], c[0], 800, 3)
    rows = np.concatenate([x.reshape(-1, d), theta2])
    z = eb.whiten(rows, mu[0], L[0]).astype(np.float64)
    # the proposal's own L is the rounded factor of a rounded inverse: log_g is exact for THAT normal, whose evidence differs
    # from the truth by the logs of the diagonal (in c) and by z' z against x' A x -- measured in long double, not bounded
    shift = np.abs((exact_logp(rows).astype(eb.LD) - eb.logg_ld(rows, mu[0], L[0], c[0])) - eb.LD(truth)).max()
    lp = np.abs(exact_logp(rows))
    bound = (eb.logg_bound(L[0], c[0], z) + eb.U * (2 * lp + abs(truth))).max() + float(shift)
    bound += (sum(eb.K_NUMPY) * (1 + abs(truth)) + 2) * eb.U + 2 * (eb.gamma(804) + eb.gamma(804))
    print(f'd = {d}: |log_ml - truth| = {abs(res["log_ml"] - truth):.2e}, bound {bound:.2e} (cond L {np.linalg.cond(L[0]):.1f})')
    assert abs(res['log_ml'] - truth) <= bound
    assert bound < 5e-12


# -- fitted proposal, targets of known evidence ---------------------------------------------------------------------------------
def run_seeds(make, logp_fn, truth, **kw):
    errors, ses, results = [], [], []
    for seed in SEEDS:
        x = make(np.random.default_rng([seed, 7]))
        res = ev.bridge_evidence(x, logp_fn(x), logp_fn, seed=seed, **kw)
        errors.append(res['log_ml'] - truth)
        ses.append(res['se'])
        results.append(res)
    return np.array(errors), np.array(ses), results


@pytest.mark.parametrize('d', DIMS)
def test_the_flat_unit_box_has_evidence_one(d):
    errors, ses, results = run_seeds(lambda rng: rng.uniform(size=(2 * N_HALF // WP, WP, d)), box_logp, 0.0, neff=None)
    worst, ratio = conditions(errors, ses, f'box d = {d}')
    assert all(r['frac_outside'] > 0 for r in results) and all(r['n1'] == N_HALF == r['n2'] for r in results)
    assert all(r['iterations'] < 100 for r in results)
    assert worst <= 4 and 0.5 <= ratio <= 2


@pytest.mark.parametrize('d', DIMS)
def test_the_gaussian_has_its_evidence(d):
    A, truth = precision(d)
    errors, ses, results = run_seeds(lambda rng: gauss_rows(A, rng, (2 * N_HALF // WP, WP)), gauss_logp(A), truth, neff=None)
    worst, ratio = conditions(errors, ses, f'gaussian d = {d}')
    assert all(r['iterations'] < 100 for r in results)
    assert worst <= 4 and 0.5 <= ratio <= 2


@pytest.mark.parametrize('d', DIMS)
def test_an_autocorrelated_chain_needs_the_tau_term(d):
    """AR(1) walkers (rho = 0.9) of the Gaussian, the bridge weighted by the number of rows (``neff=None``): with tau of f2
    the standard error matches the scatter over the seeds; with tau forced to 1 it is too small by more than the factor the
    condition allows."""
    A, truth = precision(d)
    make = lambda rng: ar1_rows(A, rng, 2 * N_HALF // WP, WP, 0.9)
    errors, ses, results = run_seeds(make, gauss_logp(A), truth, neff=None)
    worst, ratio = conditions(errors, ses, f'AR(1) d = {d} with tau')
    assert all(r['tau_f2'] > 2 for r in results)
    assert worst <= 4 and 0.5 <= ratio <= 2
    errors1, ses1, _ = run_seeds(make, gauss_logp(A), truth, neff=None, tau=1.0)
    np.testing.assert_array_equal(errors1, errors)                # (tau enters the error estimate alone)
    _, ratio1 = conditions(errors1, ses1, f'AR(1) d = {d} with tau = 1')
    assert ratio1 > 2


def test_an_autocorrelated_chain_with_the_effective_size():
    """The same chain with the default ``neff='ess'``: the bridge leans on the draws and both conditions hold."""
    A, truth = precision(7)
    errors, ses, results = run_seeds(lambda rng: ar1_rows(A, rng, 2 * N_HALF // WP, WP, 0.9), gauss_logp(A), truth)
    worst, ratio = conditions(errors, ses, 'AR(1) d = 7 with neff = ess')
    assert all(r['neff'] < r['n1'] / 4 for r in results)
    assert worst <= 4 and 0.5 <= ratio <= 2


# -- overflow ends ------------------------------------------------------------------------------------------------------------
def pass_ld(l1, l2, lstar, s1, r):
    """One pass F(r) of the iteration from l1, l2 in long double."""
    LD = eb.LD
    l1, l2 = l1.astype(LD), l2.astype(LD)
    s1, r = LD(s1), LD(r)
    s2 = LD(1) - s1
    with np.errstate(all='ignore'):
        f1 = LD(1) / (s1 + s2 * r * np.exp(-(l2 - LD(lstar))))
        f2 = LD(1) / (s1 * np.exp(l1 - LD(lstar)) + s2 * r)
    return f1.mean() / f2.mean()


def test_the_ends_do_not_overflow():
    rng = np.random.default_rng(5)
    l1 = rng.normal(size=401)
    l1[:6] += (800, -800, 800, -800, 745, -745)
    lstar = np.median(l1)
    l2 = lstar + rng.normal(size=300)
    l2[:4] = lstar + np.array([800.0, -800.0, 700.0, -700.0])
    l2[10:20] = -np.inf
    got_lstar, a1, a2 = ev.bridge_terms(l1, l2)
    assert got_lstar == lstar and np.isposinf(a1[10:20]).all() and np.isposinf(a1[1]) and a1[0] == 0.0
    assert np.isposinf(a2[0]) and a2[1] == 0.0
    s1 = 0.6
    for restated in (ev.bridge_iterate, ev.ordered_iterate):
        res = restated(a1, a2, s1)
        assert np.isfinite(res['log_r']) and 1 < res['iterations'] < 100 and np.isfinite(res['moments']).all()
        r = 1.0
        for rn in res['history']:                                 # every pass against the same sums in long double
            want = pass_ld(l1, l2, lstar, s1, r)
            assert abs(eb.LD(rn) - want) <= 1e-14 * want
            r = rn
    for restated in (ev.bridge_iterate, ev.ordered_iterate):
        dead = restated(np.full(7, np.inf), a2, s1)
        assert np.isnan(dead['r']) and np.isnan(dead['log_r']) and dead['iterations'] == 1


# -- the restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', DIMS)
def test_ordered_logg_is_log_g(d):
    """Both are within logg_bound of the exact value, and l = logp - log_g is one more rounding each."""
    A, _ = precision(d)
    rng = np.random.default_rng([d, 2])
    cov = np.linalg.inv(A) * rng.uniform(0.5, 2)
    mu, L, c = ev.proposal_factor(rng.normal(size=d), cov)
    mu, L, c = mu[0], L[0], c[0]
    x = mu + gauss_rows(A, rng, (300,)) * 1.5
    logp = rng.normal(size=300) * 50
    got, plain = ev.ordered_logg(x, logp, mu, L, c), logp - ev.log_g(x, mu, L, c)
    exact = logp.astype(eb.LD) - eb.logg_ld(x, mu, L, c)
    bound = eb.logg_bound(L, c, eb.whiten(x, mu, L).astype(np.float64)) + eb.U * np.abs(plain)
    assert (np.abs(got - exact) <= bound).all() and (np.abs(plain - exact) <= bound).all()
    assert (got != plain).any() or d == 1                          # (a restatement of the ORDER: fma, not the plain sums)


@pytest.mark.parametrize('N1, N2', ((1, 1), (255, 257), (1000, 256)))
def test_ordered_iterate_is_bridge_iterate(N1, N2):
    """The same passes in another order of summation: sums of positive terms, gamma_{N + 4} each relative, so a pass differs
    by eta and the ends by (tol + eta) / (1 - rho) each (evidence_bounds.iterate_bound); the pass count is equal."""
    rng = np.random.default_rng([N1, N2])
    a1, a2 = np.exp(rng.normal(size=N2) * 1.5 + 0.3), np.exp(rng.normal(size=N1) * 1.5)
    plain, got = ev.bridge_iterate(a1, a2, 0.45), ev.ordered_iterate(a1, a2, 0.45)
    assert got['iterations'] == plain['iterations'] and 1 <= got['iterations'] < 200
    bound = eb.iterate_bound(N1, N2, plain['history'], ev.TOL)
    assert abs(got['r'] - plain['r']) <= bound * plain['r']
    eta = 2 * (eb.gamma(N1 + 4) + eb.gamma(N2 + 4)) + bound
    np.testing.assert_allclose(got['moments'][[0, 2]], plain['moments'][[0, 2]], rtol=eta, atol=0)
    np.testing.assert_allclose(got['f2'], plain['f2'], rtol=bound + 4 * eb.U, atol=0)
    for stop in (1, 2):
        assert ev.ordered_iterate(a1, a2, 0.45, maxiter=stop)['iterations'] == min(stop, got['iterations'])


def test_the_draws_are_standard_normal_and_chunk_free():
    mu, L, c = ev.proposal_factor(np.array([1.0, -2.0, 0.5]), np.diag([4.0, 1.0, 0.25]))
    theta, lg = ev.host_draws(mu[0], L[0], c[0], 20000, seed=11)
    z = (theta - mu[0]) / np.array([2.0, 1.0, 0.5])
    assert np.abs(z.mean(axis=0)).max() < 4 / np.sqrt(20000) and np.abs(z.var(axis=0) - 1).max() < 4 * np.sqrt(2 / 20000)
    assert np.abs(np.corrcoef(z.T) - np.eye(3)).max() < 4 / np.sqrt(20000)
    np.testing.assert_allclose(lg, ev.log_g(theta, mu[0], L[0], c[0]), rtol=0, atol=1e-12)
    part = ev.host_draws(mu[0], L[0], c[0], 500, seed=11, first_draw=700)
    np.testing.assert_array_equal(part[0], theta[700:1200])
    assert (ev.host_draws(mu[0], L[0], c[0], 50, seed=12)[0] != theta[:50]).all()
    assert (ev.host_draws(mu[0], L[0], c[0], 50, seed=11, ensemble=1)[0] != theta[:50]).all()
    yard = ev.draw_yardstick(mu[0], L[0], c[0], 2000, seed=11)
    assert yard[0].dtype == np.longdouble and np.abs(yard[0] - theta[:2000]).max() < 1e-14


# -- plumbing -----------------------------------------------------------------------------------------------------------------
def test_compare_evidence_ranks_and_normalises():
    rows = ev.compare_evidence({'a': dict(log_evidence=-3.0, se=0.1), 'b': dict(log_evidence=-1.0, se=0.2),
                                'c': dict(log_evidence=-800.0, se=0.3)})
    assert [r['name'] for r in rows] == ['b', 'a', 'c'] and [r['log_bf'] for r in rows] == [0.0, -2.0, -799.0]
    assert abs(sum(r['prob'] for r in rows) - 1) < 1e-15 and rows[2]['prob'] == 0.0
    assert abs(rows[0]['prob'] - 1 / (1 + np.exp(-2.0))) < 1e-15 and [r['se'] for r in rows] == [0.2, 0.1, 0.3]
    with pytest.raises(ValueError):
        ev.compare_evidence({})
    with pytest.raises(ValueError):
        ev.compare_evidence({'batch': dict(log_evidence=np.zeros(2), se=np.zeros(2))})


def test_the_prior_volume_and_the_gaussian_offset():
    import bisip_amd
    d = 3
    bounds = np.array([[-1.0, 0.0, -5.0], [2.0, 0.5, 5.0]])
    rng = np.random.default_rng(4)
    x = rng.uniform(bounds[0], bounds[1], size=(400, 4, d))
    logp_fn = lambda t: np.where(((t > bounds[0]) & (t < bounds[1])).all(axis=-1), 0.0, -np.inf)
    res = ev.bridge_evidence(x, logp_fn(x), logp_fn, bounds=bounds, neff=None)
    assert res['log_evidence'] == res['log_ml'] - np.log([3.0, 0.5, 10.0]).sum()
    assert abs(res['log_evidence']) <= 4 * res['se']               # the normalised flat prior has evidence 1
    assert ev.bridge_evidence(x, logp_fn(x), logp_fn, neff=None)['log_evidence'] == res['log_ml']
    assert list(res)[:3] == ['log_evidence', 'log_ml', 'se'] and res['proposal_cov'].shape == (d, d)
    data = bisip_amd.utils.load_data(bisip_amd.DataFiles()['SIP-K389175'])
    s = data['zn_err']
    want = sum(0.5 * np.log(v * v) - 0.5 * np.log(2 * np.pi) for v in s.ravel())
    assert s.shape[0] == 2 and abs(ev.gaussian_offset(s) - want) <= 1e-12 * abs(want)
    assert ev.gaussian_offset(np.stack([s, s])).shape == (2,)


def test_too_few_samples_and_a_singular_covariance_are_refused():
    d = 3
    rng = np.random.default_rng(0)
    logp_fn = lambda t: np.zeros(t.shape[:-1])
    with pytest.raises(ValueError, match='too few'):
        ev.bridge_evidence(rng.normal(size=(3, 4, d)), np.zeros((3, 4)), logp_fn)          # n1 = 2, n0 * Wp = 4 < d + 2
    with pytest.raises(ValueError, match='too few'):
        ev.bridge_evidence(rng.normal(size=(2, 8, d)), np.zeros((2, 8)), logp_fn)          # n1 = 1
    assert ev.halves(4, 3, 3) == (2, 2)
    x = rng.normal(size=(40, 4, d))
    x[:, :, 2] = 0.25                                                                        # a parameter that does not move
    with pytest.raises(ValueError, match='spectrum 0.*not positive definite'):
        ev.bridge_evidence(x, np.zeros((40, 4)), logp_fn)
    with pytest.raises(ValueError, match='spectrum 5'):
        ev.proposal_factor(np.zeros((2, 2)), np.array([np.eye(2), [[1.0, 2.0], [2.0, 1.0]]]), first_spectrum=4)
    with pytest.raises(ValueError):
        ev.bridge_evidence(x[:, 0], np.zeros((40, 4)), logp_fn)                             # logp of another shape


NEW_ENTRIES = ('bisip_bridge_logg_dev', 'bisip_bridge_draw_dev', 'bisip_bridge_scale_dev', 'bisip_bridge_iterate_dev')


def test_entry_points_exist_and_refuse_on_the_host(hip_lib):
    """Every refusal happens on the host before anything is launched, so the pointers (never dereferenced) may be anything."""
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    for name in NEW_ENTRIES:
        assert hasattr(hip_lib, name) and name in _hip.SYMBOLS and name in exports
        assert re.search(r'\b%s\(' % name, header)
    p = 4096
    good = dict(chain=p, n=4, stride=70, E=2, Wp=5, ndim=7, logp=p, lstride=10, mean=p, chol=p, const=p, l=p)
    for bad in (dict(chain=0), dict(logp=0), dict(mean=0), dict(chol=0), dict(const=0), dict(l=0), dict(ndim=0), dict(ndim=17),
                dict(stride=69), dict(lstride=9), dict(n=0), dict(E=0), dict(Wp=0), dict(Wp=2 ** 27)):
        a = dict(good, **bad)
        with pytest.raises(ValueError):
            _hip.bridge_logg_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['logp'], a['lstride'], a['mean'],
                                 a['chol'], a['const'], a['l'])
    for args in ((0, p, p, 1, 3, 5, 0, 0, 0, p, p), (p, p, p, 1, 0, 5, 0, 0, 0, p, p), (p, p, p, 1, 17, 5, 0, 0, 0, p, p),
                 (p, p, p, 1, 3, 0, 0, 0, 0, p, p), (p, p, p, 1, 3, 5, 0, 0, 2 ** 32, p, p), (p, p, p, 1, 3, 5, 0, 0, 0, 0, p),
                 (p, p, p, 1, 3, 5, 0, 2 ** 64 - 3, 0, p, p), (p, p, p, 0, 3, 5, 0, 0, 0, p, p)):
        with pytest.raises(ValueError):
            _hip.bridge_draw_dev(*args)
    for args in ((0, 5, p, p, 5, 1, p, 0, p, p), (p, 0, p, p, 5, 1, p, 0, p, p), (p, 5, p, p, 5, 0, p, 0, p, p),
                 (p, 5, p, p, 5, 1, 0, 0, p, p), (p, 5, p, p, 5, 1, p, 0, 0, p)):
        with pytest.raises(ValueError):
            _hip.bridge_scale_dev(*args)
    for args in ((0, 5, p, 5, 1, p, 1e-10, 10, p, p, p), (p, 5, p, 5, 1, p, 1e-10, 0, p, p, p), (p, 5, p, 5, 1, p, -1.0, 10, p, p, p),
                 (p, 5, p, 5, 1, p, float('nan'), 10, p, p, p), (p, 5, p, 0, 1, p, 1e-10, 10, p, p, p),
                 (p, 5, p, 5, 1, p, 1e-10, 10, 0, p, p), (p, 5, p, 5, 1, p, 1e-10, 10, p, p, 0)):
        with pytest.raises(ValueError):
            _hip.bridge_iterate_dev(*args)


def test_the_models_and_the_batch_have_get_evidence():
    import bisip_amd
    from bisip_amd.batch import SpectraBatch
    from bisip_amd.summaries import DeviceChainSummaries
    for cls in (bisip_amd.PeltonColeCole, bisip_amd.PolynomialDecomposition, bisip_amd.Dias2000, bisip_amd.Shin2015, SpectraBatch):
        assert callable(cls.get_evidence)
    assert callable(DeviceChainSummaries.evidence)
