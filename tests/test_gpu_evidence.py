"""Bridge sampling on the device (bisip_bridge_logg_dev, _draw_dev, _scale_dev, _iterate_dev), from the C entry points up to
the model and SpectraBatch methods.  logg and iterate are held, bit for bit, to the order include/bisip_hip.h states
(bisip_amd.evidence.ordered_logg, ordered_iterate); scale and draw, which call the device library, to FACTOR times the
float64 NumPy definition's own worst error against a long-double yardstick over the same inputs (the margin of
tests/loo_bounds.py); get_evidence to the bound tests/evidence_bounds.py adds up."""
import functools

import numpy as np
import pytest

import evidence_bounds as eb
from chain_harness import SENTINEL, GuardedCall, assert_same_bits, shape_id, store

pytestmark = pytest.mark.gpu

LP_PAD = 3                         # the log-probability has a padding of its own
# stored samples of the fits; the first half is burn-in (the three spectra of the batch need some 1000 steps from its start)
STEPS = {'ColeCole': 400, 'PolynomialDecomposition': 1000, 'batch': 1500}


def proposal(E, ndim, seed, tiny=False):
    """(mu (E, ndim), L (E, ndim, ndim), c (E,)) of E random normals; ``tiny``: a diagonal entry of L of 1e-8."""
    from bisip_amd import evidence as ev
    rng = np.random.default_rng([seed, E, ndim])
    B = rng.normal(size=(E, ndim, ndim + 2))
    cov = B @ B.transpose(0, 2, 1) / (ndim + 2) * rng.uniform(0.01, 4.0, size=(E, 1, 1))
    mu, L, c = ev.proposal_factor(rng.normal(size=(E, ndim)), cov)
    L = L + np.triu(rng.normal(size=L.shape), 1)           # the upper triangle is never read: anything may lie there
    if tiny:
        L[0, ndim // 2, ndim // 2] = 1e-8
        c = np.log(np.abs(np.diagonal(L, axis1=1, axis2=2))).sum(axis=1) + 0.5 * ndim * np.log(2 * np.pi)
    return mu, L, c


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype or np.float64)).cuda()


# -- bisip_bridge_logg_dev ------------------------------------------------------------------------------------------------------
LOGG_SHAPES = [(2, 1, 1, 1), (3, 1, 5, 7), (4, 3, 5, 16), (9, 2, 33, 7), (5, 257, 2, 3)]


@functools.lru_cache(maxsize=None)
def logg_case(n, E, Wp, ndim, special):
    from bisip_amd import evidence as ev
    rng = np.random.default_rng([n, E, Wp, ndim])
    mu, L, c = proposal(E, ndim, 1, tiny=special)
    z = rng.normal(size=(n, E, Wp, ndim))
    x = mu[None, :, None, :] + np.einsum('ejk,newk->newj', np.tril(L), z)
    logp = rng.normal(size=(n, E, Wp)) * 30 - 40
    if special:
        logp[0, 0, 0], logp[1, E - 1, Wp - 1], logp[n - 1, 0, Wp // 2] = -np.inf, np.nan, np.inf
        x[1, 0, 0, ndim - 1] = np.nan
    want = np.empty((E, n * Wp))
    for e in range(E):
        want[e] = ev.ordered_logg(x[:, e].reshape(n * Wp, ndim), logp[:, e].reshape(n * Wp), mu[e], L[e], c[e])
    x, logp = x.reshape(n, E * Wp, ndim), logp.reshape(n, E * Wp)
    return store(x), store(logp, pad=LP_PAD, filler=-1e300), (mu, L, c), (x, logp), want


def run_logg(case, shape, **bad):
    n, E, Wp, ndim = shape
    from bisip_amd import _hip
    (samples, off, stride), (lps, loff, lstride), (mu, L, c) = case[:3]
    t, tl, dmu, dL, dc = dev(samples), dev(lps), dev(mu), dev(L), dev(c)
    call = GuardedCall()
    out = call.out('l', (E, n * Wp))
    a = dict(chain=t.data_ptr() + 8 * off, n=n, stride=stride, E=E, Wp=Wp, ndim=ndim, logp=tl.data_ptr() + 8 * loff,
             lstride=lstride, mean=dmu.data_ptr(), chol=dL.data_ptr(), const=dc.data_ptr(), l=out)
    a.update(bad)
    try:
        _hip.bridge_logg_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['logp'], a['lstride'], a['mean'],
                             a['chol'], a['const'], a['l'], call.stream)
    except ValueError:
        assert (call.finish()[0] == SENTINEL).all(), 'a refused call wrote its output'
        raise
    return call.finish()[0]


@pytest.mark.parametrize('special', (False, True), ids=('plain', 'special'))
@pytest.mark.parametrize('shape', LOGG_SHAPES, ids=shape_id)
def test_logg_has_the_bits_of_ordered_logg(shape, special):
    from bisip_amd import evidence as ev
    n, E, Wp, ndim = shape
    case = logg_case(*shape, special)
    got = run_logg(case, shape)
    want = case[4]
    assert not (got == SENTINEL).any()
    assert_same_bits(got, want, f'l {shape}')
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    if special:                                # (in the smallest shape the special entries fall on one another)
        assert np.isneginf(got[0, 0]) and np.isnan(got).any() and not np.isfinite(got).all()
        if n * Wp >= 15:
            assert np.isnan(got[E - 1, Wp + Wp - 1]) and np.isposinf(got[0, (n - 1) * Wp + Wp // 2]) and np.isnan(got[0, Wp])
            assert np.isfinite(got).sum() == got.size - 4
    else:
        assert np.isfinite(got).all()
        # ... and the restated order is the definition within its rounding (evidence_bounds.logg_bound)
        mu, L, c = case[2]
        x, logp = case[3]
        rows = x.reshape(n, E, Wp, ndim)[:, 0].reshape(n * Wp, ndim)
        plain = logp.reshape(n, E, Wp)[:, 0].reshape(n * Wp) - ev.log_g(rows, mu[0], L[0], c[0])
        bound = 2 * eb.logg_bound(L[0], c[0], eb.whiten(rows, mu[0], L[0]).astype(np.float64)) + 2 * eb.U * np.abs(plain)
        assert (np.abs(got[0] - plain) <= bound).all()
    again = run_logg(case, shape)
    np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))


def test_logg_goes_through_tiles_and_segments():
    """1025 rows of one ensemble are two segments, 300 of 257 ensembles one segment of two tiles each: more than one tile
    and tiles that cross samples.  Rows are independent: every row against the definition, a few against the bits."""
    from bisip_amd import evidence as ev
    for shape in ((205, 1, 5, 3), (100, 257, 3, 9)):
        n, E, Wp, ndim = shape
        rng = np.random.default_rng(shape)
        mu, L, c = proposal(E, ndim, 2)
        x = mu[None, :, None, :] + rng.normal(size=(n, E, Wp, ndim)) * 0.3
        logp = rng.normal(size=(n, E, Wp))
        case = (store(x.reshape(n, E * Wp, ndim)), store(logp.reshape(n, E * Wp), pad=LP_PAD), (mu, L, c))
        got = run_logg(case, shape)
        for e in (0, E - 1):
            rows, lp = x[:, e].reshape(n * Wp, ndim), logp[:, e].reshape(n * Wp)
            plain = lp - ev.log_g(rows, mu[e], L[e], c[e])
            bound = 2 * eb.logg_bound(L[e], c[e], eb.whiten(rows, mu[e], L[e]).astype(np.float64)) + 2 * eb.U * np.abs(plain)
            assert (np.abs(got[e] - plain) <= bound).all(), shape
            pick = np.r_[0:3, 254:259, n * Wp - 3:n * Wp]
            assert_same_bits(got[e, pick], ev.ordered_logg(rows[pick], lp[pick], mu[e], L[e], c[e]), str(shape))


@pytest.mark.parametrize('bad', (dict(chain=0), dict(logp=0), dict(mean=0), dict(chol=0), dict(const=0), dict(ndim=0),
                                 dict(ndim=17), dict(stride=3 * 5 * 7 - 1), dict(lstride=14)), ids=str)
def test_logg_refuses_and_writes_nothing(bad):
    shape = (3, 3, 5, 7)
    case = logg_case(*shape, False)
    with pytest.raises(ValueError):
        run_logg(case, shape, **bad)          # (run_logg checks the guards and that nothing of the output was written)
    with pytest.raises(ValueError):
        run_logg(case, shape, l=0)


# -- bisip_bridge_iterate_dev ---------------------------------------------------------------------------------------------------
ITER_SHAPES = [(1, 1, 1), (1, 255, 257), (3, 256, 1000), (2, 1000, 256), (257, 37, 41)]


def iterate_inputs(E, N1, N2, special=False):
    rng = np.random.default_rng([E, N1, N2])
    a1 = np.exp(rng.normal(size=(E, N2)) * 1.5 + rng.normal(size=(E, 1)))
    a2 = np.exp(rng.normal(size=(E, N1)) * 1.5)
    if special and N2 > 4:
        a1[:, ::3] = np.inf
        a2[:, 1::5] = np.inf
        a1[0, 1], a2[0, 0] = 0.0, 0.0
    return a1, a2, rng.uniform(0.2, 0.8, size=E)


def run_iterate(a1, a2, s1, tol=1e-10, maxiter=1000, f2=True):
    import torch
    from bisip_amd import _hip
    E, N2 = a1.shape
    N1 = a2.shape[1]
    call = GuardedCall()
    r, it = call.out('r', (E,)), call.out('iterations', (E,), dtype=torch.int64)
    mom, pf2 = call.out('moments', (E, 4)), call.out('f2', (E, N1), asked=f2)
    d1, d2, ds = dev(a1), dev(a2), dev(s1)
    _hip.bridge_iterate_dev(d1.data_ptr(), N2, d2.data_ptr(), N1, E, ds.data_ptr(), tol, maxiter, r, it, mom, pf2, call.stream)
    return call.finish()


def assert_iterate_bits(got, a1, a2, s1, ensembles, **kw):
    from bisip_amd import evidence as ev
    r, it, mom, f2 = got
    for e in ensembles:
        want = ev.ordered_iterate(a1[e], a2[e], s1[e], **kw)
        assert it[e] == want['iterations'], e
        assert_same_bits(r[e:e + 1], np.array([want['r']]), f'r of ensemble {e}')
        assert np.isnan(r[e]) == np.isnan(want['r'])
        assert_same_bits(mom[e], want['moments'], f'moments of ensemble {e}')
        assert_same_bits(f2[e], want['f2'], f'f2 of ensemble {e}')


@pytest.mark.parametrize('special', (False, True), ids=('plain', 'inf'))
@pytest.mark.parametrize('shape', ITER_SHAPES, ids=shape_id)
def test_iterate_has_the_bits_of_ordered_iterate(shape, special):
    E, N1, N2 = shape
    a1, a2, s1 = iterate_inputs(E, N1, N2, special)
    got = run_iterate(a1, a2, s1)
    assert (got[1] >= 1).all() and (got[1] < 1000).all() and np.isfinite(got[0]).all() and (got[0] > 0).all()
    assert_iterate_bits(got, a1, a2, s1, sorted({0, E // 2, E - 1}))
    again = run_iterate(a1, a2, s1)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)


def test_iterate_stops_at_maxiter_and_ends_dead_ensembles():
    E, N1, N2 = 3, 256, 1000
    a1, a2, s1 = iterate_inputs(E, N1, N2)
    full = run_iterate(a1, a2, s1)
    assert (full[1] > 2).all()
    for stop in (1, 2):
        got = run_iterate(a1, a2, s1, maxiter=stop)
        assert (got[1] == stop).all()
        assert_iterate_bits(got, a1, a2, s1, range(E), maxiter=stop)
    a1[1] = np.inf                                                 # every draw of ensemble 1 outside the box
    got = run_iterate(a1, a2, s1)
    assert np.isnan(got[0][1]) and got[1][1] == 1 and np.isnan(got[2][1]).all() and np.isnan(got[3][1]).all()
    assert_iterate_bits(got, a1, a2, s1, range(E))
    np.testing.assert_array_equal(got[0][[0, 2]], full[0][[0, 2]])
    none = run_iterate(a1, a2, s1, f2=False)                        # (finish() checks that f2 was not written)
    np.testing.assert_array_equal(none[0][[0, 2]], full[0][[0, 2]])
    np.testing.assert_array_equal(none[2][[0, 2]], full[2][[0, 2]])


# -- bisip_bridge_scale_dev -----------------------------------------------------------------------------------------------------
def test_scale_against_the_yardstick():
    """a = exp(t): the float64 definition (np.exp of the same rounded differences) against exp in long double of the exact
    differences, relative; the device is allowed FACTOR times its worst.  +-inf and NaN exactly where the definition has
    them."""
    from bisip_amd import _hip, evidence as ev
    E, N1, N2 = 3, 1000, 777
    rng = np.random.default_rng(12)
    l1 = rng.normal(size=(E, N1)) * 40 - 300
    logp2, logg2 = rng.normal(size=(E, N2)) * 40 - 310, rng.normal(size=(E, N2)) * 5 - 10
    lstar = np.median(l1, axis=1)
    l1[0, :4] = (np.inf, -np.inf, np.nan, 1e4)
    logp2[1, :3] = (-np.inf, np.nan, np.inf)
    logp2[2, 5], logg2[2, 6] = -1e4, -1e4
    with np.errstate(all='ignore'):
        l2 = logp2 - logg2
        d1, d2 = np.exp(-(l2 - lstar[:, None])), np.exp(l1 - lstar[:, None])
    call = GuardedCall()
    pl2, pa1, pa2 = call.out('l2', (E, N2)), call.out('a1', (E, N2)), call.out('a2', (E, N1))
    t = [dev(a) for a in (l1, logp2, logg2, lstar)]
    _hip.bridge_scale_dev(t[0].data_ptr(), N1, t[1].data_ptr(), t[2].data_ptr(), N2, E, t[3].data_ptr(), pl2, pa1, pa2,
                          call.stream)
    gl2, ga1, ga2 = call.finish()
    np.testing.assert_array_equal(gl2.view(np.uint64), l2.view(np.uint64))
    LD = eb.LD
    with np.errstate(all='ignore'):
        y1 = np.exp(-((logp2.astype(LD) - logg2.astype(LD)) - lstar.astype(LD)[:, None]))
        y2 = np.exp(l1.astype(LD) - lstar.astype(LD)[:, None])
    for got, plain, yard, what in ((ga1, d1, y1, 'a1'), (ga2, d2, y2, 'a2')):
        for test in (np.isnan, np.isposinf):
            np.testing.assert_array_equal(test(got), test(plain), err_msg=what)
        np.testing.assert_array_equal(got == 0, plain == 0, err_msg=what)
        ok = np.isfinite(plain) & (plain > 1e-290) & (plain < 1e290)
        own = (np.abs(plain[ok] - yard[ok]) / yard[ok]).max()
        err = (np.abs(got[ok] - yard[ok]) / yard[ok]).max()
        print(f'{what}: device {float(err):.2e}, the definition {float(own):.2e} (relative)')
        assert ok.sum() > 500 and err <= eb.FACTOR * own, what
    assert np.isposinf(ga1[1, 0]) and np.isnan(ga1[1, 1]) and ga1[1, 2] == 0.0 and np.isposinf(ga1[2, 5]) and ga1[2, 6] == 0.0
    assert np.isposinf(ga2[0, 0]) and ga2[0, 1] == 0.0 and np.isnan(ga2[0, 2]) and np.isposinf(ga2[0, 3])
    # l2 may be left out or be one of its inputs
    call = GuardedCall()
    pa1, pa2 = call.out('a1', (E, N2)), call.out('a2', (E, N1))
    _hip.bridge_scale_dev(t[0].data_ptr(), N1, t[1].data_ptr(), t[2].data_ptr(), N2, E, t[3].data_ptr(), t[2].data_ptr(), pa1,
                          pa2, call.stream)
    ha1, ha2 = call.finish()
    np.testing.assert_array_equal(ha1.view(np.uint64), ga1.view(np.uint64))
    np.testing.assert_array_equal(ha2.view(np.uint64), ga2.view(np.uint64))
    np.testing.assert_array_equal(t[2].cpu().numpy().view(np.uint64), l2.view(np.uint64))


# -- bisip_bridge_draw_dev ------------------------------------------------------------------------------------------------------
def run_draw(mu, L, c, n_draws, seed, first_draw=0, first_ensemble=0):
    from bisip_amd import _hip
    E, ndim = mu.shape
    call = GuardedCall()
    pt, pg = call.out('theta', (E, n_draws, ndim)), call.out('log_g', (E, n_draws))
    d = [dev(a) for a in (mu, L, c)]
    _hip.bridge_draw_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), E, ndim, n_draws, seed, first_draw, first_ensemble,
                         pt, pg, call.stream)
    return call.finish()


@pytest.mark.parametrize('E', (1, 3))
@pytest.mark.parametrize('n_draws', (1, 255, 1000))
@pytest.mark.parametrize('ndim', (1, 2, 7, 16))
def test_draws_against_the_yardstick(ndim, n_draws, E):
    """theta_j and log_g of every draw against the same Philox words carried through long double; per coordinate the error is
    scaled by sum_k |L_jk z_k|, log_g's by 0.5 m + |c|; the device is allowed FACTOR times the worst scaled error of the
    float64 NumPy definition (evidence.host_draws) over the same draws.  first_draw = 2^32 - 3: the counter's high word turns
    within the call."""
    from bisip_amd import evidence as ev
    mu, L, c = proposal(E, ndim, 3)
    seed, first = 0x123456789abcdef, 2 ** 32 - 3
    theta, lg = run_draw(mu, L, c, n_draws, seed, first, 5)
    assert np.isfinite(theta).all() and np.isfinite(lg).all()
    own_t = own_g = err_t = err_g = 0.0
    family = max(n_draws, 1000)                # the definition's own error over draws first ... first + 999 of the stream
    for e in range(E):
        yt, yg, z = ev.draw_yardstick(mu[e], L[e], c[e], family, seed, first, 5 + e)
        ht, hg = ev.host_draws(mu[e], L[e], c[e], family, seed, first, 5 + e)
        scale_t = np.abs(z) @ np.abs(np.tril(L[e])).T.astype(eb.LD)
        scale_g = (z * z).sum(axis=1) / 2 + abs(c[e])
        own_t = max(own_t, float((np.abs(ht - yt) / scale_t).max()))
        own_g = max(own_g, float((np.abs(hg - yg) / scale_g).max()))
        k = n_draws
        err_t = max(err_t, float((np.abs(theta[e] - yt[:k]) / scale_t[:k]).max()))
        err_g = max(err_g, float((np.abs(lg[e] - yg[:k]) / scale_g[:k]).max()))
    print(f'ndim {ndim}, {n_draws} draws, E {E}: theta {err_t:.2e} (definition {own_t:.2e}), log_g {err_g:.2e} ({own_g:.2e})')
    assert own_t > 0 and own_g > 0
    assert err_t <= eb.FACTOR * own_t and err_g <= eb.FACTOR * own_g


def test_draws_do_not_depend_on_the_call_and_do_on_the_seed():
    mu, L, c = proposal(3, 7, 4)
    whole = run_draw(mu, L, c, 1000, 77)
    a, b = run_draw(mu, L, c, 400, 77), run_draw(mu, L, c, 600, 77, first_draw=400)
    for w, p, q in zip(whole, a, b):
        np.testing.assert_array_equal(w.view(np.uint64), np.concatenate([p, q], axis=1).view(np.uint64))
    other = run_draw(mu, L, c, 1000, 78)
    assert (other[0] != whole[0]).all() and (whole[0][0] != whole[0][1]).all()
    lone = run_draw(mu[2:], L[2:], c[2:], 1000, 77, first_ensemble=2)     # the stream is the ensemble's, not the call's
    np.testing.assert_array_equal(lone[0][0].view(np.uint64), whole[0][2].view(np.uint64))
    z = np.linalg.solve(np.tril(L[0]), (whole[0][0] - mu[0]).T).T
    assert np.abs(z.mean(axis=0)).max() < 5 / np.sqrt(1000) and np.abs(z.var(axis=0) - 1).max() < 5 * np.sqrt(2 / 1000)


# -- end to end -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(kind):
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389175']
    if kind == 'ColeCole':
        m = bisip_amd.PeltonColeCole(path, n_modes=1, nwalkers=32, nsteps=STEPS[kind])
        p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(3).randn(32, 4)
        np.random.seed(8)
        m.fit(p0=p0, chain='device')
        return m
    import fitted as shared
    return shared.fitted_model('device', nsteps=STEPS[kind])


def numpy_side(res, kept, chain, logp, log_prob_fn, bounds):
    """bridge_evidence on host copies with the device's proposal, draws and effective size."""
    from bisip_amd import evidence as ev
    return ev.bridge_evidence(chain, logp, log_prob_fn, bounds, neff=res['neff'], use_all=False,
                              proposal=(res['proposal_mean'], res['proposal_cov']), draws=(kept['theta2'], kept['logg2']))


def check_against_numpy(dev_res, kept, chain, logp, log_prob_fn, bounds, what):
    """log_ml within evidence_bounds.log_ml_bound of the NumPy definition, iterations within 1."""
    from bisip_amd import evidence as ev
    host = numpy_side(dev_res, kept, chain, logp, log_prob_fn, bounds)
    n, Wp, ndim = chain.shape
    n0, n1 = ev.halves(n, Wp, ndim)
    mu, L, c = ev.proposal_factor(dev_res['proposal_mean'], dev_res['proposal_cov'])
    mu, L, c = mu[0], L[0], float(c[0])
    rows, lp1 = chain[n0:].reshape(n1 * Wp, ndim), logp[n0:].reshape(n1 * Wp)
    l1 = lp1 - ev.log_g(rows, mu, L, c)
    lp2 = np.asarray(log_prob_fn(kept['theta2']), dtype=np.float64)
    np.testing.assert_array_equal(np.isneginf(lp2), np.isneginf(kept['logp2']), err_msg=what)
    fin = np.isfinite(lp2)
    assert np.isfinite(kept['logp2'][fin]).all() and fin.any()
    dlogp2 = np.abs(lp2[fin] - kept['logp2'][fin]).max()
    assert dlogp2 <= 1e-10 * np.maximum(1.0, np.abs(lp2[fin])).max()          # the project's parity tolerance
    with np.errstate(all='ignore'):
        l2 = lp2 - kept['logg2']
    lstar, a1, a2 = ev.bridge_terms(l1, l2)
    it = ev.bridge_iterate(a1, a2, host['neff'] / (host['neff'] + l2.size))
    bound = eb.log_ml_bound(L, c, eb.whiten(rows, mu, L).astype(np.float64), lp1, l1, l2, float(lstar), float(dlogp2),
                            host['log_ml'], it['log_r'], it['history'], ev.TOL)
    err = abs(dev_res['log_ml'] - host['log_ml'])
    print(f'{what}: log_ml {dev_res["log_ml"]:.6f} +- {dev_res["se"]:.1e}, device - NumPy {err:.2e}, bound {bound:.2e}, '
          f'{dev_res["iterations"]} iterations, {dev_res["frac_outside"]:.3f} outside, logp2 differs by {dlogp2:.1e}')
    assert err <= bound, what
    assert abs(int(dev_res['iterations']) - host['iterations']) <= 1
    assert np.isfinite(dev_res['se']) and 0 <= dev_res['frac_outside'] < 1 and dev_res['n1'] == n1 * Wp == dev_res['n2']
    return host


@pytest.mark.parametrize('kind', ('ColeCole', 'PolynomialDecomposition'))
def test_get_evidence_of_a_model(kind, monkeypatch):
    from bisip_amd import evidence as ev
    m = fitted(kind)
    s = m._sampler
    assert s.chain_on_device
    KW = dict(discard=STEPS[kind] // 2, thin=1)
    res = m.get_evidence(seed=5, **KW)
    assert list(res) == ['log_evidence', 'log_ml', 'se', 'iterations', 'n1', 'n2', 'neff', 'tau_f2', 'frac_outside',
                         'gaussian_offset', 'proposal_mean', 'proposal_cov']
    ndim = s.ndim
    assert res['proposal_mean'].shape == (ndim,) and res['proposal_cov'].shape == (ndim, ndim)
    assert all(isinstance(res[k], float) for k in ('log_evidence', 'log_ml', 'se', 'neff', 'tau_f2', 'frac_outside'))
    lo, hi = m.param_bounds
    assert res['log_evidence'] == res['log_ml'] - float(np.log(hi - lo).sum())
    assert res['gaussian_offset'] == float(ev.gaussian_offset(m._data['zn_err'])) and 0 < res['neff'] <= res['n1']
    raw = ev.device_evidence(s.used_samples_dev(**KW), s.log_prob_samples_dev(**KW), s.backend.ctx, seed=5, keep_draws=True)
    assert raw['log_ml'][0] == res['log_ml'] and raw['iterations'][0] == res['iterations']
    one = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
    chain, logp = m.get_chain(**KW), s.get_log_prob(**KW)
    check_against_numpy(one, {k: raw[k][0] for k in ('theta2', 'logg2', 'logp2')}, chain, logp, m.log_prob, m.param_bounds, kind)
    # the draws in passes of 700 (the last one shorter): the same draws, the same bits
    monkeypatch.setattr(ev, 'PASS_BYTES', 8 * ndim * 700)
    passes = m.get_evidence(seed=5, **KW)
    monkeypatch.undo()
    assert res['n2'] > 1400 and res['n2'] % 700
    assert passes['log_ml'] == res['log_ml'] and passes['se'] == res['se'] and passes['frac_outside'] == res['frac_outside']
    # fewer draws, another seed, no effective size; a given proposal: all used samples enter the estimator
    other = m.get_evidence(seed=6, n_draws=1500, neff=None, **KW)
    assert other['n2'] == 1500 and other['neff'] == other['n1'] and other['log_ml'] != res['log_ml']
    fixed = m.get_evidence(seed=5, proposal=(res['proposal_mean'], res['proposal_cov']), **KW)
    assert fixed['n1'] == 2 * res['n1'] == fixed['n2']
    np.testing.assert_array_equal(fixed['proposal_cov'], res['proposal_cov'])
    print(f'{kind}: {res["log_ml"]:.4f} +- {res["se"]:.1e}; 1500 draws {other["log_ml"]:.4f} +- {other["se"]:.1e}; '
          f'given proposal {fixed["log_ml"]:.4f} +- {fixed["se"]:.1e}')
    rows = ev.compare_evidence({'a': res, 'b': other})
    assert {r['name'] for r in rows} == {'a', 'b'} and rows[0]['log_bf'] == 0.0 and abs(rows[0]['prob'] + rows[1]['prob'] - 1) < 1e-15
    with pytest.raises(ValueError, match='too few'):
        m.get_evidence(discard=STEPS[kind] - 2)
    # an explicit chain takes the NumPy path with the model's own log_prob
    host = m.get_evidence(chain=chain, log_prob=logp, seed=5)
    assert host['n1'] == res['n1'] == host['n2'] and host['iterations'] >= 1
    np.testing.assert_allclose(host['proposal_cov'], res['proposal_cov'], rtol=1e-9, atol=0)


def test_get_evidence_of_a_batch():
    import bisip_amd
    from bisip_amd import evidence as ev
    from bisip_amd.chainview import ChainView
    files = bisip_amd.DataFiles()
    E, Wp = 3, 16
    names = sorted(files)[:E]
    b = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in names], nwalkers=Wp, nsteps=STEPS['batch'], n_modes=1)
    p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(1).randn(E, Wp, 4)
    b.fit(p0, seed=6, chain='device')
    KW = dict(discard=STEPS['batch'] // 2, thin=1)
    res = b.get_evidence(seed=9, **KW)
    assert all(res[k].shape == (E,) for k in ('log_evidence', 'log_ml', 'se', 'iterations', 'neff', 'tau_f2', 'frac_outside',
                                              'gaussian_offset'))
    assert res['proposal_mean'].shape == (E, 4) and res['proposal_cov'].shape == (E, 4, 4)
    assert np.isfinite(res['se']).all() and ((res['frac_outside'] >= 0) & (res['frac_outside'] < 1)).all()
    lo, hi = b.param_bounds
    np.testing.assert_array_equal(res['log_evidence'], res['log_ml'] - float(np.log(hi - lo).sum()))
    s = b._fitted()
    view, lview = s.used_samples_dev(**KW), s.log_prob_samples_dev(**KW)
    raw = s.evidence(seed=9, keep_draws=True, **KW)
    np.testing.assert_array_equal(raw['log_ml'], res['log_ml'])
    chain, logp = b.get_chain(**KW), b.get_log_prob(**KW)              # (n, E, Wp, ndim), (n, E, Wp)
    for e in range(E):
        one = {k: (v[e] if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
        lone = bisip_amd.PeltonColeCole(files[names[e]], n_modes=1, nwalkers=Wp, nsteps=5)
        c_e, l_e = np.ascontiguousarray(chain[:, e]), np.ascontiguousarray(logp[:, e])
        check_against_numpy(one, {k: raw[k][e] for k in ('theta2', 'logg2', 'logp2')}, c_e, l_e, lone.log_prob, b.param_bounds,
                            f'spectrum {e}')
        # entry e is the single-model result on spectrum e: its own context, the same seed and the stream of ensemble e
        sub = ChainView(view.tensor, view.n, 1, Wp, b.ndim, view.offset + e * Wp * b.ndim, view.stride, view.backend)
        lsub = ChainView(lview.tensor, lview.n, 1, Wp, 1, lview.offset + e * Wp, lview.stride, lview.backend)
        single = ev.device_evidence(sub, lsub, lone._context(), seed=9, first_ensemble=e, keep_draws=True)
        np.testing.assert_array_equal(single['theta2'][0].view(np.uint64), raw['theta2'][e].view(np.uint64))
        np.testing.assert_array_equal(single['proposal_cov'][0], raw['proposal_cov'][e])
        with np.errstate(invalid='ignore'):                          # (-inf beside -inf: not a difference)
            dl = np.abs(single['logp2'][0] - raw['logp2'][e])
        dl = dl[np.isfinite(dl)].max()
        bound = dl + 2 * eb.iterate_bound(one['n1'], one['n2'], [], ev.TOL) + 8 * eb.U * abs(one['log_ml'])
        assert abs(single['log_ml'][0] - one['log_ml']) <= bound, (e, single['log_ml'][0], one['log_ml'], bound)
        assert abs(int(single['iterations'][0]) - int(one['iterations'])) <= 1
    with pytest.raises(ValueError, match='too few'):
        b.get_evidence(discard=STEPS['batch'] - 1)
    b.close()
