"""The MAP fit on the device, from the C entry points up to fit(p0='map').  bisip_gauss_newton_dev is held bit for bit to
bisip_amd.mapfit.ordered_normal_equations fed by the library's own forward at the stencil points (a single-spectrum context of
each spectrum, through the entry point that existed before); every call goes through chain_harness.GuardedCall, so the outputs
carry guards and an output that is not asked for stays untouched.  bisip_map_fit_dev is held to properties that do not depend
on the path a start takes, to mapfit.lm_fit over the same forward, and to itself: twice, alone, in a batch.

Measured on an MI355X over the five bundled cases (32 starts, at most 60 iterations, pred_tol = 0): the best chi2 equals
lm_fit's to the bit in all five; pred at the best result, recomputed on the host, 6.9e-20 ... 2.0e-15 (bound 1e-10); logp against
logprob at most 8.0e-15 relative (bound 1e-10); 32, 30, 32, 27 and 25 of 32 starts within 1e-6 of the best chi2."""
import numpy as np
import pytest

import map_bounds as mb
from chain_harness import GuardedCall, assert_same_bits
from test_gpu_fit_quality import batch_of
from test_gpu_response import single_context

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# -- bisip_gauss_newton_dev ---------------------------------------------------------------------------------------------------
def run_gauss_newton(ctx, theta, first, asked=(True, True, True)):
    """theta (E, S, ndim) -> chi2 (E, S), g (E, S, ndim), A (E, S, ndim, ndim) of spectra first ... first + E - 1."""
    import torch
    E, S, n = theta.shape
    t = torch.from_numpy(np.ascontiguousarray(theta)).cuda()
    call = GuardedCall()
    ptrs = [call.out('chi2', (E, S), asked=asked[0]), call.out('g', (E, S, n), asked=asked[1]),
            call.out('A', (E, S, n, n), asked=asked[2])]
    ctx.gauss_newton_dev(first, E, t.data_ptr(), S, *ptrs, call.stream)
    return call.finish()


def reference(b, theta, first):
    """The same from ordered_normal_equations over forward at the stencil points; a point that is not finite counts as NaN."""
    from bisip_amd import mapfit as mf
    E, S, n = theta.shape
    h, _, _ = mf.inner_box(b.param_bounds)
    out = []
    for e in range(E):
        ctx = single_context(b, first + e)
        bad = ~np.isfinite(theta[e]).all(axis=-1)
        finite = np.where(bad[:, None], theta[e][~bad][0], theta[e])
        Z = ctx.forward(mf.stencil(finite, h).reshape(-1, n)).reshape(S, 2 * n + 1, 2, -1)
        ctx.close()
        Z[bad] = np.nan
        out.append(mf.ordered_normal_equations(Z, b.zn[first + e], mb.inverse_variance(b.zn_err[first + e]), h))
    return [np.stack([o[k] for o in out]) for k in range(3)]


MODELS = (('PolynomialDecomposition', dict(poly_deg=0)), ('PolynomialDecomposition', dict(poly_deg=10)),
          ('PeltonColeCole', dict(n_modes=1)), ('PeltonColeCole', dict(n_modes=5)), ('Dias2000', {}), ('Shin2015', {}))
# (N, E, S): every N of 1, 20 and 33, E of 1 and 3 and S of 1 and 5; the context holds one spectrum more, the call starts at 1
SHAPES = ((1, 1, 1), (20, 3, 5), (33, 1, 5), (33, 3, 1))


@pytest.mark.parametrize('model,kw', MODELS, ids=lambda v: v if isinstance(v, str) else '-'.join(f'{k}{x}' for k, x in v.items()))
def test_gauss_newton_entry_point(model, kw):
    from bisip_amd import mapfit as mf
    for n_freq, E, S in SHAPES:
        b = batch_of(model, kw, n_freq, E + 1)
        assert b.n_spectra == E + 1 and b.N == n_freq
        lo, hi = b.param_bounds
        _, lo_in, hi_in = mf.inner_box(b.param_bounds)
        n = lo.size
        assert 2 * n + 1 <= 64 and (kw.get('n_modes') != 5 or 2 * n + 1 == 33)
        theta = lo + np.random.default_rng([n_freq, E, S]).uniform(0.2, 0.8, (E, S, n)) * (hi - lo)
        if S == 5:
            theta[-1, 1] = lo_in                      # a point on the inner bound: its stencil reaches the prior bound
            theta[0, 3] = hi_in
            theta[-1, 2, n // 2] = np.nan             # a point with a NaN: NaN outputs, its neighbours alone
        what = f'{model} {kw} N={n_freq} E={E} S={S}'
        got = run_gauss_newton(b.ctx, theta, 1)
        want = reference(b, theta, 1)
        for a, w, name in zip(got, want, ('chi2', 'g', 'A')):
            assert_same_bits(a, w, f'{what}: {name}')
        if S == 5:
            assert np.isnan(got[0][-1, 2]) and np.isnan(got[1][-1, 2]).all() and np.isnan(got[2][-1, 2]).all()
        for asked in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
            some = run_gauss_newton(b.ctx, theta, 1, asked)            # (finish() holds the others to their fill)
            for a, g, want_it in zip(some, got, asked):
                if want_it:
                    np.testing.assert_array_equal(bits(a), bits(g), err_msg=f'{what} {asked}')
        b.close()


def test_gauss_newton_refusals():
    b = batch_of('PeltonColeCole', dict(n_modes=1), 20, 2)
    ctx = b.ctx
    for match, kw in (('null', dict(theta=0)), ('spectra', dict(first=2)), ('spectra', dict(count=0)), ('points', dict(S=0)),
                      ('points', dict(S=1 << 31)), ('aligned', dict(chi2=4100))):
        a = dict(dict(first=0, count=1, theta=4096, S=1, chi2=4096), **kw)
        with pytest.raises(ValueError, match=match):
            ctx.gauss_newton_dev(a['first'], a['count'], a['theta'], a['S'], a['chi2'], 0, 0, 0)
        with pytest.raises(ValueError, match=match):
            ctx.map_fit_dev(a['first'], a['count'], a['theta'], a['S'], 60, 1e-8, 0, a['chi2'], 0, 0, 0, 0, 0, 0)
    for bad in (-1, 1001):
        with pytest.raises(ValueError, match='max_iter'):
            ctx.map_fit_dev(0, 1, 4096, 1, bad, 1e-8, 0, 4096, 0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match='pred_tol'):
        ctx.map_fit_dev(0, 1, 4096, 1, 60, float('nan'), 0, 4096, 0, 0, 0, 0, 0, 0)
    wide = b.param_bounds.copy()
    wide[1, 0] = np.inf
    ctx.set_bounds(wide)
    with pytest.raises(ValueError, match='not finite'):
        ctx.gauss_newton_dev(0, 1, 4096, 1, 4096, 0, 0, 0)
    with pytest.raises(ValueError, match='not finite'):
        ctx.map_fit_dev(0, 1, 4096, 1, 60, 1e-8, 0, 4096, 0, 0, 0, 0, 0, 0)
    b.close()


# -- bisip_map_fit_dev --------------------------------------------------------------------------------------------------------
def run_map_fit(ctx, starts, max_iter=60, pred_tol=0.0, first=0):
    """starts (E, S, ndim) through GuardedCall: dict of theta, chi2, logp, pred, hessian, iterations, status."""
    import torch
    E, S, n = starts.shape
    t = torch.from_numpy(np.ascontiguousarray(starts)).cuda()
    call = GuardedCall()
    names = ('theta', 'chi2', 'logp', 'pred', 'hessian', 'iterations', 'status')
    shapes = ((E, S, n), (E, S), (E, S), (E, S), (E, S, n, n), (E, S), (E, S))
    ptrs = [call.out(k, s, dtype=torch.int64 if k in ('iterations', 'status') else None) for k, s in zip(names, shapes)]
    ctx.map_fit_dev(first, E, t.data_ptr(), S, max_iter, pred_tol, *ptrs, call.stream)
    return dict(zip(names, call.finish()))


def same_result(a, b, what):
    for k in a:
        if a[k].dtype == np.int64:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f'{what}: {k}')
        else:
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=f'{what}: {k}')


@pytest.mark.parametrize('case_id', mb.CASE_IDS)
def test_map_fit_on_the_bundled_cases(case_id):
    from bisip_amd import mapfit as mf
    m = mb.model_of(mb.CASES[mb.CASE_IDS.index(case_id)])
    bounds = m.param_bounds
    ctx = m._context()
    ctx.set_bounds(bounds)
    y, iv = m.data['zn'], mb.inverse_variance(m.data['zn_err'])
    h, lo_in, hi_in = mf.inner_box(bounds)
    starts = mb.starts_of(m)
    n = starts.shape[1]
    r = {k: v[0] for k, v in run_map_fit(ctx, starts[None]).items()}
    # properties that do not depend on the path
    assert ((r['theta'] >= lo_in) & (r['theta'] <= hi_in)).all()
    assert ((r['iterations'] >= 0) & (r['iterations'] <= 60)).all() and set(r['status']) <= {0, 1, 2}
    start_chi2 = mf.ordered_chi2(ctx.forward(mf.clip(starts, lo_in, hi_in)), y, iv)
    assert (r['chi2'] <= start_chi2).all()
    np.testing.assert_array_equal(bits(r['chi2']), bits(mf.ordered_chi2(ctx.forward(r['theta']), y, iv)))    # chi2 is that of theta
    best = int(np.argmin(r['chi2']))
    Z = ctx.forward(mf.stencil(r['theta'][best], h)).reshape(2 * n + 1, 2, -1)
    c, g, A = mf.ordered_normal_equations(Z, y, iv, h)
    pred = mf.lm_pred(A, g, mf.fixed_mask(r['theta'][best], g, A, lo_in, hi_in))
    ref = mf.lm_fit(ctx.forward, y, iv, bounds, starts, max_iter=60, pred_tol=0.0)
    lp = ctx.logprob(r['theta'])
    rel = np.abs(r['logp'] - lp) / np.maximum(1.0, np.abs(lp))
    print(f'{case_id}: best chi2 {r["chi2"][best]:.12g} (lm_fit {ref["chi2"].min():.12g}, difference {r["chi2"][best] - ref["chi2"].min():.2e}), '
          f'pred at the best {pred:.2e} (the kernel\'s {r["pred"][best]:.2e}), logp against logprob {rel.max():.2e}, '
          f'{int(np.sum(r["chi2"] <= r["chi2"][best] + 1e-6))} of 32 agree, median iterations {np.median(r["iterations"])}, '
          f'status counts {np.bincount(r["status"], minlength=3)}')
    assert pred <= 1e-10
    assert bits(c) == bits(r['chi2'][best])
    np.testing.assert_array_equal(bits(A), bits(r['hessian'][best]))
    assert r['chi2'][best] <= ref['chi2'].min() + 1e-9
    assert (rel <= 1e-10).all()
    # the same bits twice, and a start alone
    same_result({k: v[0] for k, v in run_map_fit(ctx, starts[None]).items()}, r, 'twice')
    for s in (0, 13, 31):
        alone = run_map_fit(ctx, starts[None, s:s + 1])
        same_result({k: v[0, 0] for k, v in alone.items()}, {k: v[s] for k, v in r.items()}, f'start {s} alone')
    # the host wrapper and its defaults
    w = mf.device_map_fit(ctx, starts, max_iter=60, pred_tol=0.0)
    same_result({k: w[k] for k in r}, r, 'device_map_fit')
    np.testing.assert_array_equal(bits(w['g'][best]), bits(g))             # the gradient at the results comes with it
    capped = mf.device_map_fit(ctx, starts[:4], max_iter=2, pred_tol=0.0)
    assert (capped['iterations'] <= 2).all() and (capped['status'][capped['iterations'] == 2] == 2).all()


@pytest.mark.parametrize('model,kw', (('PeltonColeCole', dict(n_modes=1)), ('PolynomialDecomposition', dict(poly_deg=5))))
def test_a_batch_is_its_spectra(model, kw):
    import bisip_amd
    files = bisip_amd.DataFiles()
    b = bisip_amd.SpectraBatch(model, [files[k] for k in sorted(files)[:3]], nwalkers=8, nsteps=8, **kw)
    starts = np.random.RandomState(5).uniform(*b.param_bounds, (3, 8, b.ndim))
    whole = run_map_fit(b.ctx, starts)
    for e in range(3):
        ctx = single_context(b, e)
        one = run_map_fit(ctx, starts[e:e + 1])
        same_result({k: v[0] for k, v in one.items()}, {k: v[e] for k, v in whole.items()}, f'spectrum {e}')
        lp = ctx.logprob(whole['theta'][e])
        assert (np.abs(whole['logp'][e] - lp) <= 1e-10 * np.maximum(1.0, np.abs(lp))).all()
        ctx.close()
    part = run_map_fit(b.ctx, starts[1:], first=1)                       # first_spectrum > 0
    same_result(part, {k: v[1:] for k, v in whole.items()}, 'spectra 1-2')
    b.close()


@pytest.mark.parametrize('model,kw', (('PeltonColeCole', dict(n_modes=5)), ('PeltonColeCole', dict(n_modes=3)),
                                      ('PolynomialDecomposition', dict(poly_deg=10))), ids=('cc5', 'cc3', 'pd10'))
def test_map_fit_of_the_largest_instantiations(model, kw):
    """ndim 16 (33 stencil lanes, bit 15 of the mask, 32.7 KB of LDS), ndim 10 and degree 10 (ndim 12): the run is finite,
    chi2 does not increase, chi2 and the Hessian are those of theta, and a second run gives the same bits."""
    from bisip_amd import mapfit as mf
    b = batch_of(model, kw, 20, 2)
    bounds = b.param_bounds
    h, lo_in, hi_in = mf.inner_box(bounds)
    n = b.ndim
    starts = np.random.RandomState(11).uniform(*bounds, (2, 6, n))
    r = run_map_fit(b.ctx, starts, max_iter=25)
    for k in ('theta', 'chi2', 'logp', 'hessian'):
        assert np.isfinite(r[k]).all(), k
    assert not np.isnan(r['pred']).any() and ((r['theta'] >= lo_in) & (r['theta'] <= hi_in)).all()
    assert (r['iterations'] <= 25).all() and (r['iterations'] > 0).any() and set(r['status'].ravel()) <= {0, 1, 2}
    for e in range(2):
        ctx = single_context(b, e)
        y, iv = b.zn[e], mb.inverse_variance(b.zn_err[e])
        assert (r['chi2'][e] <= mf.ordered_chi2(ctx.forward(mf.clip(starts[e], lo_in, hi_in)), y, iv)).all()
        Z = ctx.forward(mf.stencil(r['theta'][e], h).reshape(-1, n)).reshape(6, 2 * n + 1, 2, -1)
        c, g, A = mf.ordered_normal_equations(Z, y, iv, h)
        np.testing.assert_array_equal(bits(c), bits(r['chi2'][e]))
        np.testing.assert_array_equal(bits(A), bits(r['hessian'][e]))
        ctx.close()
    same_result(run_map_fit(b.ctx, starts, max_iter=25), r, 'twice')
    b.close()


def test_one_frequency_ends_without_nan():
    """N = 1: two data for four parameters, A is rank-deficient at every point."""
    b = batch_of('PeltonColeCole', dict(n_modes=1), 1, 1)
    starts = np.random.RandomState(2).uniform(*b.param_bounds, (1, 8, b.ndim))
    r = run_map_fit(b.ctx, starts)
    for k in ('theta', 'chi2', 'logp', 'pred', 'hessian'):
        assert not np.isnan(r[k]).any(), k
    assert np.isfinite(r['chi2']).all() and (r['iterations'] <= 60).all() and set(r['status'].ravel()) <= {0, 1, 2}
    b.close()


# -- the public interface -------------------------------------------------------------------------------------------------------
KEYS = {'theta', 'logp', 'chi2', 'pred', 'status', 'at_bound', 'hessian', 'cov', 'log_evidence_laplace', 'all_theta', 'all_logp',
        'all_chi2', 'all_status', 'iterations', 'n_agree'}


def test_fit_map_of_a_model():
    m = mb.model_of(mb.CASES[2])
    np.random.seed(5)
    state = np.random.get_state()
    out = m.fit_map(seed=7)
    after = np.random.get_state()
    assert state[0] == after[0] and (state[1] == after[1]).all() and state[2:] == after[2:]       # the global state is untouched
    assert set(out) == KEYS and m.get_map() is out
    j = m.param_names.index('log_tau1')
    assert out['at_bound'][j] and out['at_bound'].sum() == 1 and np.isnan(out['log_evidence_laplace'])
    assert out['theta'].shape == (4,) and out['all_theta'].shape == (32, 4) and out['hessian'].shape == out['cov'].shape == (4, 4)
    assert out['n_agree'] >= 20 and out['status'] in ('converged', 'stalled', 'cap') and out['iterations'].dtype == np.int64
    assert out['logp'] == out['all_logp'].max() and out['chi2'] == out['all_chi2'].min()
    again = m.fit_map(seed=7)
    np.testing.assert_array_equal(bits(again['all_theta']), bits(out['all_theta']))
    given = m.fit_map(starts=mb.starts_of(m), pred_tol=0.0)
    assert given['chi2'] <= out['chi2'] + 1e-7 and given['all_theta'].shape == (32, 4)
    with pytest.raises(ValueError, match='starts must have shape'):
        m.fit_map(starts=np.zeros((3, 5)))


def test_at_bound_is_the_fixed_set():
    """Shin2015 on SIP-K389175: R1 goes to its lower bound, where the misfit all but stops depending on log_Q1 and n1 (A_jj of
    1e-19 or exactly 0), which end on bounds of their own, and log_Q2 sits on its upper bound -- at_bound is the fit's fixed set
    at the result, recomputed here from forward, and the covariance of the other two is the inverse of their block."""
    from bisip_amd import mapfit as mf
    m = mb.model_of(mb.CASES[4])
    out = m.fit_map(starts=mb.starts_of(m), pred_tol=0.0)
    names = m.param_names
    assert [names[j] for j in np.flatnonzero(out['at_bound'])] == ['R1', 'log_Q1', 'log_Q2', 'n1']
    h, lo_in, hi_in = mf.inner_box(m.param_bounds)
    Z = m._context().forward(mf.stencil(out['theta'], h)).reshape(13, 2, -1)
    _, g, A = mf.ordered_normal_equations(Z, m.data['zn'], mb.inverse_variance(m.data['zn_err']), h)
    np.testing.assert_array_equal(out['at_bound'], mf.fixed_mask(out['theta'], g, A, lo_in, hi_in))
    np.testing.assert_array_equal(bits(A), bits(out['hessian']))
    assert np.isnan(out['log_evidence_laplace'])
    free = ~out['at_bound']
    assert np.isnan(out['cov'][~free]).all() and np.isnan(out['cov'][:, ~free]).all()
    np.testing.assert_allclose(out['cov'][np.ix_(free, free)] @ out['hessian'][np.ix_(free, free)], np.eye(2), atol=1e-9)
    p0 = mf.ball(out['theta'], out['cov'], out['at_bound'], m.param_bounds, 32, np.random.RandomState(1))
    assert ((p0 > m.param_bounds[0]) & (p0 < m.param_bounds[1])).all()
    assert p0[:, free].std(axis=0) == pytest.approx(np.sqrt(np.diag(out['cov'])[free]), rel=0.5)


def test_spectra_batch_fit_map_is_the_models():
    import bisip_amd
    files = bisip_amd.DataFiles()
    keys = sorted(files)[:3]
    b = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in keys], nwalkers=8, nsteps=8, n_modes=1)
    starts = np.random.RandomState(9).uniform(*b.param_bounds, (3, 16, b.ndim))
    got = b.fit_map(starts=starts)
    assert set(got) == KEYS and b.get_map() is got and got['theta'].shape == (3, 4) and got['all_theta'].shape == (3, 16, 4)
    for e, k in enumerate(keys):
        m = bisip_amd.PeltonColeCole(files[k], n_modes=1, nwalkers=8, nsteps=8)
        one = m.fit_map(starts=starts[e])
        for name in KEYS:
            a, w = np.asarray(got[name][e]), np.asarray(one[name])
            if a.dtype == np.float64:
                np.testing.assert_array_equal(np.isnan(a), np.isnan(w), err_msg=name)
                np.testing.assert_array_equal(bits(a[~np.isnan(a)]), bits(w[~np.isnan(w)]), err_msg=name)
            else:
                np.testing.assert_array_equal(a, w, err_msg=name)
    auto = b.fit_map(n_starts=4, seed=1)
    assert auto['all_theta'].shape == (3, 4, 4)
    b.close()


def test_fit_from_the_map():
    """PolynomialDecomposition, 32 walkers x 200 steps on SIP-K389175: started in the Laplace ball the ensemble's median
    log-probability is within 3 ndim of the optimum's at the first stored step (the expected deficit of draws from the Laplace
    normal is ndim / 2); started uniformly in the box it is not."""
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389175']
    first = {}
    for p0 in ('map', None):
        m = bisip_amd.PolynomialDecomposition(path, nwalkers=32, nsteps=200)
        np.random.seed(3)
        m.fit(p0=p0, chain='device')
        first[p0] = float(np.median(m._sampler.get_log_prob()[0]))
        if p0 == 'map':
            best = m.get_map()
    ndim = best['theta'].size
    print(f'logp of the optimum {best["logp"]:.3f}; median logp of the first stored step: from the map {first["map"]:.3f}, uniform '
          f'{first[None]:.3f}')
    assert first['map'] >= best['logp'] - 3 * ndim
    assert not first[None] >= best['logp'] - 3 * ndim
    assert np.isfinite(best['log_evidence_laplace']) and not best['at_bound'].any()


RHAT_SCREEN = 1.05          # the split R-hat above which examples/batch_of_spectra.py counts a spectrum as one to look at


def test_the_chain_from_the_map_passes_the_rhat_screening():
    """The same fit held to the project's screening, max split R-hat < 1.05 over the whole chain with nothing discarded, on a
    chain long enough for that number to mean something.  Split R-hat^2 is (L - 1) / L + Bn / Wn over halves of L steps, and for
    a stationary ensemble Bn / Wn, the variance of a half's mean over that of a draw, is tau / L with tau the integrated
    autocorrelation time: 1.05 needs L > 10 tau whatever the start.  tau of this fit is 53-75 steps (get_autocorr_time on 2000
    steps), so halves of 100 steps read 1.42-1.46 from the map (and 1.09-1.27 from the uniform start, whose transient inflates Wn):
    no 200-step chain of this model can pass, and 2000 steps read 1.046-1.055, at the threshold.  8000 steps (halves of 53 tau
    or more) should read sqrt(1 + 75 / 4000) = 1.01: a margin of four in R-hat - 1, a tenth of a second of sampling.  Measured on an
    MI355X: 1.0071-1.0096, the rank-normalised R-hat the same."""
    import bisip_amd
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], nwalkers=32, nsteps=8000)
    np.random.seed(3)
    m.fit(p0='map', chain='device')
    rhat, rank = m.get_rhat(discard=0), m.get_rank_rhat(discard=0)
    print(f'split R-hat over 8000 steps from the map, nothing discarded: {rhat.min():.4f} ... {rhat.max():.4f}; rank-normalised '
          f'{rank.min():.4f} ... {rank.max():.4f}')
    assert rhat.shape == (7,) and np.isfinite(rhat).all() and rhat.max() < RHAT_SCREEN
    assert np.isfinite(rank).all() and rank.max() < RHAT_SCREEN


def test_batch_fit_from_the_map():
    import bisip_amd
    files = bisip_amd.DataFiles()
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', [files[k] for k in sorted(files)[:2]], nwalkers=32, nsteps=20, poly_deg=3)
    np.random.seed(4)
    b.fit(p0='map', seed=1)
    best = b.get_map()
    lp = b.get_log_prob()                                              # (n, E, Wp)
    assert (np.median(lp[0], axis=1) >= best['logp'] - 3 * b.ndim).all()
    with pytest.raises(ValueError, match="'map'"):
        b.fit(p0='mode')
    # the walkers of a spectrum do not depend on how the survey is split over ranks
    np.random.seed(4)
    whole = b._map_walkers(np.random)
    b.close()
    files = bisip_amd.DataFiles()
    part = bisip_amd.SpectraBatch('PolynomialDecomposition', [files[k] for k in sorted(files)[:2]], nwalkers=32, nsteps=20, poly_deg=3,
                                  rank=1, world=2)
    assert part.spectrum_range == (1, 2)
    np.random.seed(4)
    np.testing.assert_array_equal(bits(part._map_walkers(np.random)), bits(whole[1:]))
    part.close()
