"""WAIC, DIC and the per-point misfit on the device (bisip_fit_quality_dev), from the C entry point up to the model and
SpectraBatch methods.  The reference of every comparison is the library's own forward over the host copy of the same
samples: mean_q and var_q are held to the bits of the order include/bisip_hip.h states
(bisip_amd.fitquality.ordered_fit_sums), and all three outputs, against the long-double definitions, to the bounds
tests/fit_quality_bounds.py derives.  Every call goes through chain_harness.GuardedCall: the outputs and the workspace
carry guards, an output that is not asked for stays untouched, and the chain is read through store()'s offset, stride
and NaN padding."""
import functools

import numpy as np
import pytest

from chain_harness import GuardedCall, assert_same_bits, store
from conftest import assert_logp_close
from fit_quality_bounds import K_DEVICE, K_NUMPY, U, assert_all_within, inverse_variance, reference_and_bounds
from test_gpu_response import MODEL_ID, inside, make_batch

pytestmark = pytest.mark.gpu

NAMES = ('mean_q', 'var_q', 'lmeh')
SCATTER = 1e-2                     # relative: how far the rows of a chain lie from their spectrum's centre


def model_options(b):
    if b.model == 'PolynomialDecomposition':
        return dict(poly_deg=b.poly_deg, c_exp=b.c_exp, taus=b.taus, log_taus=b.log_taus)
    if b.model == 'PeltonColeCole':
        return dict(n_modes=b.n_modes)
    return {}


def batch_of(model, kw, n_freq, E):
    """A SpectraBatch of E spectra: the frequencies, the prior box and the model's options.  N = 20: the bundled spectra
    while they last (five); else synthetic ones."""
    if n_freq == 20 and E <= 5:
        return make_batch(model, kw, n_freq, 2, count=E)
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    return bisip_amd.SpectraBatch(model, [synthetic_columns(n_freq, i) for i in range(E)], nwalkers=2, nsteps=8, **kw)


def chain_near_a_centre(b, E, Wp, n, seed):
    """(n, E * Wp, ndim): the rows of every spectrum scattered about a centre of its own inside the prior box."""
    lo, hi = b.param_bounds
    centre = inside(b.model, lo, hi, (E,), seed)
    rng = np.random.default_rng(seed)
    x = centre[None, :, None, :] * (1 + SCATTER * rng.normal(size=(n, E, Wp, lo.size)))
    x = np.clip(x, lo + 1e-3 * (hi - lo), hi - 1e-3 * (hi - lo))
    return np.ascontiguousarray(x.reshape(n, E * Wp, lo.size))


def rows_of(chain, E):
    """(n, E * Wp, ndim) -> (E, R, ndim), row r = k * Wp + w of every spectrum."""
    n, W, ndim = chain.shape
    return np.ascontiguousarray(chain.reshape(n, E, W // E, ndim).transpose(1, 0, 2, 3).reshape(E, -1, ndim))


def forward_rows(ctx, chain, E):
    """Z (E, R, 2, N): ctx.forward of every spectrum's rows; a row with a parameter that is not finite counts as NaN."""
    rows = rows_of(chain, E)
    bad = ~np.isfinite(rows).all(axis=-1)
    finite = np.where(bad[..., None], rows[~bad][0], rows)            # (forward is given finite rows only)
    Z = ctx.forward(finite.reshape(-1, rows.shape[-1])).reshape(E, rows.shape[1], 2, ctx.N)
    Z[bad] = np.nan
    return Z


def data_near(Z, seed):
    """A measurement within about an error of the first row's response, errors of 2 % of it and a floor."""
    rng = np.random.default_rng(seed)
    err = 0.02 * np.abs(Z[:, 0]) * rng.uniform(0.5, 2.0, Z[:, 0].shape) + 3e-3
    return Z[:, 0] + err * rng.normal(size=err.shape), err


def context(b, zn, err):
    from bisip_amd import _hip
    return _hip.HipContext(MODEL_ID[b.model], b.w, zn, err, b.param_bounds, **model_options(b))


def run_abi(ctx, chain, E, first=0, asked=(True, True, True), **storage):
    """One call on chain (n, E * Wp, ndim) through store(chain, **storage).  Returns the three outputs (E, 2, N)."""
    import torch
    from bisip_amd import response as rs
    n, W, ndim = chain.shape
    Wp, N = W // E, ctx.N
    stored, offset, stride = store(chain, **storage)
    t = torch.from_numpy(stored).cuda()
    call = GuardedCall()
    ptrs = [call.out(name, (E, 2, N), asked=a) for name, a in zip(NAMES, asked)]
    nbytes = ctx.fit_quality_workspace(n, E, Wp)
    nseg = rs.plan(n, E, Wp)[1]
    assert nbytes == (8 * E * (8 * nseg + 2) * N if nseg > 1 else 0)      # as large as the kernels index and no larger
    ctx.fit_quality_dev(first, E, t.data_ptr() + 8 * offset, n, stride, Wp, *ptrs, call.work(nbytes), nbytes, call.stream)
    return call.finish()


def check(ctx, chain, E, zn, err, what, Z=None, first=0, n_spectra=None):
    """The call against the stated order and the bounds; twice the same bits, through other storage too, and every subset
    of the outputs.  zn, err: those of the E spectra of the call."""
    from bisip_amd import fitquality as fq
    Z = forward_rows(ctx, chain, E) if Z is None else Z
    iv = inverse_variance(err)
    got = run_abi(ctx, chain, E, first)
    want = fq.ordered_fit_sums(Z, zn, iv, n_spectra)
    assert_same_bits(got[0], want[0], f'{what}: mean_q')
    assert_same_bits(got[1], want[1], f'{what}: var_q')
    ref = reference_and_bounds(Z, zn, iv, n_spectra, K_DEVICE)
    worst = assert_all_within(got, ref, what)
    # NumPy's exp and log in the same order: each side within its own bound of the definition
    both = (ref['dlmeh'] + reference_and_bounds(Z, zn, iv, n_spectra, K_NUMPY)['dlmeh']).astype(np.float64)
    fin = np.isfinite(want[2])
    assert (np.abs(got[2] - want[2])[fin] <= both[fin]).all(), what
    print(f'{what}: mean_q, var_q, lmeh at most {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f} of their bounds')
    for kw in ({}, dict(discard=0, thin=1, pad=0), dict(discard=3, thin=4, pad=11)):
        again = run_abi(ctx, chain, E, first, **kw)
        for a, b in zip(again, got):
            np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=f'{what} {kw}')
    for asked in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        some = run_abi(ctx, chain, E, first, asked)                   # (finish() holds the others to their fill)
        for a, b, want_it in zip(some, got, asked):
            if want_it:
                np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=f'{what} {asked}')
    return got, ref


# model, options, N, E, Wp, samples.  Rows per spectrum 1, 63, 64, 65, 255, 256, 257, 1024, 1025 and 2500: both sides of a
# run of 64 slots, of the 256 slots and of the smallest segment, and three ragged segments; Wp = 3 and 5 put the rows of a
# slot's stride across samples; E = 256 takes the one-kernel path; N = 3 lies below the tile of 4 frequencies, 6 is no
# multiple of it, 20 and 32 are (20 is no multiple of the response kernel's tile of 8)
CASES = [('PolynomialDecomposition', dict(poly_deg=0), 3, 1, 1, 1),
         ('PeltonColeCole', dict(n_modes=1), 20, 3, 3, 21),
         ('Dias2000', {}, 32, 1, 1, 64),
         ('Shin2015', {}, 20, 3, 5, 13),
         ('PolynomialDecomposition', dict(poly_deg=5), 32, 1, 5, 51),
         ('PeltonColeCole', dict(n_modes=2), 3, 3, 1, 256),
         ('PolynomialDecomposition', dict(poly_deg=0), 20, 1, 1, 257),
         ('PeltonColeCole', dict(n_modes=1), 32, 3, 1, 1024),
         ('Dias2000', {}, 3, 1, 5, 205),
         ('Shin2015', {}, 6, 3, 3, 100),
         ('PeltonColeCole', dict(n_modes=2), 32, 1, 5, 500),
         ('PolynomialDecomposition', dict(poly_deg=5), 20, 3, 5, 500),
         ('PeltonColeCole', dict(n_modes=2), 20, 256, 3, 9)]
# the other shapes a context can have, at the smallest sizes above: each of the 18 takes a kernel of its own
CASES += [('PolynomialDecomposition', dict(poly_deg=p), 3 if p <= 2 else 20, 1, 1 + p % 3, 64 - 3 * p) for p in (1, 2, 3, 4, 6, 7, 8, 9, 10)]
CASES += [('PeltonColeCole', dict(n_modes=d), 20, 1, d - 2, 9 * d) for d in (3, 4, 5)]


@pytest.mark.parametrize('model,kw,n_freq,E,Wp,n', CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_entry_point(model, kw, n_freq, E, Wp, n):
    from bisip_amd import response as rs
    b = batch_of(model, kw, n_freq, E)
    assert b.n_spectra == E
    chain = chain_near_a_centre(b, E, Wp, n, seed=n + Wp)
    Z = forward_rows(b.ctx, chain, E)
    zn, err = data_near(Z, seed=n)
    ctx = context(b, zn, err)
    what = f'{model} {kw} N={n_freq} E={E} Wp={Wp} n={n}'
    got, ref = check(ctx, chain, E, zn, err, what, Z)
    assert (ref['q_max'] < 1e6).all(), 'the data lie near the model: else the inputs are wrong'
    if n * Wp == 1:
        assert np.isnan(got[1]).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    if E == 256:
        assert rs.plan(n, E, Wp) == (n * Wp, 1, 256) and ctx.fit_quality_workspace(n, E, Wp) == 0
    if E == 3:
        # spectra 1 and 2 of the three: first_spectrum > 0, n_spectra < E; the same bits where the plan is the same
        sub = np.ascontiguousarray(chain[:, Wp:])
        part, _ = check(ctx, sub, 2, zn[1:], err[1:], what + ' spectra 1-2', Z[1:], first=1)
        if rs.plan(n, 2, Wp) == rs.plan(n, 3, Wp):
            for a, whole in zip(part, got):
                np.testing.assert_array_equal(a.view(np.uint64), whole[1:].view(np.uint64))
    ctx.close()
    b.close()


def special_case(which, E=3, Wp=3, n=240, n_freq=20):
    """A Cole-Cole context of E spectra and a chain of 720 rows whose q at point (part 0, frequency 1) of spectrum 1
    breaks a naive kernel; elsewhere the data lie near the model."""
    b = make_batch('PeltonColeCole', dict(n_modes=1), n_freq, 2, count=E)
    chain = chain_near_a_centre(b, E, Wp, n, seed=77)
    if which == 'all rows equal':
        chain[:] = np.repeat(chain[:1, ::Wp], Wp, axis=1)
    Z = forward_rows(b.ctx, chain, E)
    zn, err = data_near(Z, seed=7)
    col = Z[1, :, 0, 1]
    if which == 'all above 1500':                 # the error of one point shrunk: exp(-q / 2) underflows to 0
        zn[1, 0, 1] = col.min() - 0.05 * np.abs(col).max()
        err[1, 0, 1] = 1e-3 * np.abs(col).max()
    elif which == 'first row far out':            # q of the median row is 0, that of the first 2500
        zn[1, 0, 1] = np.sort(col)[col.size // 2]
        assert col[0] != zn[1, 0, 1]
        err[1, 0, 1] = np.abs(col[0] - zn[1, 0, 1]) / 50
    elif which == 'decreasing':                   # the rows of spectrum 1 in the order of falling q: a rescale at every row
        order = np.argsort(-(zn[1, 0, 1] - col) ** 2, kind='stable')
        rows = rows_of(chain, E)
        rows[1] = rows[1][order]
        chain = np.ascontiguousarray(rows.reshape(E, n, Wp, -1).transpose(1, 0, 2, 3).reshape(n, E * Wp, -1))
        Z[1] = Z[1][order]
    return b, context(b, zn, err), chain, Z, zn, err


def q_of_the_point(Z, zn, err):
    from bisip_amd import fitquality as fq
    return fq.pointwise_q(Z[1], zn[1], inverse_variance(err[1]))[:, 0, 1]


def test_every_q_above_1500():
    b, ctx, chain, Z, zn, err = special_case('all above 1500')
    got, ref = check(ctx, chain, 3, zn, err, 'q > 1500', Z)
    assert ref['q_min'][1, 0, 1] > 1500                               # a condition on the input
    assert np.isfinite(got[2]).all() and got[2][1, 0, 1] < -750
    ctx.close()
    b.close()


def test_first_row_far_out():
    b, ctx, chain, Z, zn, err = special_case('first row far out')
    got, ref = check(ctx, chain, 3, zn, err, 'first row far out', Z)
    assert q_of_the_point(Z, zn, err)[0] - ref['q_min'][1, 0, 1] > 1500   # a condition on the input
    assert np.isfinite(got[2]).all()
    ctx.close()
    b.close()


def test_q_decreasing_along_every_slot():
    b, ctx, chain, Z, zn, err = special_case('decreasing')
    assert (np.diff(q_of_the_point(Z, zn, err)) < 0).all()
    np.testing.assert_array_equal(Z, forward_rows(ctx, chain, 3))
    check(ctx, chain, 3, zn, err, 'decreasing', Z)
    ctx.close()
    b.close()


def test_all_rows_equal():
    from bisip_amd import fitquality as fq
    b, ctx, chain, Z, zn, err = special_case('all rows equal')
    got, ref = check(ctx, chain, 3, zn, err, 'all rows equal', Z)
    q0 = fq.pointwise_q(Z[:, 0], zn, inverse_variance(err))
    assert (got[1] == 0.0).all()
    np.testing.assert_array_equal(got[0], q0)
    assert (np.abs(got[2] - (-q0 / 2)) <= ref['dlmeh'].astype(np.float64)).all()
    ctx.close()
    b.close()


def test_a_parameter_that_is_not_finite_stays_in_its_spectrum():
    b, ctx, chain, Z, zn, err = special_case('none')
    clean = run_abi(ctx, chain, 3)
    Wp = 3
    for value, column, sample in ((np.nan, 2, 17), (np.inf, 1, 0), (-np.inf, 0, 239)):
        dirty = chain.copy()
        dirty[sample, Wp + (1 if sample else 0), column] = value      # spectrum 1; sample 0, walker 0 is the row of the shift
        got, _ = check(ctx, dirty, 3, zn, err, f'{value} in spectrum 1')
        for a, c in zip(got, clean):
            assert np.isnan(a[1]).all()
            np.testing.assert_array_equal(a[[0, 2]].view(np.uint64), c[[0, 2]].view(np.uint64))
    ctx.close()
    b.close()


def test_refusals_leave_the_outputs_alone():
    """Every refused call is refused on the host before anything is launched: the pointers are never dereferenced."""
    b = make_batch('PeltonColeCole', dict(n_modes=1), 20, 8, count=2)
    ctx = b.ctx
    ok = dict(first=0, count=1, chain=4096, n=8, stride=2 * 8 * 4, Wp=8, mean_q=4096, var_q=4096, lmeh=4096, work=4096,
              nbytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        ctx.fit_quality_dev(a['first'], a['count'], a['chain'], a['n'], a['stride'], a['Wp'], a['mean_q'], a['var_q'],
                            a['lmeh'], a['work'], a['nbytes'], 0)

    for match, kw in (('neither', dict(mean_q=0, var_q=0, lmeh=0)), ('null', dict(chain=0)), ('spectra', dict(first=2)),
                      ('bad chain shape', dict(count=3)), ('bad chain shape', dict(n=0)), ('sample_stride', dict(stride=31)),
                      ('workspace', dict(n=300, work=0)), ('workspace', dict(n=300, nbytes=8)), ('aligned', dict(lmeh=4100))):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    assert ctx.fit_quality_workspace(8, 1, 8) == 0
    assert ctx.fit_quality_workspace(300, 1, 8) == 8 * (3 * 8 + 2) * ctx.N        # 2400 rows: three segments
    assert ctx.fit_quality_workspace(0, 1, 8) < 0 and ctx.fit_quality_workspace(8, 3, 8) < 0
    for method in (b.get_pointwise_misfit, b.get_waic, b.get_dic):
        with pytest.raises(AssertionError, match='not fitted'):
            method()
    b.close()


# -- through the public interface -------------------------------------------------------------------------------------
KW = dict(discard=10, thin=3)


def check_public(mean_q, waic, dic, Z, zn, err, flat, logp, log_prob_of, what):
    """The three methods' results of ONE spectrum against the NumPy definitions on its rows: Z (R, 2, N) = forward(flat),
    logp (R,) the stored log-probabilities.  Each side lies within its own bound of the long-double definition."""
    from bisip_amd import fitquality as fq
    iv = inverse_variance(err)
    dev = reference_and_bounds(Z[None], zn, iv, 1, K_DEVICE)
    host = reference_and_bounds(Z[None], zn, iv, 1, K_NUMPY)
    tol = {k: (dev['d' + k] + host['d' + k])[0].astype(np.float64) for k in NAMES}
    d_mean, d_var, d_lmeh = fq.fit_sums(fq.pointwise_q(Z, zn, iv))
    assert (np.abs(mean_q - d_mean) <= tol['mean_q']).all(), what
    want = fq.waic(fq.pointwise_log_lik(Z, zn, err))
    # lppd = lmeh - log sigma^2 and elpd_i = lppd - p_waic_i: one rounding each on either side; the sums: 2N - 1 more
    n_points = mean_q.size
    t_lppd = tol['lmeh'] + 2 * U * np.abs(want['lppd'])
    t_p = tol['var_q'] / 4 + 2 * U * np.abs(want['p_waic_i'])
    t_elpd = t_lppd + t_p + 2 * U * np.abs(want['elpd_i'])
    assert (np.abs(waic['lppd'] - want['lppd']) <= t_lppd).all(), what
    assert (np.abs(waic['p_waic_i'] - want['p_waic_i']) <= t_p).all(), what
    assert (np.abs(waic['elpd_i'] - want['elpd_i']) <= t_elpd).all(), what
    assert abs(waic['elpd_waic'] - want['elpd_waic']) <= t_elpd.sum() + 2 * n_points * U * np.abs(want['elpd_i']).sum(), what
    assert abs(waic['p_waic'] - want['p_waic']) <= t_p.sum() + 2 * n_points * U * want['p_waic_i'].sum(), what
    assert waic['waic'] == -2 * waic['elpd_waic'] and waic['n_high'] == want['n_high']
    # se = sqrt(n) std(elpd_i): a std moves by at most the largest change of an element; its own roundings: n u of the
    # largest element
    assert abs(waic['se'] - want['se']) <= np.sqrt(n_points) * (t_elpd.max() + 2 * n_points * U * np.abs(want['elpd_i']).max()), what
    # the pointwise log-likelihoods add up to the stored log-probability: their means too
    assert_logp_close(np.array([np.sum(-mean_q / 2 - np.log(err ** 2))]), np.array([logp.mean()]))
    want_dic = fq.dic(logp.mean(), log_prob_of(flat.mean(axis=0)))
    for k in ('mean_deviance', 'deviance_at_mean', 'dic'):
        assert_logp_close(np.array([dic[k]]), np.array([want_dic[k]]))
    assert dic['p_d'] == dic['mean_deviance'] - dic['deviance_at_mean'] and dic['dic'] == dic['mean_deviance'] + dic['p_d']


@functools.lru_cache(maxsize=None)
def fitted_model():
    import bisip_amd
    m = bisip_amd.PeltonColeCole(bisip_amd.DataFiles()['SIP-K389175'], n_modes=1, nwalkers=8, nsteps=40)
    p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(3).randn(8, 4)
    np.random.seed(8)
    m.fit(p0=p0, chain='device')
    assert m._sampler.chain_on_device
    return m


def test_model_methods():
    m = fitted_model()
    flat = m.get_chain(flat=True, **KW)
    Z = m._context().forward(np.ascontiguousarray(flat))
    logp = m._sampler.get_log_prob(flat=True, **KW)
    with pytest.warns(UserWarning, match='No samples were discarded'):
        assert m.get_pointwise_misfit().shape == (2, Z.shape[-1])
    mean_q, waic, dic = m.get_pointwise_misfit(**KW), m.get_waic(**KW), m.get_dic(**KW)
    assert mean_q.shape == waic['lppd'].shape == waic['p_waic_i'].shape == waic['elpd_i'].shape == (2, Z.shape[-1])
    assert all(isinstance(waic[k], float) for k in ('elpd_waic', 'p_waic', 'waic', 'se')) and isinstance(waic['n_high'], int)
    assert set(dic) == {'dic', 'p_d', 'mean_deviance', 'deviance_at_mean'}
    check_public(mean_q, waic, dic, Z, m._data['zn'], m._data['zn_err'], flat, logp, m.log_prob, 'model')
    # an explicit chain goes up once and gives the same sums in the same order
    np.testing.assert_array_equal(m.get_pointwise_misfit(chain=flat).view(np.uint64), mean_q.view(np.uint64))
    np.testing.assert_array_equal(m.get_waic(chain=flat)['elpd_i'].view(np.uint64), waic['elpd_i'].view(np.uint64))
    assert_logp_close(np.array([m.get_dic(chain=flat)['dic']]), np.array([dic['dic']]))
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_waic(chain=flat, discard=3)


def test_spectra_batch_methods():
    import bisip_amd
    from bisip_amd import fitquality as fq
    from bisip_amd.chainview import ChainView
    files = bisip_amd.DataFiles()
    E, Wp = 3, 8
    b = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in sorted(files)[:E]], nwalkers=Wp, nsteps=40, n_modes=1)
    p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(1).randn(E, Wp, 4)
    b.fit(p0, seed=6, chain='device')
    mean_q, waic, dic = b.get_pointwise_misfit(**KW), b.get_waic(**KW), b.get_dic(**KW)
    assert mean_q.shape == waic['elpd_i'].shape == (E, 2, b.N)
    assert all(waic[k].shape == (E,) for k in ('elpd_waic', 'p_waic', 'waic', 'se', 'n_high'))
    assert all(dic[k].shape == (E,) for k in ('dic', 'p_d', 'mean_deviance', 'deviance_at_mean'))
    flat = b.get_chain(flat=True, **KW)                                # (E, n * Wp, ndim)
    Z = b.forward(flat)
    logp = b.get_log_prob(**KW)                                        # (n, E, Wp)
    view = b._fitted().used_samples_dev(**KW)
    for e in range(E):
        one_waic = {k: v[e] for k, v in waic.items()}
        one_dic = {k: v[e] for k, v in dic.items()}
        log_prob_of = lambda theta, e=e: b.log_prob(np.tile(theta, (E, 1, 1)))[e, 0]
        check_public(mean_q[e], one_waic, one_dic, Z[e], b.zn[e], b.zn_err[e], flat[e], logp[:, e].reshape(-1), log_prob_of,
                     f'spectrum {e}')
        # a one-spectrum call with first_spectrum = e: the plan of one spectrum is that of three here, the same bits
        one = ChainView(view.tensor, view.n, 1, Wp, b.ndim, view.offset + e * Wp * b.ndim, view.stride, view.backend)
        for a, whole in zip(fq.device_fit_quality(one, b.ctx, first_spectrum=e), b._fitted().fit_quality(**KW)):
            np.testing.assert_array_equal(a[0].view(np.uint64), whole[e].view(np.uint64))
    with pytest.raises(ValueError):
        b.get_waic(discard=40)
    b.close()
