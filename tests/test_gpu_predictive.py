"""Posterior predictive checks on the device (bisip_predictive_check_dev), from the C entry point up to the model and
SpectraBatch methods.  The reference of every comparison is the library's own forward over the host copy of the same
samples: the histogram of sign changes and chi2_mean are held to the counts and the bits of the order include/bisip_hip.h
states (bisip_amd.predictive.ordered_predictive_sums), and pit, p_chi2 and p_max, against the long-double yardstick, to the
bounds tests/predictive_bounds.py derives.  Every call goes through chain_harness.GuardedCall: the outputs and the
workspace carry guards, an output that is not asked for stays untouched, and the chain is read through store()'s offset,
stride and NaN padding.

Measured on an MI355X over the cases below: pit, chi2_mean, p_chi2 and p_max at most 0.097, 0.033, 0.048 and 0.046 of their
bounds."""
import functools

import numpy as np
import pytest

import predictive_bounds as pb
from chain_harness import GuardedCall, assert_same_bits, store
from fit_quality_bounds import inverse_variance
from test_gpu_fit_quality import CASES as FIT_CASES
from test_gpu_fit_quality import batch_of, chain_near_a_centre, context, data_near, forward_rows, rows_of
from test_gpu_response import make_batch

pytestmark = pytest.mark.gpu


def run_abi(ctx, chain, E, first=0, asked=(True, True, True), **storage):
    """One call on chain (n, E * Wp, ndim) through store(chain, **storage).  Returns pit (E, 2, N), row (E, 3) and
    sign_changes (E, 2N - 1) int64."""
    import torch
    from bisip_amd import response as rs
    n, W, ndim = chain.shape
    Wp, N = W // E, ctx.N
    stored, offset, stride = store(chain, **storage)
    t = torch.from_numpy(stored).cuda()
    call = GuardedCall()
    ptrs = [call.out('pit', (E, 2, N), asked=asked[0]), call.out('row', (E, 3), asked=asked[1]),
            call.out('sign_changes', (E, 2 * N - 1), dtype=torch.int64, asked=asked[2])]
    nbytes = ctx.predictive_check_workspace(n, E, Wp)
    nseg = rs.plan(n, E, Wp)[1]
    assert nbytes == 8 * E * nseg * (2 * N + 4)                       # as large as the kernels index and no larger
    ctx.predictive_check_dev(first, E, t.data_ptr() + 8 * offset, n, stride, Wp, *ptrs, call.work(nbytes), nbytes, call.stream)
    return call.finish()


def same_bits(a, b, what):
    if a.dtype == np.int64:
        np.testing.assert_array_equal(a, b, err_msg=what)
    else:
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=what)


def check(ctx, chain, E, zn, err, what, Z=None, first=0, n_spectra=None):
    """The call against the stated order and the bounds; twice the same bits, through other storage too, and every subset
    of the outputs.  zn, err: those of the E spectra of the call."""
    from bisip_amd import predictive as pp
    Z = forward_rows(ctx, chain, E) if Z is None else Z
    iv = inverse_variance(err)
    got = run_abi(ctx, chain, E, first)
    want = pp.ordered_predictive_sums(Z, zn, iv, n_spectra)
    np.testing.assert_array_equal(got[2], want[2], err_msg=f'{what}: sign_changes')
    assert_same_bits(got[1][:, 0], want[1][:, 0], f'{what}: chi2_mean')
    ref = pb.reference_and_bounds(Z, zn, iv, pb.K_DEVICE)
    worst = pb.assert_all_within(got[0], got[1], ref, what)
    np.testing.assert_array_equal(got[2].sum(axis=1), ref['good'].sum(axis=1), err_msg=f'{what}: the bins add up to the good rows')
    # glibc's functions in the same order: each side within its own bound of the yardstick
    both = pb.sum_bounds(ref, pb.reference_and_bounds(Z, zn, iv, pb.K_NUMPY))
    fin = np.isfinite(want[0])
    assert (np.abs(got[0] - want[0])[fin] <= both['dpit'].astype(np.float64)[fin]).all(), what
    fin = np.isfinite(want[1])
    assert (np.abs(got[1] - want[1])[fin] <= both['drow'].astype(np.float64)[fin]).all(), what
    print(f'{what}: pit, chi2_mean, p_chi2, p_max at most {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f}, {worst[3]:.3f} of their bounds')
    for kw in ({}, dict(discard=0, thin=1, pad=0), dict(discard=3, thin=4, pad=11)):
        for a, b in zip(run_abi(ctx, chain, E, first, **kw), got):
            same_bits(a, b, f'{what} {kw}')
    for asked in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
                  (False, True, True)):
        some = run_abi(ctx, chain, E, first, asked)                   # (finish() holds the others to their fill)
        for a, b, want_it in zip(some, got, asked):
            if want_it:
                same_bits(a, b, f'{what} {asked}')
    return got, ref


# the shapes of tests/test_gpu_fit_quality.py (rows per spectrum 1, 63, 64, 65, 255, 256, 257, 1024, 1025 and 2500; Wp of 1, 3
# and 5; E of 1, 3 and 256; N of 3, 6, 20 and 32; every one of the 18 model shapes), then N = 1, the smallest a context
# accepts (one bin), and N = 9 and 17, one above a multiple of the point pass's tile of 8 frequencies
CASES = FIT_CASES + [('PolynomialDecomposition', dict(poly_deg=0), 1, 1, 3, 30),
                     ('PeltonColeCole', dict(n_modes=1), 1, 3, 1, 70),
                     ('PeltonColeCole', dict(n_modes=1), 9, 1, 3, 90),
                     ('Dias2000', {}, 17, 3, 1, 300)]


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
    (pit, row, hist), ref = check(ctx, chain, E, zn, err, what, Z)
    assert np.isfinite(pit).all() and np.isfinite(row).all() and (hist.sum(axis=1) == n * Wp).all() and (hist >= 0).all()
    assert ((pit >= 0) & (pit <= 1)).all() and ((row[:, 1:] >= 0) & (row[:, 1:] <= 1)).all()
    assert (ref['x_max'] < 1e6).all(), 'the data lie near the model: else the inputs are wrong'
    if E == 256:
        assert rs.plan(n, E, Wp) == (n * Wp, 1, 256)
    if E == 3:
        # spectra 1 and 2 of the three: first_spectrum > 0, n_spectra < E; the same bits where the plan is the same
        sub = np.ascontiguousarray(chain[:, Wp:])
        part, _ = check(ctx, sub, 2, zn[1:], err[1:], what + ' spectra 1-2', Z[1:], first=1)
        if rs.plan(n, 2, Wp) == rs.plan(n, 3, Wp):
            for a, whole in zip(part, (pit, row, hist)):
                same_bits(a, whole[1:], what + ' spectra 1-2 of 3')
    ctx.close()
    b.close()


def special_case(which, E=3, Wp=3, n=240, n_freq=20):
    """A Cole-Cole context of E spectra and a chain of 720 rows; ``which`` says what is special about spectrum 1."""
    b = make_batch('PeltonColeCole', dict(n_modes=1), n_freq, 2, count=E)
    chain = chain_near_a_centre(b, E, Wp, n, seed=77)
    if which == 'all rows equal':
        chain[:] = np.repeat(chain[:1, ::Wp], Wp, axis=1)
    Z = forward_rows(b.ctx, chain, E)
    zn, err = data_near(Z, seed=7)
    col = Z[1, :, 0, 1]
    if which == 'underflow':                      # the error of one point shrunk: the measurement some 50 sigma below every row
        err[1, 0, 1] = 1e-3 * np.abs(col).max()
        zn[1, 0, 1] = col.min() - 50 * err[1, 0, 1]
    elif which == 'd = 0':                        # the measurement IS the response of row 100, to the bit; one point of others too
        zn[1] = Z[1, 100]
    return b, context(b, zn, err), chain, Z, zn, err


def test_phi_and_q_underflow_to_zero():
    b, ctx, chain, Z, zn, err = special_case('underflow')
    (pit, row, hist), ref = check(ctx, chain, 3, zn, err, 'underflow', Z)
    assert ref['x_min'][1] > 1200                                     # a condition on the input
    assert pit[1, 0, 1] == 0.0 and row[1, 1] == 0.0 and row[1, 2] == 0.0 and np.isfinite(row).all() and hist[1].sum() == 720
    assert (row[[0, 2], 1] > 0).all()
    ctx.close()
    b.close()


def test_a_residual_of_exactly_zero():
    b, ctx, chain, Z, zn, err = special_case('d = 0')
    np.testing.assert_array_equal(Z, forward_rows(ctx, chain, 3))    # the kernel's Z has the bits of forward()
    (pit, row, hist), ref = check(ctx, chain, 3, zn, err, 'd = 0', Z)
    assert hist[1, 0] >= 1 and ref['x_min'][1] == 0.0                 # row 100: T = 0, no sign change
    # that row alone: pit 0.5 everywhere, p_chi2 = p_max = 1, to the bit
    one = np.ascontiguousarray(rows_of(chain, 3)[1:2, 100:101].transpose(1, 0, 2))
    p1, r1, h1 = run_abi(ctx, one, 1, first=1)
    assert (p1 == 0.5).all() and list(r1[0]) == [0.0, 1.0, 1.0] and h1[0, 0] == 1 and h1.sum() == 1
    ctx.close()
    b.close()


def test_all_rows_equal():
    b, ctx, chain, Z, zn, err = special_case('all rows equal')
    (pit, row, hist), ref = check(ctx, chain, 3, zn, err, 'all rows equal', Z)
    assert ((hist > 0).sum(axis=1) == 1).all() and (hist.max(axis=1) == 720).all()
    one = run_abi(ctx, np.ascontiguousarray(chain[:1, ::3]), 3)       # one row per spectrum: the terms themselves
    assert (hist > 0).tolist() == (one[2] > 0).tolist()
    tol = 2 * ref['dpit'].astype(np.float64)
    assert (np.abs(pit - one[0]) <= tol).all() and (np.abs(row - one[1]) <= 2 * ref['drow'].astype(np.float64)).all()
    ctx.close()
    b.close()


def test_a_parameter_that_is_not_finite_stays_in_its_spectrum():
    b, ctx, chain, Z, zn, err = special_case('none')
    clean = run_abi(ctx, chain, 3)
    Wp = 3
    for value, column, sample in ((np.nan, 2, 17), (np.inf, 1, 0), (-np.inf, 0, 239)):
        dirty = chain.copy()
        dirty[sample, Wp + (1 if sample else 0), column] = value      # spectrum 1
        (pit, row, hist), _ = check(ctx, dirty, 3, zn, err, f'{value} in spectrum 1')
        assert np.isnan(pit[1]).all() and np.isnan(row[1]).all() and hist[1].sum() == 720 - 1
        assert (clean[2][1] - hist[1]).sum() == 1 and (clean[2][1] - hist[1]).min() == 0
        for a, c in zip((pit, row, hist), clean):
            same_bits(a[[0, 2]], c[[0, 2]], f'{value}: the neighbours')
    ctx.close()
    b.close()


def test_many_frequencies():
    """Above N = 700 the row outputs are refused on the host and pit alone is served; at 700 everything is."""
    from bisip_amd import predictive as pp
    for n_freq in (700, 701):
        b = batch_of('PeltonColeCole', dict(n_modes=1), n_freq, 1)
        chain = chain_near_a_centre(b, 1, 1, 5, seed=5)
        Z = forward_rows(b.ctx, chain, 1)
        zn, err = data_near(Z, seed=5)
        ctx = context(b, zn, err)
        iv = inverse_variance(err)
        asked = (True, True, True) if n_freq == 700 else (True, False, False)
        pit, row, hist = run_abi(ctx, chain, 1, asked=asked)
        ref = pb.reference_and_bounds(Z, zn, iv, pb.K_DEVICE)
        pb.assert_within(pit, ref, 'pit', f'N = {n_freq}')
        if n_freq == 700:
            want = pp.ordered_predictive_sums(Z, zn, iv)
            np.testing.assert_array_equal(hist, want[2])
            assert_same_bits(row[:, 0], want[1][:, 0], 'chi2_mean')
            pb.assert_all_within(pit, row, ref, 'N = 700')
        else:
            for asked in ((True, True, False), (False, False, True)):
                with pytest.raises(RuntimeError, match='status -4.*row outputs'):
                    run_abi(ctx, chain, 1, asked=asked)
        ctx.close()
        b.close()


def test_refusals_leave_the_outputs_alone():
    """Every refused call is refused on the host before anything is launched: the pointers are never dereferenced."""
    b = make_batch('PeltonColeCole', dict(n_modes=1), 20, 8, count=2)
    ctx = b.ctx
    ok = dict(first=0, count=1, chain=4096, n=8, stride=2 * 8 * 4, Wp=8, pit=4096, row=4096, hist=4096, work=4096,
              nbytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        ctx.predictive_check_dev(a['first'], a['count'], a['chain'], a['n'], a['stride'], a['Wp'], a['pit'], a['row'],
                                 a['hist'], a['work'], a['nbytes'], 0)

    for match, kw in (('neither', dict(pit=0, row=0, hist=0)), ('null', dict(chain=0)), ('spectra', dict(first=2)),
                      ('bad chain shape', dict(count=3)), ('bad chain shape', dict(n=0)), ('sample_stride', dict(stride=31)),
                      ('workspace', dict(work=0)), ('workspace', dict(nbytes=8)), ('workspace', dict(n=300, nbytes=8 * 2 * 44)),
                      ('aligned', dict(hist=4100)), ('aligned', dict(row=4100))):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    assert ctx.predictive_check_workspace(8, 1, 8) == 8 * 44
    assert ctx.predictive_check_workspace(300, 1, 8) == 8 * 3 * 44                    # 2400 rows: three segments
    assert ctx.predictive_check_workspace(0, 1, 8) < 0 and ctx.predictive_check_workspace(8, 3, 8) < 0
    for method in (b.get_predictive_check, b.get_pit):
        with pytest.raises(AssertionError, match='not fitted'):
            method()
    b.close()


# -- through the public interface -------------------------------------------------------------------------------------
KW = dict(discard=10, thin=3)
KEYS = {'pit', 'n_extreme', 'chi2_mean', 'chi2_reduced', 'p_chi2', 'p_max', 'sign_changes', 'p_runs', 'n_rows'}


def check_public(got, Z, zn, err, logp, what):
    """A get_predictive_check result of ONE spectrum against the NumPy definition on its rows: Z (R, 2, N) = forward(flat),
    logp (R,) the stored log-probabilities.  Each side lies within its own bound of the long-double yardstick."""
    from bisip_amd import predictive as pp
    assert set(got) == KEYS
    iv = inverse_variance(err)
    want = pp.predictive_check(Z, zn, err)
    tol = pb.sum_bounds(pb.reference_and_bounds(Z[None], zn, iv, pb.K_DEVICE),
                        pb.reference_and_bounds(Z[None], zn, iv, pb.K_NUMPY, pb.K_ARG_DEFINITION))
    dpit, drow = tol['dpit'][0].astype(np.float64), tol['drow'][0].astype(np.float64)
    N = Z.shape[-1]
    assert got['pit'].shape == (2, N) and (np.abs(got['pit'] - want['pit']) <= dpit).all(), what
    for c, k in enumerate(('chi2_mean', 'p_chi2', 'p_max')):
        assert abs(got[k] - want[k]) <= drow[c], (what, k)
    np.testing.assert_array_equal(got['sign_changes'], want['sign_changes'])
    assert got['sign_changes'].dtype == np.int64 and got['n_rows'] == want['n_rows'] == Z.shape[0]
    assert got['p_runs'] == pytest.approx(want['p_runs'], rel=1e-14) and got['chi2_reduced'] == got['chi2_mean'] / (2 * N)
    assert got['n_extreme'] == ((got['pit'] < 0.025) | (got['pit'] > 0.975)).sum()
    # T is minus twice the log-likelihood up to the constant: the pointwise q add up to the stored log-probability
    assert got['chi2_mean'] == pytest.approx(-2 * (logp.mean() + np.sum(np.log(err ** 2))), rel=1e-9)


@functools.lru_cache(maxsize=None)
def fitted(where):
    from fitted import fitted_model
    return fitted_model(where)


@pytest.mark.parametrize('where', ('device', 'host'))
def test_model_methods(where):
    m = fitted(where)
    flat = m.get_chain(flat=True, **KW)
    Z = m._context().forward(np.ascontiguousarray(flat))
    logp = m._sampler.get_log_prob(flat=True, **KW)
    got = m.get_predictive_check(**KW)
    assert all(isinstance(got[k], float) for k in ('chi2_mean', 'chi2_reduced', 'p_chi2', 'p_max', 'p_runs'))
    assert isinstance(got['n_extreme'], int) and isinstance(got['n_rows'], int)
    check_public(got, Z, m._data['zn'], m._data['zn_err'], logp, f'model, chain on the {where}')
    same_bits(m.get_pit(**KW), got['pit'], 'get_pit')
    # an explicit chain goes up once and gives the same sums in the same order
    again = m.get_predictive_check(chain=flat)
    for k in ('pit', 'sign_changes'):
        same_bits(again[k], got[k], k)
    assert all(again[k] == got[k] for k in KEYS - {'pit', 'sign_changes'})
    with pytest.warns(UserWarning, match='No samples were discarded'):
        assert m.get_pit().shape == (2, Z.shape[-1])
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_predictive_check(chain=flat, discard=3)


@pytest.mark.parametrize('where', ('device', 'host'))
def test_spectra_batch_methods(where):
    import bisip_amd
    from bisip_amd import predictive as pp
    from bisip_amd.chainview import ChainView
    files = bisip_amd.DataFiles()
    E, Wp = 3, 8
    b = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in sorted(files)[:E]], nwalkers=Wp, nsteps=40, n_modes=1)
    p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(1).randn(E, Wp, 4)
    b.fit(p0, seed=6, chain=where)
    got = b.get_predictive_check(**KW)
    assert set(got) == KEYS and got['pit'].shape == (E, 2, b.N) and got['sign_changes'].shape == (E, 2 * b.N - 1)
    assert all(got[k].shape == (E,) for k in KEYS - {'pit', 'sign_changes'})
    same_bits(b.get_pit(**KW), got['pit'], 'get_pit')
    flat = b.get_chain(flat=True, **KW)                                # (E, n * Wp, ndim)
    Z = b.forward(flat)
    logp = b.get_log_prob(**KW)                                        # (n, E, Wp)
    view = b._fitted().used_samples_dev(**KW)
    whole = b._fitted().predictive_check(**KW)
    for e in range(E):
        one = {k: (v[e] if v[e].ndim else v[e].item()) for k, v in got.items()}
        check_public(one, Z[e], b.zn[e], b.zn_err[e], logp[:, e].reshape(-1), f'spectrum {e}, chain on the {where}')
        # a one-spectrum call with first_spectrum = e: the plan of one spectrum is that of three here, the same bits
        single = ChainView(view.tensor, view.n, 1, Wp, b.ndim, view.offset + e * Wp * b.ndim, view.stride, view.backend)
        for a, w in zip(pp.device_predictive_check(single, b.ctx, first_spectrum=e), whole):
            same_bits(a[0], w[e], f'spectrum {e} alone')
    with pytest.raises(ValueError):
        b.get_predictive_check(discard=40)
    b.close()


# -- detection ------------------------------------------------------------------------------------------------------
def two_mode_table(n_freq=20, seed=2, noise=0.01):
    """A double Cole-Cole spectrum (the truth of bisip_amd.synthetic) with 1 % of noise on the amplitude and 10 mrad on the
    phase, and errors that say so: 1 % of |Z| on either part."""
    from bisip_amd import synthetic as sy
    f = np.logspace(np.log10(sy.F_MAX), np.log10(sy.F_MIN), n_freq)
    w = 2 * np.pi * f
    z = np.zeros(n_freq, dtype=np.complex128)
    for m, lt, c in zip(sy.TRUTH_M, sy.TRUTH_LN_TAU, sy.TRUTH_C):
        z += m * (1.0 - 1.0 / (1.0 + (1j * w * np.exp(lt)) ** c))
    z = sy.TRUTH_SCALE * (1.0 - z)
    rng = np.random.default_rng(seed)
    amp = np.abs(z) * (1 + noise * rng.standard_normal(n_freq))
    pha = 1e3 * (np.angle(z) + noise * rng.standard_normal(n_freq))
    return np.column_stack([f, amp, pha, noise * amp, np.full(n_freq, 1e3 * noise)])


def test_a_missing_mode_is_detected(tmp_path):
    """One Cole-Cole mode fitted to a spectrum of two: the chi-square says so with a probability below 1e-3, where the fit
    with two modes passes every check.  (With the host sampler around a NumPy forward of the same spectrum and seed the
    definition gave chi2_reduced 0.97, p_chi2 0.54, p_runs 0.64, p_max 0.41 with two modes, and 3.15, 1e-10, 0.02, 4e-4 with
    one.)"""
    import bisip_amd
    from bisip_amd import predictive as pp
    from bisip_amd import synthetic as sy
    path = tmp_path / 'two_modes.csv'
    np.savetxt(path, two_mode_table(), delimiter=',', fmt='%.18e', header='freq, amp, pha, amp_err, pha_err', comments='')
    checks = {}
    for n_modes in (1, 2):
        m = bisip_amd.PeltonColeCole(str(path), n_modes=n_modes, nwalkers=32, nsteps=600)
        if n_modes == 2:
            m.params.update(log_tau1=[-5, 5], log_tau2=[-15, -10])
            centre = np.array([1.0, *sy.TRUTH_M, *sy.TRUTH_LN_TAU, *sy.TRUTH_C])
        else:
            centre = np.array([1.0, 0.5, -12.0, 0.6])
        centre[0] = sy.TRUTH_SCALE / m._data['norm_factor']
        np.random.seed(2)
        m.fit(p0=centre + 1e-3 * np.random.randn(32, centre.size), chain='device')
        got = m.get_predictive_check(discard=300)
        flat = m.get_chain(flat=True, discard=300)
        Z = m._context().forward(np.ascontiguousarray(flat))
        logp = m._sampler.get_log_prob(flat=True, discard=300)
        check_public(got, Z, m._data['zn'], m._data['zn_err'], logp, f'{n_modes} modes')
        checks[n_modes] = pp.predictive_check(Z, m._data['zn'], m._data['zn_err'])          # the definition alone
        print(n_modes, {k: v for k, v in checks[n_modes].items() if k not in ('pit', 'sign_changes')})
    assert checks[1]['p_chi2'] < 1e-3 and checks[1]['chi2_reduced'] > 2
    assert checks[2]['p_chi2'] > 1e-3 and checks[2]['p_runs'] > 1e-3
    assert checks[2]['chi2_reduced'] < checks[1]['chi2_reduced'] and checks[2]['n_extreme'] < checks[1]['n_extreme']
