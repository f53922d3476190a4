"""The differential-evolution and snooker moves on the device (csrc/move_kernels.h; bisip_move_*_dev) against their NumPy
statement (bisip_amd/moves.py): the draw kernel against ``move_stream``; the chain, the stored log-probability and the
acceptance of a device run against a replay of the definition around ``ctx.logprob`` on the arrays the device drew, bit
for bit; the moves against a posterior that is drawn exactly (tests/exact_posterior.py, judged as
tests/test_gpu_exact_posterior.py judges the stretch move); the guard of the QR-reduced tiers under a mixture; the public
surface.

The replay's proposal is the device's bit for bit (subtract, multiply, add, divide and square root are correctly rounded
on both sides and nothing is contracted).  The snooker factor passes through ``log`` on both sides and enters the
acceptance test only: a last-bit difference there could flip a decision whose two sides agree to 1e-16, which no run here
comes near."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_posterior as ep
from numpy_move_backend import MOVE_ARRAYS, NumpyMoveBackend
from test_gpu_exact_posterior import REDUCED, _batch, _check_logprob, _judge, _lone_context
from test_gpu_parity import make_ctx
from test_gpu_sampler import CASES, _case, _start, _valley

pytestmark = pytest.mark.gpu

MIXTURE = [('de', 0.8), ('snooker', 0.2)]
THREE = [('de', 1.0), ('snooker', 1.0), ('stretch', 1.0)]
MOVES = {'de': 'de', 'snooker': 'snooker', 'three': THREE}


class DeviceDrawnBackend(NumpyMoveBackend):
    """The NumPy statement of the moves on the arrays the DEVICE drew (bisip_move_draw_dev, bisip_stretch_draw_dev)."""

    def __init__(self, ctx, n_ensembles=1):
        super().__init__(ctx.logprob, n_ensembles)
        self.ctx = ctx

    def _from_device(self, st, names, launch):
        import torch
        dev = {name: torch.empty(st[name].shape, dtype=st[name].dtype, device='cuda') for name in names}
        launch(st['perm'].cuda().data_ptr(), *[dev[name].data_ptr() for name in names], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for name in names:
            st[name][:] = dev[name].cpu()

    def draw_moves(self, st, W, seed, step0, n_steps, g0, sigma):
        self._from_device(st, ['mv_' + name for name in MOVE_ARRAYS],
                          lambda perm, *rest: self.ctx.move_draw_dev(W, seed, step0, n_steps, perm, g0, sigma, *rest))

    def draw(self, st, W, a, seed, step0, n_steps):
        self._from_device(st, ['active', 'partner', 'zz', 'factor', 'logu'],
                          lambda perm, *rest: self.ctx.stretch_draw_dev(W, a, seed, step0, n_steps, perm, *rest))


def _same(a, b):
    assert np.array_equal(a.get_chain(), b.get_chain())
    assert np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)


def _one_mode_batch(Wp, nsteps=1):
    """Three different spectra in one batch context, single Cole-Cole (ndim 4: ensembles of 8 are allowed)."""
    import bisip_amd
    from test_gpu_modes import spectrum_files
    return bisip_amd.SpectraBatch('PeltonColeCole', list(spectrum_files()), nwalkers=Wp, nsteps=nsteps, n_modes=1)


# ---------------------------------------------------------------------------------------------------------------
# the draw kernel
# ---------------------------------------------------------------------------------------------------------------

def _drawn(ctx, W, E, seed, step0, n, g0, sigma):
    import torch
    from bisip_amd.sampler import affine_splits
    perm = affine_splits(seed, W, step0, n)
    nh = (W + 1) // 2
    bufs = {name: torch.empty((n, 2, E * nh), dtype=torch.float64 if name in ('gamma', 'logu') else torch.int32, device='cuda')
            for name in MOVE_ARRAYS}
    ctx.move_draw_dev(W, seed, step0, n, torch.from_numpy(perm).cuda().data_ptr(), g0, sigma,
                      *[bufs[name].data_ptr() for name in MOVE_ARRAYS], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return perm, {name: t.cpu().numpy() for name, t in bufs.items()}


def _check_draw(got, want):
    for name in ('active', 'p0', 'p1', 'p2'):
        assert np.array_equal(got[name], want[name]), name
    np.testing.assert_allclose(got['gamma'], want['gamma'], rtol=1e-15, atol=0)
    np.testing.assert_allclose(got['logu'], want['logu'], rtol=1e-15, atol=0)


def test_move_draw_kernel_matches_its_statement():
    """bisip_move_draw_dev against moves.move_stream: 4 walkers (halves of two: no third partner), 6 and 7 (halves of
    three), 32 / 33 (the flat launch shape), 4096, and 65537 (past 2^16 walkers the modular products need 64 bits); a
    batch of three ensembles of 8 keyed by a survey offset.  Integers exact, gamma and ln u to 1e-15."""
    from bisip_amd.moves import move_stream
    g = np.load(_case('case16_'))
    ctx = make_ctx(g, 'PeltonColeCole')
    for W, n, step0, seed, g0, sigma in [(4, 40, 0, 1, 0.84, 1e-5), (6, 30, 3, 2, 0.84, 1e-5), (7, 30, 1000, 0xdeadbeefcafe, 0.5, 1e-2),
                                         (32, 9, 0, 4, 0.84, 1e-5), (33, 5, 7, 5, 0.84, 1e-5), (4096, 3, 7, 42, 0.84, 1e-5),
                                         (65537, 2, 11, 5, 0.84, 1e-5)]:
        perm, got = _drawn(ctx, W, 1, seed, step0, n, g0, sigma)
        _check_draw(got, move_stream(W, seed, step0, perm, g0, sigma))
        if W == 4:
            assert not got['p2'].any()
        assert np.isfinite(got['gamma']).all() and np.isfinite(got['logu'][:, 0]).all()
    with pytest.raises(ValueError, match='at least 4'):
        _drawn(ctx, 3, 1, 1, 0, 2, 0.84, 1e-5)
    ctx.close()
    batch = _one_mode_batch(8)
    batch.ctx.set_spectrum_offset(5)
    perm, got = _drawn(batch.ctx, 8, 3, 77, 2, 12, 0.84, 1e-5)
    _check_draw(got, move_stream(8, 77, 2, perm, 0.84, 1e-5, E=3, e0=5))
    batch.close()


# ---------------------------------------------------------------------------------------------------------------
# bit-identical replay
# ---------------------------------------------------------------------------------------------------------------

def _replay_lone(ctx, p0, steps=40, seed=2024):
    """'de', 'snooker' and the three-way mixture on a lone context: the device run equals the replay, and moves."""
    from bisip_amd.sampler import DeviceEnsembleSampler
    W, ndim = p0.shape
    for name, moves in MOVES.items():
        dev = DeviceEnsembleSampler(W, ndim, ctx, rng='philox', seed=seed, moves=moves)
        dev.run_mcmc(p0, steps)
        assert dev.last_path == 'launch-per-half-step' and dev.last_stream == 'arrays'
        rep = DeviceEnsembleSampler(W, ndim, backend=DeviceDrawnBackend(ctx), rng='philox', seed=seed, moves=moves, chunk=25)
        rep.run_mcmc(p0, steps)
        _same(dev, rep)
        assert 0.0 < dev.acceptance_fraction.mean() < 1.0, (name, W, dev.acceptance_fraction.mean())


# test_gpu_sampler.CASES and, as its multi-workgroup test adds it, the compensated QR-reduced kernel
REPLAY_CASES = CASES + [('case13_', 'PolynomialDecomposition', 'reduced_comp'), ('case04_', 'PolynomialDecomposition', 'reduced_comp')]


@pytest.mark.parametrize('prefix,model,variant', REPLAY_CASES)
def test_device_moves_equal_their_replay(prefix, model, variant):
    """Every model and formulation -- the plain reduced kernel, the compensated one, the collapsed one, Cole-Cole, Dias,
    Shin --, 32 and 33 walkers, 40 steps of 'de', of 'snooker' and of a three-way mixture with 'stretch': chain, stored
    log-probability and acceptance of the device run equal the replay's."""
    g = np.load(_case(prefix))
    ctx = make_ctx(g, model, variant)
    assert variant == 'auto' or ctx.variant == variant
    ndim = g['bounds'].shape[1]
    for W in (32, 33):
        if W < 2 * ndim:
            continue
        _replay_lone(ctx, _start(g, W, 500 + W))
    ctx.close()


def _ball(bounds, n, seed):
    """n starts in a small ball inside a PolynomialDecomposition box: r0 near 1, small coefficients."""
    rng = np.random.RandomState(seed)
    ndim = bounds.shape[1]
    centre = np.concatenate([[1.0], 1e-3 * rng.randn(ndim - 1)])
    p0 = centre + 1e-4 * rng.randn(n, ndim)
    assert np.all((p0 > bounds[0]) & (p0 < bounds[1]))
    return p0


@pytest.mark.parametrize('poly_deg,variant', [(4, 'reduced_comp'), (6, 'reduced_comp'), (7, 'reduced_comp'), (8, 'reduced_comp'),
                                              (10, 'reduced'), (10, 'reduced_comp')])
def test_reduced_kernels_whose_operands_overflow_the_scalar_registers_equal_their_replay(poly_deg, variant):
    """The QR-reduced functors whose kernel-argument operands no longer fit the scalar registers (the instantiations
    with scratch in the resource report: degree 10 plain; 4, 7, 8 compensated) and their neighbours, 33 walkers."""
    from test_gpu_parity import _pd_context
    ctx, bounds, *_ = _pd_context(32, poly_deg, 1.0, 0, variant=variant)
    assert ctx.variant == variant
    _replay_lone(ctx, _ball(bounds, 33, poly_deg), steps=24)
    ctx.close()


def test_chunks_continuation_and_thinning_of_a_device_run():
    """A lone Cole-Cole context, 33 walkers, the three-way mixture: chunk 7 against one chunk, run_mcmc(None, n) against
    one run, thin_by = 3 against every third sample -- and the replay of the thinned run."""
    from bisip_amd.sampler import DeviceEnsembleSampler
    g = np.load(_case('case16_'))
    ctx = make_ctx(g, 'PeltonColeCole')
    W, ndim = 33, g['bounds'].shape[1]
    p0 = _start(g, W, 9)

    def run(n, **kw):
        s = DeviceEnsembleSampler(W, ndim, ctx, rng='philox', seed=31, moves=THREE, **{k: v for k, v in kw.items() if k != 'thin'})
        s.run_mcmc(p0, n, thin_by=kw.get('thin', 1))
        return s
    whole = run(42)
    _same(run(42, chunk=7), whole)
    cont = run(30, chunk=7)
    cont.run_mcmc(None, 12)
    _same(cont, whole)
    thinned = run(14, thin=3, chunk=4)
    assert np.array_equal(thinned.get_chain(), whole.get_chain()[2::3])
    assert np.array_equal(thinned.get_log_prob(), whole.get_log_prob()[2::3])
    assert np.array_equal(thinned.acceptance_fraction, whole.acceptance_fraction)
    rep = DeviceEnsembleSampler(W, ndim, backend=DeviceDrawnBackend(ctx), rng='philox', seed=31, moves=THREE)
    rep.run_mcmc(p0, 14, thin_by=3)
    _same(thinned, rep)
    cont.reset()
    cont.run_mcmc(None, 3)
    assert cont.get_chain().shape == (3, W, ndim) and cont.acceptance_fraction.max() <= 1.0
    ctx.close()


def _replay_batch(ctx, E, Wp, p0, steps, distinct=True):
    """Every move on a batch context: the device run equals the replay; no ensemble reads a walker of another."""
    from bisip_amd.sampler import DeviceEnsembleSampler
    ndim = p0.shape[1]
    for name, moves in MOVES.items():
        dev = DeviceEnsembleSampler(Wp, ndim, ctx, rng='philox', seed=12, n_ensembles=E, moves=moves, chunk=16)
        dev.run_mcmc(p0, steps)
        rep = DeviceEnsembleSampler(Wp, ndim, backend=DeviceDrawnBackend(ctx, E), rng='philox', seed=12, n_ensembles=E, moves=moves)
        rep.run_mcmc(p0, steps)
        _same(dev, rep)
        assert dev.last_path == 'launch-per-half-step'
        assert 0.0 < dev.acceptance_fraction.mean() < 1.0, (name, dev.acceptance_fraction.mean())
        if distinct:
            chain = dev.get_chain().reshape(steps, E, Wp, ndim)
            assert len({chain[:, e].tobytes() for e in range(E)}) == E


def test_batch_of_different_spectra_equals_its_replay():
    """Three different spectra in one batch context, every move: 8 walkers each of a single Cole-Cole (halves of four,
    waves that straddle spectra), and 128 walkers each of a double Cole-Cole (every wave inside one spectrum -- the
    uniform operand path -- and several lanes per slot)."""
    import bisip_amd
    from test_gpu_modes import spectrum_files
    batch = _one_mode_batch(8)
    assert batch.ndim == 4
    lo, hi = batch.param_bounds
    p0 = np.random.RandomState(8).uniform(lo + 0.4 * (hi - lo), hi - 0.4 * (hi - lo), (3 * 8, 4))
    _replay_batch(batch.ctx, 3, 8, p0, 40)
    batch.close()
    batch = bisip_amd.SpectraBatch('PeltonColeCole', list(spectrum_files()), nwalkers=128, nsteps=1, n_modes=2)
    lo, hi = batch.param_bounds
    p0 = np.random.RandomState(9).uniform(lo + 0.4 * (hi - lo), hi - 0.4 * (hi - lo), (3 * 128, 7))
    _replay_batch(batch.ctx, 3, 128, p0, 16)
    batch.close()


def test_batch_on_a_tier_per_spectrum_equals_its_replay():
    """The compensated batch functor with and without its tier-per-spectrum pointer: 24 spectra of degree 5, c = 0.5 on
    'auto' run plain and compensated arithmetic inside one launch (tests/test_gpu_batch.py:
    test_every_spectrum_of_a_batch_runs_the_tier_its_own_context_would), at 128 walkers each (every wave inside one
    spectrum) and at 40 (waves that straddle two); then the same batch forced onto the compensated tier.  The guard is
    off: the replay must meet the context as the device run left it."""
    import bisip_amd
    from test_gpu_batch import _tables
    E = 24
    for Wp in (128, 40):
        batch = bisip_amd.SpectraBatch('PolynomialDecomposition', _tables(E, 20), nwalkers=Wp, nsteps=1, poly_deg=5, c_exp=0.5)
        ctx = batch.ctx
        ctx.reduced_guard(enable=False)
        tiers = ctx.reduced_tiers
        assert ctx.variant == 'reduced_comp' and tiers[0] >= 2 and tiers[1] >= 2, tiers
        rng = np.random.RandomState(Wp)
        centre = np.array([1.0, 0.005, -0.003, -0.001, 0.0005, 0.0002, 0.00001])
        p0 = (centre + 1e-4 * rng.randn(E, Wp, 7)).reshape(E * Wp, 7)
        _replay_batch(ctx, E, Wp, p0, 12)
        assert ctx.reduced_tiers == tiers
        ctx.set_variant('reduced_comp')
        assert ctx.reduced_tiers == (0, E)
        _replay_batch(ctx, E, Wp, p0, 12)
        batch.close()


@pytest.mark.parametrize('poly_deg,variant', [(6, 'reduced_comp'), (10, 'reduced')])
def test_batch_reduced_kernels_with_scratch_equal_their_replay(poly_deg, variant):
    """The two batch instantiations with scratch in the resource report (uniform operands: 128 walkers per spectrum)."""
    import bisip_amd
    from test_gpu_batch import _tables
    batch = bisip_amd.SpectraBatch('PolynomialDecomposition', _tables(2, 32), nwalkers=128, nsteps=1, poly_deg=poly_deg)
    batch.ctx.reduced_guard(enable=False)
    batch.ctx.set_variant(variant)
    assert batch.ctx.variant == variant
    _replay_batch(batch.ctx, 2, 128, _ball(batch.param_bounds, 2 * 128, poly_deg), 12)
    batch.close()


def test_survey_shape_equals_its_replay():
    """512 spectra x 256 walkers, the shape of the README's survey: 65,536 slots per half-step go out as four-wave
    workgroups, one lane per slot, every wave inside one spectrum.  Four steps of every move."""
    prob = ep.problem(8, 2)
    E, Wp = 512, 256
    batch = _batch(prob, E, Wp)
    batch.ctx.reduced_guard(enable=False)
    p0, _ = prob.exact_draws(E * Wp, np.random.RandomState(21))
    _replay_batch(batch.ctx, E, Wp, p0, 4, distinct=False)
    batch.close()


def test_a_mixture_that_is_all_stretch_is_the_stretch_sampler():
    from bisip_amd.sampler import DeviceEnsembleSampler
    g = np.load(_case('case16_'))
    ctx = make_ctx(g, 'PeltonColeCole')
    W, ndim = 33, g['bounds'].shape[1]
    p0 = _start(g, W, 4)
    plain = DeviceEnsembleSampler(W, ndim, ctx, rng='philox', seed=3, persistent=False)
    plain.run_mcmc(p0, 50, thin_by=2)
    mixed = DeviceEnsembleSampler(W, ndim, ctx, rng='philox', seed=3, moves=[('stretch', 0.3), ('stretch', 0.7)], chunk=11)
    mixed.run_mcmc(p0, 50, thin_by=2)
    assert plain.last_path == mixed.last_path == 'launch-per-half-step'
    _same(mixed, plain)
    ctx.close()
    batch = _one_mode_batch(8)
    p0 = np.random.RandomState(8).uniform(*batch.param_bounds, (3 * 8, 4))
    runs = []
    for kw in (dict(persistent=False), dict(moves='stretch')):
        runs.append(DeviceEnsembleSampler(8, 4, batch.ctx, rng='philox', seed=3, n_ensembles=3, **kw))
        runs[-1].run_mcmc(p0, 30)
    _same(*runs)
    batch.close()


# ---------------------------------------------------------------------------------------------------------------
# the exact posterior
# ---------------------------------------------------------------------------------------------------------------

def _run_batch(label, prob, E, W, steps, thin, moves, variant='auto', seed=1):
    from bisip_amd.sampler import DeviceEnsembleSampler
    batch = _batch(prob, E, W)
    ctx = batch.ctx
    if variant != 'auto':
        ctx.reduced_guard(enable=False)               # a forced formulation is the caller's: nothing may move it
        ctx.set_variant(variant)
    err = _check_logprob(ctx, prob, multiple_of=E)
    kernel = ctx.kernel_name
    if variant == 'auto':
        assert kernel in REDUCED, kernel
    else:
        assert kernel == 'k_logprob<PDCollapsed>' and ctx.variant == 'collapsed'
    p0, _ = prob.exact_draws(E * W, np.random.RandomState(2000 + seed))
    s = DeviceEnsembleSampler(W, prob.ndim, ctx, rng='philox', seed=seed, n_ensembles=E, moves=moves)
    s.run_mcmc(p0, steps // thin, thin_by=thin)
    assert s.last_path == 'launch-per-half-step' and s.last_stream == 'arrays'
    assert ctx.kernel_name == kernel and s.guard_['escalations'] == 0 and s.guard_['reruns'] == 0
    if variant == 'auto':
        assert s.guard_['checks'] >= 1                # the sampler measured the kernel on its own rows
    n = steps // thin
    chain = s.get_chain().reshape(n, E, W, prob.ndim)
    logp = s.get_log_prob().reshape(n, E, W)
    acc = s.acceptance_fraction.mean()
    batch.close()
    _judge(label, prob, chain, logp, E, f'; {kernel}, {s.last_path}, logp err {err:.1e}, acceptance {acc:.3f}')


EXACT_CASES = {
    'de-8-2': dict(shape=(8, 2), moves='de'),
    'snooker-8-2': dict(shape=(8, 2), moves='snooker'),
    'mixture-20-4': dict(shape=(20, 4), moves=MIXTURE),
    'three-20-6': dict(shape=(20, 6), moves=THREE),
    'mixture-cut-box': dict(shape='cut', moves=MIXTURE),
    'de-collapsed-20-4': dict(shape=(20, 4), moves='de', variant='collapsed'),
    # the smallest halves the moves take: two members for 'de', three for 'snooker'
    'de-smallest': dict(shape=(8, 0), moves='de', E=512, W=4),
    'snooker-smallest': dict(shape=(8, 0), moves='snooker', E=512, W=6),
}


@pytest.mark.parametrize('name', sorted(EXACT_CASES))
def test_batch_moves_have_the_exact_posterior(name):
    """E = 128 ensembles of W = 32 walkers (the smallest: 512 of 4 and of 6), 600 steps stored every 4, launch per
    half-step, every walker started at an exact draw: max|T| within ep.t_limit, the stored log-probability within 1e-10
    of the helper's, no two ensembles alike, the guard checked and escalated nothing (``_judge``)."""
    case = dict(EXACT_CASES[name])
    shape = case.pop('shape')
    prob = ep.truncated_problem() if shape == 'cut' else ep.problem(*shape)
    E, W = case.pop('E', 128), case.pop('W', 32)
    _run_batch(name, prob, E, W, 600, 4, seed=sorted(EXACT_CASES).index(name) + 1, **case)


def test_lone_spectrum_mixture_has_the_exact_posterior():
    """A single-spectrum context, 33 walkers (halves of 17 and 16), the 0.8 / 0.2 mixture: independence comes from
    R = 32 runs with seeds of their own.  (8, 2), 300 steps stored every 2."""
    from bisip_amd.sampler import DeviceEnsembleSampler
    prob = ep.problem(8, 2)
    R, W, steps, thin = 32, 33, 300, 2
    n = steps // thin
    ctx = _lone_context(prob)
    err = _check_logprob(ctx, prob)
    kernel = ctx.kernel_name
    assert kernel in REDUCED, kernel
    p0, _ = prob.exact_draws(R * W, np.random.RandomState(177))
    chain, logp = np.empty((n, R, W, prob.ndim)), np.empty((n, R, W))
    for r in range(R):
        s = DeviceEnsembleSampler(W, prob.ndim, ctx, rng='philox', seed=9100 + r, moves=MIXTURE)
        s.run_mcmc(p0[r * W:(r + 1) * W], n, thin_by=thin)
        assert s.last_path == 'launch-per-half-step' and s.guard_['escalations'] == 0 and s.guard_['checks'] >= 1
        chain[:, r], logp[:, r] = s.get_chain(), s.get_log_prob()
    assert ctx.kernel_name == kernel
    ctx.close()
    _judge('lone-mixture-33', prob, chain, logp, R, f'; {kernel}, logp err {err:.1e}')


# ---------------------------------------------------------------------------------------------------------------
# the guard of the QR-reduced tiers
# ---------------------------------------------------------------------------------------------------------------

def test_guard_sends_a_mixture_s_chunk_back_to_the_compensated_kernel(monkeypatch, tmp_path):
    """By the means of test_device_fit_never_keeps_a_chunk_of_a_failing_tier: the plain tier's estimate is let through on
    the worst-conditioned valley fixture and the walkers start on its shell rows.  Under the mixture the run ends on the
    compensated kernel, the chunk was run again on the same counters, and the chain is that of a run that sampled with
    the compensated kernel from the start, bit for bit."""
    import bisip_amd
    from bisip_amd.sampler import DeviceEnsembleSampler
    from bisip_amd.synthetic import write_spectrum_file
    g = _valley('valley06_')
    path = write_spectrum_file(str(tmp_path / 's.csv'), 64, 0)
    rows = g['theta'][np.all((g['bounds'][0] < g['theta']) & (g['theta'] < g['bounds'][1]), axis=1)]
    W = len(rows) - len(rows) % 2
    assert W >= 2 * rows.shape[1]
    p0 = np.ascontiguousarray(rows[:W])

    def model(variant):
        m = bisip_amd.PolynomialDecomposition(path, nwalkers=W, nsteps=120, poly_deg=9, c_exp=0.5, variant=variant)
        assert np.array_equal(m.data['w'], g['w']) and np.array_equal(m.data['zn'], g['zn'])     # the fixture's design
        return m
    m = model('auto')
    monkeypatch.setenv('BISIP_AUTO_ERR_MAX', '1e-6')
    ctx = m._context()
    monkeypatch.delenv('BISIP_AUTO_ERR_MAX')
    ctx.set_bounds(m.param_bounds)
    assert ctx.variant == 'reduced' and ctx.kernel_name == 'k_logprob_pd_reduced'
    s = DeviceEnsembleSampler(W, p0.shape[1], ctx, rng='philox', seed=5, moves=MIXTURE, chunk=40)
    s.run_mcmc(p0, 120)
    assert ctx.kernel_name == 'k_logprob_pd_reduced_comp' and ctx.variant == 'reduced_comp'
    assert s.guard_['escalations'] == 1 and s.guard_['reruns'] == 1 and s.guard_['checks'] >= 2
    ref_model = model('reduced_comp')
    ref_ctx = ref_model._context()
    ref_ctx.set_bounds(ref_model.param_bounds)
    ref = DeviceEnsembleSampler(W, p0.shape[1], ref_ctx, rng='philox', seed=5, moves=MIXTURE, chunk=40)
    ref.run_mcmc(p0, 120)
    assert ref.guard_['escalations'] == 0
    _same(s, ref)


# ---------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------

def test_fit_runs_the_moves_and_the_summaries_work_on_the_result():
    import bisip_amd
    from test_gpu_modes import WP, spectrum_files, starts
    m = bisip_amd.PeltonColeCole(spectrum_files()[0], n_modes=2, nwalkers=WP, nsteps=120)
    np.random.seed(31)
    m.fit(p0=starts(np.random.default_rng(4), (WP,)), moves=MIXTURE, chain='device')
    assert m.sampler.last_path == 'launch-per-half-step' and m.sampler.rng == 'philox'
    assert m.get_chain().shape == (120, WP, 7)
    assert m.get_param_mean(discard=40).shape == (7,) and np.isfinite(m.get_param_mean(discard=40)).all()
    assert m.get_summary(discard=40) is not None
    rate = m.get_mode_switch_rate(discard=40)
    assert rate.shape == (WP,) and np.all((rate >= 0) & (rate <= 1))
    assert 0.02 < m.sampler.acceptance_fraction.mean() < 0.98
    b = bisip_amd.SpectraBatch('PeltonColeCole', list(spectrum_files()), nwalkers=WP, nsteps=120, n_modes=2)
    b.fit(starts(np.random.default_rng(5), (3, WP)), seed=6, chain='device', moves='de')
    assert b._fitted().last_path == 'launch-per-half-step'
    assert b.get_param_mean(40).shape == (3, 7) and np.isfinite(b.get_param_mean(40)).all()
    assert b.get_summary(discard=40) is not None
    assert b.get_mode_switch_rate('log_tau', 40).shape == (3, WP)
    # the refusals, with their reasons
    ctx = m._context()
    from bisip_amd.sampler import DeviceEnsembleSampler
    for kw, text in ((dict(nwalkers=3, moves='de'), 'at least 4'), (dict(nwalkers=5, moves='snooker'), 'at least 6'),
                     (dict(moves='de', persistent=True), 'persistent'), (dict(moves='de', rng='numpy'), 'philox'),
                     (dict(moves='de', distributed=True), 'one rank'), (dict(moves='walk'), 'unknown move')):
        kw = dict(dict(nwalkers=WP, rng='philox'), **kw)
        with pytest.raises(ValueError, match=text):
            DeviceEnsembleSampler(kw.pop('nwalkers'), 7, ctx, **kw)
    with pytest.raises(ValueError, match='philox'):
        m.fit(moves='de', rng='numpy')
    with pytest.raises(ValueError, match='persistent'):
        b.fit(moves='de', persistent=True)
    b.close()


def test_library_refuses_halves_too_small_for_a_move():
    """bisip_move_half_dev: BISIP_EINVAL (ValueError) for 'de' on fewer than 4 walkers and 'snooker' on fewer than 6,
    before anything is launched."""
    import torch
    from bisip_amd import _hip
    g = np.load(_case('case16_'))
    ctx = make_ctx(g, 'PeltonColeCole')
    ndim = g['bounds'].shape[1]
    for W, kind, text in ((3, 1, 'at least 4'), (5, 2, 'at least 6'), (8, 7, 'unknown move kind')):
        coords = torch.from_numpy(_start(g, W, 1)).cuda()
        logp = torch.zeros(W, dtype=torch.float64, device='cuda')
        ints = torch.zeros(W, dtype=torch.int32, device='cuda')
        dbl = torch.zeros(W, dtype=torch.float64, device='cuda')
        a = _hip.MoveArgs()
        a.stretch.coords, a.stretch.logp, a.stretch.status = coords.data_ptr(), logp.data_ptr(), ints.data_ptr()
        a.stretch.n_slots = W // 2
        a.active = a.p0 = a.p1 = a.p2 = ints.data_ptr()
        a.gamma = a.logu = dbl.data_ptr()
        a.snooker_gamma = 1.7
        with pytest.raises(ValueError, match=text):
            ctx.move_half_dev(a, kind, W)
    torch.cuda.synchronize()
    ctx.close()
