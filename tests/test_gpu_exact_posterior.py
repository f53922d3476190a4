"""The stretch-move samplers on the device against a posterior that is drawn exactly (tests/exact_posterior.py).

Every case: the context's log-probability is first held to the helper's closed form (1e-10, -inf rows exact); then every
walker of E independent ensembles -- a batch of E copies of one spectrum, or R lone runs with seeds of their own --
starts at an exact draw, so the ensemble is stationary from step 0 and every stored sample has the posterior's
expectations exactly.  T = (mean over ensembles - reference mean) / standard error, for the coordinates, the second
moments about the reference mean and the three indicators logp >= q10 / q50 / q90, is held to the Student-t quantile
``t_limit`` at a family-wise 1e-3 per case: no per-case constant, seeds fixed here.  A wrong power of z, a proposal
density other than 1/sqrt(z) or an acceptance rule that treats a prior face wrongly fails this by a factor of several
(tests/test_exact_posterior.py measures 28 .. 34 against a limit of 4.3 at a quarter of this size).

A case that fails is not given another seed: rerun it with three more seeds and four times the steps and record the four
T -- a bias grows like the square root of the samples, a fluke does not -- and look for the cause in the NumPy statement
of the contract and the bitwise replay tests."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_posterior as ep
from conftest import assert_logp_close

pytestmark = pytest.mark.gpu

REDUCED = ('k_logprob_pd_reduced', 'k_logprob_pd_reduced_comp')


def _check_logprob(ctx, prob, multiple_of=1):
    """ctx.logprob == the helper's logp on 512 exact draws and on rows on either side of every face."""
    rng = np.random.RandomState(5)
    draws, _ = prob.exact_draws(512, rng)
    inside, outside = ep.face_rows(prob, rng)
    rows = np.concatenate([draws, inside, outside])
    pad = -rows.shape[0] % multiple_of                # a batch context takes the same number of rows for every spectrum
    if pad:
        rows = np.concatenate([rows, prob.exact_draws(pad, rng)[0]])
    want = prob.logp(rows)
    assert np.isfinite(want[:512 + inside.shape[0]]).all()
    assert np.isneginf(want[512 + inside.shape[0]:512 + 2 * inside.shape[0]]).all()
    return assert_logp_close(ctx.logprob(rows), want, 1e-10)


def _judge(label, prob, chain, logp, n_independent, extra=''):
    """max|T| <= t_limit for the chain's features and for the indicators of the STORED log-probability; the stored
    log-probability is the one of the stored position; no two ensembles ran the same chain."""
    ref = ep.reference(prob)
    n, E, W, ndim = chain.shape
    assert E == n_independent and logp.shape == (n, E, W)
    assert chain.nbytes <= 64 << 20
    assert np.isfinite(logp).all()                    # no sample ever sits on or outside a face
    assert len({chain[:, e].tobytes() for e in range(E)}) == E
    own = prob.logp(chain)
    assert np.max(np.abs(own - logp) / np.maximum(1.0, np.abs(own))) <= 1e-10
    limit = ep.t_limit(E, ref['mean'].size)
    T = prob.t_statistics(chain, ref, logp=own)
    T_stored = prob.t_statistics_logp(logp, ref)
    worst, where = ep.worst(T, ref['names'])
    worst_stored, where_stored = ep.worst(T_stored, ref['names'][-3:])
    print(f'\n{label}: max|T| = {worst:.2f} at {where}; stored logp: {worst_stored:.2f} at {where_stored}; '
          f'limit {limit:.2f} ({E} x {W} walkers, {n} samples){extra}')
    assert worst <= limit, (label, worst, where, limit)
    assert worst_stored <= limit, (label, worst_stored, where_stored, limit)


def _batch(prob, E, W):
    """E copies of the spectrum in one batch context, under the problem's box."""
    import bisip_amd
    batch = bisip_amd.SpectraBatch('PolynomialDecomposition', [prob.table] * E, nwalkers=W, nsteps=1,
                                   poly_deg=prob.poly_deg, c_exp=prob.c_exp)
    # the helper's operands are the batch's
    assert np.array_equal(batch.w[E - 1], prob.w) and np.array_equal(batch.zn[E - 1], prob.zn)
    assert np.array_equal(batch.zn_err[E - 1], prob.zn_err) and np.array_equal(batch.log_taus, prob.log_taus)
    for name, lo, hi in zip(batch.param_names, prob.lo, prob.hi):
        batch.params[name] = [float(lo), float(hi)]
    assert np.array_equal(batch.param_bounds, prob.bounds)
    batch.ctx.set_bounds(batch.param_bounds)
    return batch


def _run_batch(label, prob, E, W, steps, thin, a=2.0, persistent=True, variant='auto', seed=1):
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
    p0, _ = prob.exact_draws(E * W, np.random.RandomState(1000 + seed))
    s = DeviceEnsembleSampler(W, prob.ndim, ctx, a=a, rng='philox', seed=seed, n_ensembles=E, persistent=persistent)
    s.run_mcmc(p0, steps // thin, thin_by=thin)
    assert s.last_path == ('persistent' if persistent else 'launch-per-half-step')
    assert s.last_stream == 'arrays'
    # the kernel named above is the one that sampled: nothing escalated on the way
    assert ctx.kernel_name == kernel and s.guard_['escalations'] == 0 and s.guard_['reruns'] == 0
    if variant == 'auto':
        assert s.guard_['checks'] >= 1                # ... and the sampler measured it on its own rows
    n = steps // thin
    chain = s.get_chain().reshape(n, E, W, prob.ndim)
    logp = s.get_log_prob().reshape(n, E, W)
    acc = s.acceptance_fraction.mean()
    batch.close()
    _judge(label, prob, chain, logp, E, f'; {kernel}, {s.last_path}, logp err {err:.1e}, acceptance {acc:.3f}')


BATCH_CASES = {
    # the four shapes (ndim 2, 4, 6, 8) on the persistent path, variant 'auto'
    'shape-8-0': dict(shape=(8, 0)),
    'shape-8-2': dict(shape=(8, 2)),
    'shape-20-4': dict(shape=(20, 4)),
    'shape-20-6': dict(shape=(20, 6)),
    'launches-8-2': dict(shape=(8, 2), persistent=False),
    # halves of two walkers
    'smallest-ensemble': dict(shape=(8, 0), E=512, W=4),
    # three faces moved into the posterior: -inf proposals and the strict inequalities
    'cut-box': dict(shape='cut'),
    'a-1.5': dict(shape=(8, 2), a=1.5),
    # the per-frequency formulation must sample the same law as the QR-reduced one 'auto' chose above
    'collapsed-20-4': dict(shape=(20, 4), variant='collapsed'),
}


@pytest.mark.parametrize('name', sorted(BATCH_CASES))
def test_batch_sampler_has_the_exact_posterior(name):
    """E = 128 ensembles of W = 32 walkers (the smallest ensemble: 512 of 4), rng='philox', 600 steps stored every 4."""
    case = dict(BATCH_CASES[name])
    shape = case.pop('shape')
    prob = ep.truncated_problem() if shape == 'cut' else ep.problem(*shape)
    E, W = case.pop('E', 128), case.pop('W', 32)
    _run_batch(name, prob, E, W, 600, 4, seed=sorted(BATCH_CASES).index(name) + 1, **case)


def _lone_context(prob):
    from bisip_amd import _hip
    return _hip.HipContext(_hip.MODEL_POLYDECOMP, prob.w, prob.zn, prob.zn_err, prob.bounds, poly_deg=prob.poly_deg,
                           c_exp=prob.c_exp, taus=prob.taus, log_taus=prob.log_taus)


@pytest.mark.parametrize('rng,W', [('numpy', 32), ('philox', 33)])
def test_lone_spectrum_sampler_has_the_exact_posterior(rng, W):
    """A single-spectrum context, launch per half-step: independence comes from R = 32 runs with seeds of their own.
    'numpy': the host-ordered MT19937 stream; 'philox' with 33 walkers: halves of 17 and 16.  (8, 2), 300 steps
    stored every 2."""
    from bisip_amd.sampler import DeviceEnsembleSampler
    prob = ep.problem(8, 2)
    R, steps, thin = 32, 300, 2
    n = steps // thin
    ctx = _lone_context(prob)
    err = _check_logprob(ctx, prob)
    kernel = ctx.kernel_name
    assert kernel in REDUCED, kernel
    p0, _ = prob.exact_draws(R * W, np.random.RandomState(77 + W))
    chain, logp = np.empty((n, R, W, prob.ndim)), np.empty((n, R, W))
    state = np.random.get_state()
    try:
        for r in range(R):
            np.random.seed(4000 + r)                  # rng='numpy': the sampler's stream starts from the global state
            s = DeviceEnsembleSampler(W, prob.ndim, ctx, rng=rng, seed=9000 + r, persistent=False)
            s.run_mcmc(p0[r * W:(r + 1) * W], n, thin_by=thin)
            assert s.last_path == 'launch-per-half-step' and s.guard_['escalations'] == 0
            assert rng == 'philox' or s.last_stream == 'host'
            chain[:, r], logp[:, r] = s.get_chain(), s.get_log_prob()
    finally:
        np.random.set_state(state)
    assert ctx.kernel_name == kernel
    ctx.close()
    _judge(f'lone-{rng}-{W}', prob, chain, logp, R, f'; {kernel}, logp err {err:.1e}')
