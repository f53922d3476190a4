"""Every model shape a context can have -- PolynomialDecomposition of degree 0 ... 10, Cole-Cole with 1 ... 5 modes, Dias,
Shin -- through every host entry point that turns the shape into a kernel's template argument (csrc/host.h: with_model,
with_pd_degree; csrc/lp_build.h): log-probability and forward of a single spectrum and of a batch, the stretch move's
half-step and persistent kernels and the other moves' half-step kernels of both.  A wrong case in a dispatch launches a kernel of another degree without any error, so each
shape is held to invariants the neighbouring tests state for a few shapes only:

  * spectrum e of a batch context returns the bits of a context of that spectrum alone (test_gpu_batch.py);
  * the log-probabilities a device sampler stores are the bits ctx.logprob returns for the stored coordinates, from the
    persistent kernel and from one launch per half-step, single spectrum and batch (test_gpu_sampler.py, test_gpu_batch.py);
  * the per-frequency formulations agree with the oracle (test_gpu_parity.py).  The forced QR-reduced variants are held
    bit for bit to their host emulation in test_gpu_reduced_bits.py; their accuracy at high degree is the guard's
    business and is not measured here.

Eight frequencies (2N >= P + 2 at degree 10), 16 walkers, 6 steps.  16 walkers are fewer than twice the dimensions from
degree 7 and from three modes on, hence live_dangerously: the chains are compared, not believed."""
import numpy as np
import pytest

import oracle
from conftest import assert_logp_close, assert_Z_close
from test_gpu_response import MODEL_ID, inside

pytestmark = pytest.mark.gpu

N_FREQ, WALKERS, STEPS = 8, 16, 6
SPECTRA = (1, 2)                     # synthetic_columns indices of the batch's two spectra
MOVES = [('de', 1.0), ('snooker', 1.0), ('stretch', 1.0)]

PD = [('PolynomialDecomposition', dict(poly_deg=p)) for p in range(11)]
OTHERS = [('PeltonColeCole', dict(n_modes=d)) for d in range(1, 6)] + [('Dias2000', {}), ('Shin2015', {})]
CASES = [(m, kw, v) for m, kw in PD for v in ('collapsed', 'reduced', 'reduced_comp')] + [(m, kw, 'auto') for m, kw in OTHERS]
KERNEL = {'collapsed': 'k_logprob<PDCollapsed>', 'reduced': 'k_logprob_pd_reduced', 'reduced_comp': 'k_logprob_pd_reduced_comp',
          'PeltonColeCole': 'k_logprob<ColeCole>', 'Dias2000': 'k_logprob<Dias>', 'Shin2015': 'k_logprob<Shin>'}


def _case_id(v):
    if isinstance(v, dict):
        return '-'.join(f'{k}{x}' for k, x in v.items()) or None
    return v


def _options(b):
    if b.model == 'PolynomialDecomposition':
        return dict(poly_deg=b.poly_deg, c_exp=b.c_exp, taus=b.taus, log_taus=b.log_taus)
    if b.model == 'PeltonColeCole':
        return dict(n_modes=b.n_modes)
    return {}


def _force(ctx, variant, name):
    if variant != 'auto':
        ctx.set_variant(variant)
        ctx.reduced_guard(False)
    assert ctx.kernel_name == name, (ctx.kernel_name, name)


def _stored_logp_is_logprob(ctx, ndim, p0, n_ensembles):
    """The last stored row of log-probabilities against ctx.logprob of the last stored coordinates: both sampler paths of
    the stretch move, then the differential-evolution and snooker moves' half-steps (halves of eight: enough partners)."""
    from bisip_amd.sampler import DeviceEnsembleSampler
    for kw, path in ((dict(persistent=True), 'persistent'), (dict(persistent=False), 'launch-per-half-step'),
                     (dict(persistent=False, moves=MOVES), 'launch-per-half-step')):
        s = DeviceEnsembleSampler(WALKERS, ndim, ctx, rng='philox', seed=11, n_ensembles=n_ensembles, live_dangerously=True, **kw)
        s.run_mcmc(p0, STEPS)
        assert s.last_path == path, (s.last_path, path)
        last = np.ascontiguousarray(s.get_chain()[-1].reshape(-1, ndim))
        assert np.array_equal(ctx.logprob(last), s.get_log_prob()[-1].ravel()), (kw, n_ensembles)


@pytest.mark.parametrize('model,kw,variant', CASES, ids=_case_id)
def test_shape_through_every_dispatch(model, kw, variant):
    import bisip_amd
    from bisip_amd import _hip
    from bisip_amd.synthetic import synthetic_columns
    E = len(SPECTRA)
    name = KERNEL[variant] if model == 'PolynomialDecomposition' else KERNEL[model]
    batch = bisip_amd.SpectraBatch(model, [synthetic_columns(N_FREQ, i) for i in SPECTRA], nwalkers=WALKERS, nsteps=STEPS, **kw)
    _force(batch.ctx, variant, name)
    bounds = np.array(batch.param_bounds)
    lo, hi = bounds
    ndim = lo.size
    singles = []
    for e in range(E):
        singles.append(_hip.HipContext(MODEL_ID[model], batch.w[e], batch.zn[e], batch.zn_err[e], bounds, **_options(batch)))
        _force(singles[e], variant, name)

    # batch against single
    rng = np.random.RandomState(100 * ndim + len(variant))
    theta = rng.uniform(lo, hi, (E, WALKERS, ndim))
    if model == 'PolynomialDecomposition':
        theta[:, :WALKERS // 2, 1:] *= 1e-3          # a cloud where the fit is decent (small |logp|)
    got = batch.ctx.logprob(theta.reshape(-1, ndim)).reshape(E, WALKERS)
    alone = [singles[e].logprob(theta[e]) for e in range(E)]
    for e in range(E):
        assert np.array_equal(alone[e], got[e]), e

    # sampler against log-probability
    centre = inside(model, lo, hi, (E,), seed=ndim)
    p0 = centre[:, None, :] + 1e-4 * (hi - lo) * rng.standard_normal((E, WALKERS, ndim))
    _stored_logp_is_logprob(singles[0], ndim, p0[0], 1)
    _stored_logp_is_logprob(batch.ctx, ndim, p0.reshape(E * WALKERS, ndim), E)

    # the per-frequency formulations against the oracle
    if variant in ('collapsed', 'auto'):
        okw = _options(batch)
        okw.pop('poly_deg', None)
        prob = oracle.OracleProblem(model, batch.w[0], batch.zn[0], batch.zn_err[0], bounds, **okw)
        want_Z = oracle.forward(prob, theta[0, :8])
        errs = (assert_logp_close(alone[0], oracle.logprob(prob, theta[0])), assert_Z_close(singles[0].forward(theta[0, :8]), want_Z),
                assert_Z_close(batch.forward(theta[:, :8])[0], want_Z))
        print(f'{model} {kw}: logp, Z, batch Z within {errs[0]:.2e}, {errs[1]:.2e}, {errs[2]:.2e} (relative) of the oracle')

    for ctx in singles:
        ctx.close()
    batch.close()
