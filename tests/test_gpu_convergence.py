"""Per-walker moments and R-hat on the device (bisip_chain_rhat_dev), from the C entry point up to the model and
SpectraBatch methods.  Mean, variance and R-hat are held, bit for bit, to the summation order include/bisip_hip.h
states (bisip_amd.convergence.ordered_rhat) and, against the long-double evaluation of the definitions, to the
first-order bound of any summation order that tests/convergence_bounds.py derives and computes per case from the data."""
import functools

import numpy as np
import pytest

import fitted
from chain_harness import SENTINEL, GuardedCall, assert_same_bits, shape_id, store
from convergence_bounds import assert_within_bounds, hand_built_chain, reference_and_bounds

pytestmark = pytest.mark.gpu

# (n, E, Wp, ndim).  Small columns counts are cut into segments of 32 samples (convergence.segment_plan): n = 64, 65 have
# halves of one segment, 66 and 67 of two (the second of one sample), 129 and 130 of two and three.  (9, 256, 3, 2) is the
# first ensemble count that takes the one-kernel path without workspace, (9, 255, 3, 2) the last that does not;
# (5, 256, 128, 16) is the largest ensemble that path takes (4096 chain moments in LDS); (4, 1, 100, 3) has 300 columns:
# no multiple of the 256-column tile.
SHAPES = [(4, 1, 2, 1), (5, 3, 2, 2), (7, 2, 63, 7), (7, 2, 64, 7), (7, 2, 65, 7), (6, 5, 9, 3), (4, 1, 257, 16),
          (4, 1, 100, 3), (64, 1, 5, 3), (65, 1, 5, 3), (66, 1, 5, 3), (67, 1, 5, 3), (129, 2, 3, 2), (130, 2, 3, 2),
          (9, 255, 3, 2), (9, 256, 3, 2), (5, 256, 128, 16), (5000, 1, 32, 7), (600, 64, 64, 7)]


@functools.lru_cache(maxsize=None)
def case(n, E, Wp, ndim):
    """(store() of the chain, used chain (n, E * Wp, ndim), {split: (ordered mean, var, rhat)}, {split: reference and
    bounds})"""
    from bisip_amd import convergence as cv
    x, centre, width = hand_built_chain(n, E, Wp, ndim)
    stored = store(x)
    ordered = {s: cv.ordered_rhat(x, s, n_ensembles=E) for s in (True, False)}
    ref = {s: reference_and_bounds(x, E, s) for s in (True, False)}
    x.setflags(write=False)
    return stored, x, ordered, ref


def run_abi(stored, n, E, Wp, ndim, splits, mean=True, var=True, rhat=True):
    """One call; outputs not asked for stay SENTINEL.  Outputs and workspace are followed by guard values."""
    import torch
    from bisip_amd import _hip
    samples, offset, stride = stored
    t = torch.from_numpy(samples).cuda()
    call = GuardedCall()
    m = call.out('the mean', (splits, E, Wp, ndim), asked=mean)
    v = call.out('the variance', (splits, E, Wp, ndim), asked=var)
    r = call.out('R-hat', (E, ndim), asked=rhat)
    nbytes = _hip.chain_rhat_workspace(n, E, Wp, ndim, splits)
    _hip.chain_rhat_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, splits, m, v, r, call.work(nbytes), nbytes,
                        call.stream)
    return (*call.finish(), nbytes)


@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_entry_point(shape):
    from bisip_amd import convergence as cv
    n, E, Wp, ndim = shape
    stored, x, ordered, refs = case(*shape)
    for split in (True, False):
        splits = 2 if split else 1
        L = n // 2 if split else n
        m, v, r, nbytes = run_abi(stored, n, E, Wp, ndim, splits)
        assert not (m == SENTINEL).any() and not (v == SENTINEL).any() and not (r == SENTINEL).any()
        if shape == (5000, 1, 32, 7):
            assert cv.segment_plan(L, E * Wp * ndim, splits)[1] > 1          # the quickstart is cut into segments
        if E >= 256:
            assert nbytes == 0
        om, ov, orh = ordered[split]
        assert_same_bits(m, om, 'mean')
        assert_same_bits(v, ov, 'var')
        assert_same_bits(r, orh, 'rhat')
        ref = refs[split]
        worst = assert_within_bounds(m, v, r, ref, label=f'{shape} split={split}')
        # parameter 0 has its centre at 0: there the bound itself must be small, else the inputs are wrong
        with np.errstate(all='ignore'):
            fin = np.isfinite(ref['rhat'][:, 0].astype(np.float64))
            rel_r = (ref['drhat'][:, 0] / ref['rhat'][:, 0])[fin]
            pos = ref['var'][..., 0] > 0
            rel_v = (ref['dvar'][..., 0] / ref['var'][..., 0])[pos]
        assert fin.any() and pos.any()
        assert rel_r.max() < 1e-9 and rel_v.max() < 1e-9, (float(rel_r.max()), float(rel_v.max()))
        print(f'shape {shape} split={split}: error at most {worst:.3f} of its bound; bound on R-hat {float(rel_r.max()):.1e}, '
              f'on the variance {float(rel_v.max()):.1e} relative; workspace {nbytes} bytes')
        # the constant walker: variance exactly 0, mean exactly its value; the constant parameter: NaN
        assert (v[:, 0, Wp - 1, 0] == 0.0).all() and (m[:, 0, Wp - 1, 0] == 0.25).all()
        if ndim > 1:
            assert np.isnan(r[E - 1, ndim - 1])
        assert np.isfinite(r[:, 0]).all()


@pytest.mark.parametrize('shape', [(7, 2, 65, 7), (67, 1, 5, 3), (9, 256, 3, 2)], ids=shape_id)
def test_null_outputs_and_repeat(shape):
    """Every combination of outputs gives the bits of the full call and leaves the others alone; twice the same bits."""
    n, E, Wp, ndim = shape
    stored, x, ordered, _ = case(*shape)
    for splits in (1, 2):
        full = run_abi(stored, n, E, Wp, ndim, splits)[:3]
        for k in range(1, 8):
            ask = [bool(k & 1), bool(k & 2), bool(k & 4)]
            got = run_abi(stored, n, E, Wp, ndim, splits, *ask)[:3]
            for a, g, f in zip(ask, got, full):
                if a:
                    np.testing.assert_array_equal(g.view(np.uint64), f.view(np.uint64))
                else:
                    assert (g == SENTINEL).all()


def test_refused_shapes():
    import torch
    from bisip_amd import _hip
    t = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = t.data_ptr()
    for n, Wp, splits in [(3, 4, 2), (1, 4, 1), (2, 1, 1), (0, 4, 1)]:
        with pytest.raises(ValueError):
            _hip.chain_rhat_dev(p, n, Wp * 2, 1, Wp, 2, splits, p, p, p, p, 4096 * 8, 0)
    with pytest.raises(ValueError, match='none of'):
        _hip.chain_rhat_dev(p, 4, 8, 1, 4, 2, 2, 0, 0, 0, p, 4096 * 8, 0)


def test_rhat_of_a_device_tensor():
    import torch
    from bisip_amd import convergence as cv
    x = np.random.default_rng(5).normal(size=(40, 6, 3))
    for split in (True, False):
        got = cv.rhat(torch.from_numpy(x).cuda(), split)
        assert got.shape == (3,)
        np.testing.assert_array_equal(got, cv.ordered_rhat(x, split)[2][0])
        np.testing.assert_allclose(got, cv.rhat(x, split), rtol=1e-12)


# -- through the layers ---------------------------------------------------------------------------------------------
def check_against_definitions(chain, lp, rhat_of, mean, std, lp_rhat_of, E):
    """chain (n, E * Wp, ndim), lp (n, E * Wp): the methods' values within the bound of the long-double definitions."""
    n, W, ndim = chain.shape
    Wp = W // E
    for split in (True, False):
        ref = reference_and_bounds(chain, E, split)
        assert_within_bounds(None, None, rhat_of(split).reshape(E, ndim), ref)
        refl = reference_and_bounds(lp[:, :, None], E, split)
        assert_within_bounds(None, None, np.asarray(lp_rhat_of(split), dtype=np.float64).reshape(E, 1), refl)
    ref = reference_and_bounds(chain, E, False)
    var = std.reshape(1, E, Wp, ndim) ** 2
    assert_within_bounds(mean.reshape(1, E, Wp, ndim), None, None, ref)
    # std = sqrt(var): |d(std^2)| <= dvar + 4 u var
    assert (np.abs(var - ref['var']) <= ref['dvar'] + 4 * 2.0 ** -53 * ref['var']).all()


@pytest.mark.parametrize('where', ['device', 'host'])
def test_model_methods(where):
    m = fitted.fitted_model(where, nsteps=40)
    for kw in (dict(discard=10, thin=3), dict()):
        chain, lp = m.get_chain(**kw), m._sampler.get_log_prob(**kw)
        assert m.get_rhat(**kw).shape == (m.ndim,) and m.get_walker_mean(**kw).shape == (32, m.ndim)
        assert isinstance(m.get_log_prob_rhat(**kw), float)
        check_against_definitions(chain, lp, lambda s: m.get_rhat(split=s, **kw), m.get_walker_mean(**kw),
                                  m.get_walker_std(**kw), lambda s: m.get_log_prob_rhat(split=s, **kw), 1)
    with pytest.raises(ValueError, match='no samples'):
        m.get_rhat(discard=40)
    with pytest.raises(ValueError, match='2 per chain'):
        m.get_rhat(discard=37)
    with pytest.raises(TypeError, match='flat'):
        m.get_walker_mean(flat=True)


@pytest.mark.parametrize('where', ['device', 'host'])
def test_spectra_batch_methods(where):
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    spectra = [bisip_amd.DataFiles()['SIP-K389175']] + [synthetic_columns(20, i) for i in range(2)]
    E, Wp = 3, 16
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=Wp, nsteps=30, poly_deg=2)
    np.random.seed(5)
    b.fit(seed=11, chain=where)
    for kw in (dict(), dict(discard=7, thin=2)):
        chain, lp = b.get_chain(**kw), b.get_log_prob(**kw)          # (n, E, Wp, ndim), (n, E, Wp)
        n = chain.shape[0]
        assert b.get_rhat(**kw).shape == (E, b.ndim) and b.get_log_prob_rhat(**kw).shape == (E,)
        assert b.get_walker_mean(**kw).shape == b.get_walker_std(**kw).shape == (E, Wp, b.ndim)
        check_against_definitions(chain.reshape(n, E * Wp, b.ndim), lp.reshape(n, E * Wp),
                                  lambda s: b.get_rhat(split=s, **kw), b.get_walker_mean(**kw), b.get_walker_std(**kw),
                                  lambda s: b.get_log_prob_rhat(split=s, **kw), E)
    with pytest.raises(ValueError, match='no samples'):
        b.get_rhat(discard=30)
    b.close()
