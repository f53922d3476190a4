"""Posterior mean and standard deviation on the device (bisip_chain_moments_dev), from the C entry point up to the model
and SpectraBatch methods.  Mean and std are held, bit for bit, to the summation order include/bisip_hip.h states
(bisip_amd.chainview.ordered_moments) and, against the long-double evaluation of np.mean / np.std, to the first-order
bound of any summation order that tests/moments_bounds.py derives and computes per case from the data."""
import numpy as np
import pytest

import fitted
from chain_harness import SENTINEL, GuardedCall, shape_id, store
from moments_bounds import (BOTH_INFINITIES, EXTREMES, SHAPES, assert_agrees_with_numpy, assert_same_bits,
                            assert_within_bounds, case, has_extremes, reference_and_bounds)

pytestmark = pytest.mark.gpu

ids = dict(ids=shape_id)


def run_abi(x, E, **storage):
    """One call on x (n, E * Wp, ndim) through store(x, **storage).  Outputs start as SENTINEL; the workspace holds exactly
    chain_moments_workspace() doubles; both are followed by guard values that must come back untouched."""
    import torch
    from bisip_amd import _hip
    from bisip_amd.chainview import moment_splits
    n, W, ndim = x.shape
    stored, offset, stride = store(x, **storage)
    t = torch.from_numpy(stored).cuda()
    call = GuardedCall()
    mean, std = call.out('the mean', (E, ndim)), call.out('the std', (E, ndim))
    doubles = _hip.chain_moments_workspace(n, E, ndim)
    assert doubles == E * moment_splits(n, E) * ndim                  # as large as the header says and no larger
    _hip.chain_moments_dev(t.data_ptr() + 8 * offset, n, stride, E, W // E, ndim, mean, std, call.work(8 * doubles),
                           call.stream)
    return call.finish()


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_entry_point(shape):
    n, E, Wp, ndim = shape
    c = case(*shape)
    x, ref = c['x'], c['ref']
    mean, std = run_abi(x, E)
    assert not (mean == SENTINEL).any() and not (std == SENTINEL).any()
    if c['ordered'] is not None:
        assert_same_bits(mean, c['ordered'][0], 'mean')
        assert_same_bits(std, c['ordered'][1], 'std')
    assert_agrees_with_numpy(mean, std, ref, c['ref_numpy'], c['np_mean'], c['np_std'], label=str(shape))
    worst = assert_within_bounds(mean, std, ref, label=str(shape))
    # parameter 0 has its centre at 0 and stays finite: it is held to the bound, and there the bound itself must be small,
    # else the inputs are wrong
    assert ref['checked'][:, 0].all()
    with np.errstate(all='ignore'):
        pos = ref['var'][:, 0] > 0
        rel = (ref['dvar'][:, 0] / ref['var'][:, 0])[pos]
    assert rel.size == 0 or rel.max() < 1e-9, float(rel.max())
    print(f'shape {shape}: error at most {worst:.3f} of its bound; {int(ref["checked"].sum())} of {E * ndim} held to it')
    if ndim > 1:
        assert mean[E - 1, ndim - 1] == 0.25 and std[E - 1, ndim - 1] == 0.0        # the constant parameter
    if has_extremes(E, ndim):
        e, q, _ = EXTREMES['tiny']
        assert ref['checked'][e, q] and 1e-141 < std[e, q] < 1e-139
        e, q, _ = EXTREMES['huge']
        assert std[e, q] == np.inf and np.isfinite(mean[e, q])
        e, q, _ = EXTREMES['vanishing']
        assert std[e, q] == 0.0 and mean[e, q] > 1e-300
        assert np.isnan(mean[BOTH_INFINITIES]) and np.isnan(std[BOTH_INFINITIES])
    # the same bits on a second call, and through other storage of the same used samples
    for kw in ({}, dict(discard=0, thin=1, pad=0), dict(discard=3, thin=4, pad=11)):
        m2, s2 = run_abi(x, E, **kw)
        assert same_bits(m2, mean) and same_bits(s2, std), kw


def test_three_quarters_of_the_columns_are_held_to_the_bound():
    """test_entry_point holds every ``checked`` (ensemble, parameter) to the bound; over its shapes they are the bulk."""
    checked = sum(int(case(*s)['ref']['checked'].sum()) for s in SHAPES)
    total = sum(s[1] * s[3] for s in SHAPES)
    assert 4 * checked >= 3 * total, (checked, total)


def test_refusals_leave_the_outputs_alone():
    import torch
    from bisip_amd import _hip
    n, E, Wp, ndim = 8, 2, 3, 4
    t = torch.zeros(n * E * Wp * ndim, dtype=torch.float64, device='cuda')
    mean = torch.full((E, 17), SENTINEL, dtype=torch.float64, device='cuda')           # (room for the ndim refused)
    std = torch.full((E, 17), SENTINEL, dtype=torch.float64, device='cuda')
    work = torch.zeros(4096, dtype=torch.float64, device='cuda')
    good = dict(d_chain_ptr=t.data_ptr(), n_samples=n, sample_stride=E * Wp * ndim, n_ensembles=E,
                walkers_per_ensemble=Wp, ndim=ndim, d_mean_ptr=mean.data_ptr(), d_std_ptr=std.data_ptr(),
                d_work_ptr=work.data_ptr())
    bad = [dict(d_chain_ptr=0), dict(d_mean_ptr=0), dict(d_std_ptr=0), dict(d_work_ptr=0), dict(ndim=0), dict(ndim=17),
           dict(n_samples=0), dict(n_ensembles=0), dict(walkers_per_ensemble=0), dict(n_ensembles=2 ** 31),
           dict(sample_stride=E * Wp * ndim - 1)]
    for change in bad:
        with pytest.raises(ValueError):
            _hip.chain_moments_dev(**dict(good, **change))
        torch.cuda.synchronize()
        assert (mean == SENTINEL).all() and (std == SENTINEL).all(), change
    _hip.chain_moments_dev(**good)                                   # and the call they were variations of is taken
    torch.cuda.synchronize()
    flat_mean, flat_std = mean.flatten(), std.flatten()              # (E, ndim) at the head of the buffers
    assert (flat_mean[:E * ndim] == 0.0).all() and (flat_std[:E * ndim] == 0.0).all()
    assert (flat_mean[E * ndim:] == SENTINEL).all() and (flat_std[E * ndim:] == SENTINEL).all()
    for shape in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (8, -2, 4)]:
        assert _hip.chain_moments_workspace(*shape) == 0
    assert _hip.chain_moments_workspace(8, 2, 4) == 2 * 2 * 4 and _hip.chain_moments_workspace(3, 2, 4) == 2 * 4


# -- through the layers ---------------------------------------------------------------------------------------------
def test_device_moments_of_a_view_with_offset_and_stride_and_of_a_derived_one():
    import torch
    from bisip_amd.chainview import ChainView, device_moments, ordered_moments
    n, E, Wp, ndim = 8, 5, 19, 13
    c = case(n, E, Wp, ndim)
    x = c['x']
    stored, offset, stride = store(x)
    view = ChainView(torch.from_numpy(stored).cuda(), n, E, Wp, ndim, offset=offset, stride=stride)
    mean, std = device_moments(view)
    assert_same_bits(mean, c['ordered'][0], 'mean')
    assert_same_bits(std, c['ordered'][1], 'std')
    # quantities derived row by row: another ndim on the same rows, contiguous
    y = np.ascontiguousarray(x[:, :, :3] * np.array([1.0, -2.0, 1e-3]))
    derived = view.derived(torch.from_numpy(y).cuda())
    assert (derived.n, derived.n_ensembles, derived.walkers_per_ensemble, derived.ndim) == (n, E, Wp, 3)
    mean, std = device_moments(derived)
    want = ordered_moments(y, E)
    assert_same_bits(mean, want[0], 'derived mean')
    assert_same_bits(std, want[1], 'derived std')
    assert_within_bounds(mean, std, reference_and_bounds(y, E), label='derived')


def check_methods(chain, E, mean, std, device):
    """chain (n, E * Wp, ndim) of get_chain: the methods' (E, ndim) results within the bound of the long-double
    reference (NumPy's, one rounding more, for a host chain), and with the stated order's bits when from the device."""
    from bisip_amd.chainview import ordered_moments
    ref = reference_and_bounds(chain, E, c=6 if device else 7)
    assert ref['checked'].all()
    assert_within_bounds(mean, std, ref)
    if device:
        want = ordered_moments(chain, E)
        assert_same_bits(mean, want[0], 'mean')
        assert_same_bits(std, want[1], 'std')


@pytest.mark.parametrize('where', ['device', 'host'])
def test_model_methods(where):
    m = fitted.fitted_model(where, nsteps=40)
    for kw in (dict(discard=10, thin=3), dict()):
        mean, std = m.get_param_mean(**kw), m.get_param_std(**kw)
        assert mean.shape == std.shape == (m.ndim,)
        check_methods(m.get_chain(**kw), 1, mean[None], std[None], where == 'device')


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
        mean, std = b.get_param_mean(**kw), b.get_param_std(**kw)
        assert mean.shape == std.shape == (E, b.ndim)
        chain = b.get_chain(**kw)                                    # (n, E, Wp, ndim)
        check_methods(chain.reshape(chain.shape[0], E * Wp, b.ndim), E, mean, std, where == 'device')
    b.close()


def test_mcse_mean_is_made_of_the_two_device_results():
    import torch
    from bisip_amd.chainview import ChainView, device_moments
    from bisip_amd.ess import device_ess, device_mcse_mean
    n, E, Wp, ndim = 12, 2, 33, 16
    x = case(n, E, Wp, ndim)['x']
    view = ChainView(torch.from_numpy(x.copy()).cuda(), n, E, Wp, ndim)
    N = n * Wp
    for split in (True, False):
        with np.errstate(all='ignore'):
            want = device_moments(view)[1] * np.sqrt(N / (N - 1.0)) / np.sqrt(device_ess(view, 'mean', split))
        got = device_mcse_mean(view, split)
        assert_same_bits(got, want, f'split={split}')
        fin = np.isfinite(got)
        assert 2 * fin.sum() > fin.size and (got[fin] >= 0).all()
