"""Effective sample size and rank-normalisation on the device (bisip_chain_ess_dev, bisip_chain_rank_normalize_dev)
against the NumPy definition (bisip_amd.ess), from the C entry points up to the model and SpectraBatch methods.

Tolerances: ``|got - want| <= 1e-10 * max(1, |want|)`` for every ESS, NaN exactly where the definition has it, and
``1e-14 * max(1, |z|)`` for the rank-normalised values -- one rank off by one moves z by more than 2 / N, so that also
proves the ranks, ties included.  Every case is held to the margin of tests/ess_cases.py: no decision of Geyer's sequence
within 1e-9 of zero (tests/test_ess.py checks that for the generated cases without a GPU)."""
import numpy as np
import pytest

import ess_cases as ec
from bisip_amd import ess as es
from chain_harness import SENTINEL, GuardedCall, used_window

pytestmark = pytest.mark.gpu


def on_device(case):
    """The stored chain of a COVER case on the device and how its used samples are read: ``(tensor, offset, stride)`` in
    doubles."""
    import torch
    E, Wp, ndim, n, discard, thin = case
    stored = ec.cover_case(*case)[0]
    offset, stride, used = used_window(stored.shape[0], stored.shape[1], discard, thin)
    assert used == n
    return torch.from_numpy(stored.copy()).cuda(), offset, stride


def run_rank(t, offset, stride, n, E, Wp, ndim):
    """One bisip_chain_rank_normalize_dev call; output and workspace are followed by guard values."""
    from bisip_amd import _hip
    nbytes = _hip.chain_rank_normalize_workspace(n, E, Wp, ndim)
    assert nbytes > 0
    call = GuardedCall()
    z = call.out('z', (n, E * Wp, ndim))
    _hip.chain_rank_normalize_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, z, call.work(nbytes), nbytes,
                                  call.stream)
    return call.finish()[0]


def run_ess(t, offset, stride, n, E, Wp, ndim, splits, thr=None):
    """One bisip_chain_ess_dev call: (E, ndim), or (len(thr), E, ndim) for thresholds (T, E, ndim)."""
    import torch
    from bisip_amd import _hip
    T = 0 if thr is None else thr.shape[0]
    nbytes = _hip.chain_ess_workspace(n, E, Wp, ndim, splits, T)
    assert nbytes > 0
    call = GuardedCall()
    out = call.out('the effective sample sizes', (max(1, T), E, ndim))
    d_thr = torch.from_numpy(np.ascontiguousarray(thr)).cuda() if T else None
    _hip.chain_ess_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, splits, d_thr.data_ptr() if T else 0, T,
                       out, call.work(nbytes), nbytes, call.stream)
    res = call.finish()[0]
    assert not (res == SENTINEL).any()
    return res if T else res[0]


def z_definition(used, E):
    Wp = used.shape[1] // E
    return np.concatenate([es.z_scale(used[:, e * Wp:(e + 1) * Wp]) for e in range(E)], axis=1)


@pytest.mark.parametrize('case', ec.COVER, ids=ec.cover_id)
def test_entry_points_on_the_covering_set(case):
    """Both entry points on every shape, the used samples taken by pointer offset and stride (what lies between is NaN)."""
    E, Wp, ndim, n = case[:4]
    t, offset, stride = on_device(case)
    used = ec.cover_case(*case)[1]
    z = run_rank(t, offset, stride, n, E, Wp, ndim)
    ec.assert_close(z, z_definition(used, E), ec.Z_RTOL, f'{case} z')
    for split in (True, False):
        want, gs, ge, lags = ec.cover_reference(case, 'mean', split)
        ec.assert_margins(gs, ge, (case, split))
        got = run_ess(t, offset, stride, n, E, Wp, ndim, 2 if split else 1)
        ec.assert_close(got, want, what=f'{case} split={split}')
        if n == 2001:                     # rho = 0 ends in the first block of lags, rho = 0.99 after more than one round
            assert lags[0, 0] <= 5 and lags[0, -1] > es.round_lags(n, E, Wp, ndim, split) + 64


@pytest.mark.parametrize('case', ec.THRESHOLD_COVER, ids=ec.cover_id)
def test_thresholded_mode_and_the_kinds(case):
    """n_threshold = 1, 2 and 4: the 5 % and 95 % quantiles, a threshold below and one above every sample (constant
    indicators: S), NaN thresholds; then 'bulk' and 'tail' as device_ess takes them, through the same offset and stride."""
    import torch
    from bisip_amd.chainview import ChainView
    E, Wp, ndim, n = case[:4]
    t, offset, stride = on_device(case)
    thr = ec.cover_thresholds(case)
    view = ChainView(t.reshape(-1), n, E, Wp, ndim, offset=offset, stride=stride)
    for split in (True, False):
        splits = 2 if split else 1
        want, gs, ge, _ = ec.cover_threshold_reference(case, split)
        ec.assert_margins(gs, ge, (case, split))
        ec.assert_close(run_ess(t, offset, stride, n, E, Wp, ndim, splits, thr[:1]), want[:1], what=f'{case} one threshold')
        ec.assert_close(run_ess(t, offset, stride, n, E, Wp, ndim, splits, thr[1:3]), want[1:3], what=f'{case} two')
        both = run_ess(t, offset, stride, n, E, Wp, ndim, splits, thr)
        ec.assert_close(both, want, what=f'{case} four thresholds')
        S = (n // 2 * 2 if split else n) * Wp
        assert np.all(both[2][~np.isnan(want[2])] == S) and np.all(both[3][~np.isnan(want[3])] == S)
        for kind in ('bulk', 'tail'):
            want, gs, ge, _ = ec.cover_reference(case, kind, split)
            ec.assert_margins(gs, ge, (case, kind, split))
            ec.assert_close(es.device_ess(view, kind, split), want, what=f'{case} {kind} split={split}')
    zv = es.device_rank_normalize(view)
    assert (zv.n, zv.n_ensembles, zv.walkers_per_ensemble, zv.ndim) == (n, E, Wp, ndim)
    ec.assert_close(zv.tensor.cpu().numpy(), z_definition(ec.cover_case(*case)[1], E), ec.Z_RTOL, f'{case} z of the view')
    del t, zv
    torch.cuda.empty_cache()


def test_hand_built_chain():
    """A constant walker among moving ones, a constant parameter (S), duplicated values, NaN / +inf / -inf planted: NaN
    for that (ensemble, parameter) only, in all three kinds; a NaN in the middle sample of an odd n is seen by the ranks
    and the quantiles, not by the 'mean' of the halves."""
    import torch
    from bisip_amd.chainview import ChainView
    x, nan_all, nan_ranked = ec.hand_built()
    n, W, ndim = x.shape
    E = nan_all.shape[0]
    Wp = W // E
    t = torch.from_numpy(x).cuda()
    view = ChainView(t, n, E, Wp, ndim)
    z = es.device_rank_normalize(view).tensor.cpu().numpy().reshape(n, E, Wp, ndim)
    np.testing.assert_array_equal(np.isnan(z).any(axis=(0, 2)), nan_ranked)
    np.testing.assert_array_equal(np.isnan(z).all(axis=(0, 2)), nan_ranked)
    ec.assert_close(z.reshape(n, W, ndim), z_definition(x, E), ec.Z_RTOL, 'hand-built z')
    for split in (True, False):
        for kind in es.KINDS:
            want, gs, ge, _ = ec.definition(x, E, kind, split)
            ec.assert_margins(gs, ge, (kind, split))
            np.testing.assert_array_equal(np.isnan(want), nan_all if kind == 'mean' and split else nan_ranked)
            got = es.device_ess(view, kind, split)
            ec.assert_close(got, want, what=f'hand-built {kind} split={split}')
            L = n // 2 if split else n
            assert got[E - 1, ndim - 1] == L * (2 if split else 1) * Wp          # the constant parameter: S exactly


def test_repeatable_to_the_bit():
    case = (3, 300, 7, 65, 1, 2)
    E, Wp, ndim, n = case[:4]
    t, offset, stride = on_device(case)
    thr = ec.cover_thresholds(case)[:2]
    for splits in (1, 2):
        a, b = (run_ess(t, offset, stride, n, E, Wp, ndim, splits) for _ in range(2))
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
        a, b = (run_ess(t, offset, stride, n, E, Wp, ndim, splits, thr) for _ in range(2))
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    a, b = (run_rank(t, offset, stride, n, E, Wp, ndim) for _ in range(2))
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


def test_refused_arguments():
    import torch
    from bisip_amd import _hip
    t = torch.zeros(1 << 16, dtype=torch.float64, device='cuda')
    p, nbytes = t.data_ptr(), 8 << 16
    for n, splits in [(3, 2), (1, 1), (0, 1), (8, 3), (8, 0)]:
        with pytest.raises(ValueError):
            _hip.chain_ess_dev(p, n, 8, 1, 4, 2, splits, 0, 0, p, p, nbytes, 0)
    with pytest.raises(ValueError, match='null'):
        _hip.chain_ess_dev(0, 8, 8, 1, 4, 2, 2, 0, 0, p, p, nbytes, 0)
    with pytest.raises(ValueError, match='sample_stride'):
        _hip.chain_ess_dev(p, 8, 7, 1, 4, 2, 2, 0, 0, p, p, nbytes, 0)
    with pytest.raises(ValueError, match='workspace'):
        _hip.chain_ess_dev(p, 8, 8, 1, 4, 2, 2, 0, 0, p, p, _hip.chain_ess_workspace(8, 1, 4, 2, 2) - 1, 0)
    with pytest.raises(ValueError, match='workspace'):
        _hip.chain_rank_normalize_dev(p, 8, 8, 1, 4, 2, p, p, _hip.chain_rank_normalize_workspace(8, 1, 4, 2) - 1, 0)
    with pytest.raises(ValueError, match='4 used samples'):
        es.ess(t[:3 * 4 * 2].reshape(3, 4, 2))
    with pytest.raises(ValueError, match='unflattened'):
        es.ess(t[:32].reshape(8, 4))


def test_ess_of_a_device_tensor():
    import torch
    x = ec.ar1(np.random.default_rng(5), 200, 6, [0.0, 0.6, 0.9])
    for kind in es.KINDS:
        for split in (True, False):
            got = es.ess(torch.from_numpy(x).cuda(), kind, split)
            want, gs, ge, _ = ec.definition(x, 1, kind, split)
            ec.assert_margins(gs, ge, (kind, split))
            assert got.shape == (3,)
            ec.assert_close(got, want[0], what=f'tensor {kind} split={split}')


# -- through the layers ---------------------------------------------------------------------------------------------
def check_against_definition(chain, lp, E, ess_of, mcse, lp_ess_of, label):
    """chain (n, E * Wp, ndim), lp (n, E * Wp): the methods' values against the definition at the tolerance above."""
    n, W, ndim = chain.shape
    for kind in es.KINDS:
        for split in (True, False):
            want, gs, ge, _ = ec.definition(chain, E, kind, split)
            ec.assert_margins(gs, ge, (label, kind, split))
            ec.assert_close(np.reshape(ess_of(kind, split), (E, ndim)), want, what=f'{label} {kind} split={split}')
            want, gs, ge, _ = ec.definition(lp[:, :, None], E, kind, split)
            ec.assert_margins(gs, ge, (label, 'log-probability', kind, split))
            ec.assert_close(np.reshape(lp_ess_of(kind, split), (E, 1)), want, what=f'{label} log-probability {kind} {split}')
    Wp = W // E
    want = np.stack([es.mcse_mean(chain[:, e * Wp:(e + 1) * Wp]) for e in range(E)])
    ec.assert_close(np.reshape(mcse, (E, ndim)), want, what=f'{label} mcse of the mean')


@pytest.mark.parametrize('cls_name,kw', [('PolynomialDecomposition', dict(poly_deg=3)), ('PeltonColeCole', dict(n_modes=1))])
def test_model_methods(cls_name, kw):
    import bisip_amd
    m = getattr(bisip_amd, cls_name)(bisip_amd.DataFiles()['SIP-K389175'], nwalkers=32, nsteps=400, **kw)
    np.random.seed(4)
    m.fit(chain='device')
    assert m._sampler.chain_on_device
    for used in (dict(discard=100, thin=3), dict(discard=200)):
        chain, lp = m.get_chain(**used), m._sampler.get_log_prob(**used)
        assert m.get_ess(**used).shape == (m.ndim,) and isinstance(m.get_log_prob_ess(**used), float)
        np.testing.assert_array_equal(m.get_ess(**used), m.get_ess('bulk', split=True, **used))
        check_against_definition(chain, lp, 1, lambda kind, split: m.get_ess(kind, split=split, **used),
                                 m.get_mcse_mean(**used), lambda kind, split: m.get_log_prob_ess(kind, split=split, **used),
                                 f'{cls_name} {used}')
    with pytest.raises(ValueError, match='no samples'):
        m.get_ess(discard=400)
    with pytest.raises(ValueError, match='4 used samples'):
        m.get_ess(discard=397)
    with pytest.raises(ValueError, match='unflattened'):
        m.get_ess(chain=m.get_chain(flat=True))


@pytest.mark.parametrize('where', ['device', 'host'])
def test_spectra_batch_methods(where):
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    spectra = [bisip_amd.DataFiles()['SIP-K389175']] + [synthetic_columns(20, i) for i in range(2)]
    E, Wp = 3, 64
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=Wp, nsteps=300, poly_deg=2)
    np.random.seed(5)
    b.fit(seed=11, chain=where)
    for used in (dict(discard=100), dict(discard=60, thin=2)):
        chain, lp = b.get_chain(**used), b.get_log_prob(**used)          # (n, E, Wp, ndim), (n, E, Wp)
        n = chain.shape[0]
        assert b.get_ess(**used).shape == (E, b.ndim) and b.get_log_prob_ess(**used).shape == (E,)
        assert b.get_mcse_mean(**used).shape == (E, b.ndim)
        check_against_definition(chain.reshape(n, E * Wp, b.ndim), lp.reshape(n, E * Wp), E,
                                 lambda kind, split: b.get_ess(kind, split=split, **used), b.get_mcse_mean(**used),
                                 lambda kind, split: b.get_log_prob_ess(kind, split=split, **used), f'batch {where} {used}')
    got = b.get_ess('tail', discard=100)
    np.testing.assert_array_equal(b.gather(got), got)                   # one rank: its own block
    with pytest.raises(ValueError, match='no samples'):
        b.get_ess(discard=300)
    b.close()
