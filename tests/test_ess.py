"""The effective sample size and its pieces (bisip_amd.ess) without a GPU: the NumPy definition against known answers and
hand-built inputs, the condition on the inputs of tests/test_gpu_ess.py, and the plumbing."""
import os
import re
import statistics

import numpy as np
import pytest

import ess_cases as ec
from bisip_amd import ess as es
from bisip_amd.autocorr import _acf
from fitted import fitted_on_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- ndtri ----------------------------------------------------------------------------------------------------------------
def test_ndtri_against_python_inv_cdf():
    """statistics.NormalDist.inv_cdf is the same algorithm (AS 241, PPND16); all three branches, down to 1e-300."""
    central = np.linspace(0.0751, 0.9249, 2001)                   # |p - 0.5| <= 0.425
    mid = np.concatenate([10.0 ** np.linspace(-10.8, -1.13, 500), [0.0749, 1.4e-11]])      # r = sqrt(-log p) <= 5
    far = 10.0 ** np.linspace(-300.0, -10.9, 800)                 # r > 5
    assert np.all(np.abs(central - 0.5) <= 0.425) and np.all(np.abs(mid - 0.5) > 0.425)
    assert np.all(np.sqrt(-np.log(mid)) <= 5.0) and np.all(np.sqrt(-np.log(far)) > 5.0)
    nd = statistics.NormalDist()
    edges = np.array([0.075, 0.925, 0.5 - 0.425, 0.5 + 0.425, np.exp(-25.0), np.nextafter(np.exp(-25.0), 1.0)])
    for p in (central, mid, far, 1.0 - mid, 1.0 - 10.0 ** np.linspace(-15.9, -10.9, 200), edges):
        assert np.all((p > 0.0) & (p < 1.0))
        want = np.array([nd.inv_cdf(float(v)) for v in p])
        got = es.ndtri(p)
        assert np.all(np.abs(got - want) <= 1e-14 * np.maximum(1.0, np.abs(want))), float(np.max(np.abs(got - want)))
    assert es.ndtri(0.5) == 0.0 and es.ndtri(0.0) == -np.inf and es.ndtri(1.0) == np.inf
    assert np.isnan(es.ndtri([np.nan, -0.1, 1.1])).all()
    assert abs(es.ndtri(0.975) - 1.959963984540054) < 1e-14


# -- z_scale --------------------------------------------------------------------------------------------------------------
def test_z_scale_of_a_hand_worked_column_with_ties():
    #        value: 3    1    3    2    1    3     ranks of the sorted column 1 1 2 3 3 3: 1.5 1.5 3 5 5 5
    col = np.array([3.0, 1.0, 3.0, 2.0, 1.0, 3.0])
    ranks = np.array([5.0, 1.5, 5.0, 3.0, 1.5, 5.0])
    nd = statistics.NormalDist()
    want = np.array([nd.inv_cdf((r - 0.375) / 6.25) for r in ranks])
    x = np.stack([col, -col, np.arange(6.0)], axis=1).reshape(3, 2, 3)       # (n, W, ndim): rows k * W + w
    z = es.z_scale(x).reshape(6, 3)
    np.testing.assert_allclose(z[:, 0], want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(z[:, 1], -want, rtol=0, atol=1e-15)            # the ranks mirrored: 7 - r
    assert np.all(np.diff(z[:, 2]) > 0) and abs(z[:, 2].sum()) < 1e-14
    # -0.0 and 0.0 are one value; a value that is not finite takes the whole parameter, and only it
    assert es.z_scale(np.array([0.0, -0.0]).reshape(2, 1, 1)).ravel().tolist() == [0.0, 0.0]
    x[1, 1, 1] = np.inf
    z = es.z_scale(x)
    assert np.isnan(z[:, :, 1]).all() and np.isfinite(z[:, :, [0, 2]]).all()
    with pytest.raises(ValueError, match='unflattened'):
        es.z_scale(np.zeros((4, 2)))


# -- autocov --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,M', [(2, 1), (7, 3), (64, 5), (257, 2)])
def test_autocov_against_the_fft_form(L, M):
    c = ec.ar1(np.random.default_rng(L), L, M, [0.8], ties=False)[:, :, 0]
    a = es.autocov(c)
    assert a.shape == (L, M)
    y = c - c.mean(axis=0)
    np.testing.assert_allclose(a[0], (y * y).sum(axis=0) / L, rtol=1e-14)
    fft = _acf(c) * a[0]                                         # emcee's form divides by lag 0
    assert np.all(np.abs(a - fft) <= 1e-12 * a[0])


# -- ess_of_chains on hand-built inputs -------------------------------------------------------------------------------------
def test_constant_and_not_finite():
    assert es.ess_of_chains(np.full((10, 4), 0.25)) == 40.0
    assert es.ess_of_chains(np.full((10, 4), 0.25) + 1e-16 * np.arange(4)) == 40.0      # within the resolution
    c = np.random.default_rng(0).normal(size=(10, 4))
    for bad in (np.nan, np.inf, -np.inf):
        d = c.copy()
        d[3, 2] = bad
        assert np.isnan(es.ess_of_chains(d))
    assert es.ess_of_chains(c, margins=True)[0] == es.ess_of_chains(c)
    with pytest.raises(ValueError, match='2 samples'):
        es.ess_of_chains(np.zeros((1, 4)))


@pytest.mark.parametrize('n', [4, 5, 7])
def test_shortest_chains_give_the_floor(n):
    """Halves of 2 and 3 samples: the sequence never starts (max_t = -1), tau = 0 and the floor 1 / log10(S) decides."""
    x = np.random.default_rng(n).normal(size=(n, 3, 2))
    S = (n // 2) * 6
    for kind in ('mean', 'bulk'):
        np.testing.assert_allclose(es.ess(x, kind), S * np.log10(S), rtol=1e-14)
    for got in es.ess(x, 'tail'):                               # (an indicator may be constant over the halves: S)
        assert got == S or abs(got / (S * np.log10(S)) - 1.0) < 1e-14


def test_antithetic_chain_is_capped_by_the_floor():
    L, M = 200, 4
    c = np.where(np.arange(L)[:, None] % 2 == 0, 1.0, -1.0) + 1e-3 * np.random.default_rng(1).normal(size=(L, M))
    got = es.ess_of_chains(c)
    S = L * M
    assert got > S
    np.testing.assert_allclose(got, S * np.log10(S), rtol=1e-14)


def test_walkers_that_disagree_cost_samples():
    rng = np.random.default_rng(2)
    w = rng.normal(size=(500, 1))
    alone = es.ess_of_chains(w)
    assert alone > 300
    two = np.concatenate([w, rng.normal(size=(500, 1)) + 5.0], axis=1)
    assert es.ess_of_chains(two) < 0.05 * alone                  # the between-chain term bites
    same = np.concatenate([w, rng.normal(size=(500, 1))], axis=1)
    assert es.ess_of_chains(same) > alone


def test_odd_n_drops_the_middle_sample_from_the_chains_only():
    x = ec.ar1(np.random.default_rng(3), 41, 4, [0.5, 0.5], ties=False)
    moved = x.copy()
    moved[20] += 100.0                                           # the middle sample of every walker
    np.testing.assert_array_equal(es.ess(moved, 'mean'), es.ess(x, 'mean'))
    assert not np.array_equal(es.ess(moved, 'bulk'), es.ess(x, 'bulk'))      # it takes part in the ranking
    moved[20, 0, 0] = np.nan
    assert np.isfinite(es.ess(moved, 'mean')).all()
    assert np.isnan(es.ess(moved, 'bulk')[0]) and np.isnan(es.ess(moved, 'tail')[0]) and np.isfinite(es.ess(moved, 'bulk')[1])


def test_shapes_are_refused():
    with pytest.raises(ValueError, match='4 used samples'):
        es.ess(np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match='2 per chain'):
        es.ess(np.zeros((1, 4, 2)), split=False)
    with pytest.raises(ValueError, match='unflattened'):
        es.ess(np.zeros((40, 2)))
    with pytest.raises(ValueError, match='kind'):
        es.ess(np.zeros((8, 4, 2)), kind='median')
    assert es.ess(np.random.default_rng(0).normal(size=(2, 1, 1)), 'mean', split=False).shape == (1,)    # one chain of 2


# -- known answers ------------------------------------------------------------------------------------------------------------
# Seeds 0 and 1 are the first two tried: the definition alone gives 0.98 ... 1.04 of the theory with them, inside the 15 %
# the estimator is good for at these sizes.
def test_known_answers_iid_and_ar1():
    x = np.random.default_rng(0).normal(size=(1000, 8, 1))
    for kind in ('mean', 'bulk'):
        got = es.ess(x, kind)[0]
        assert abs(got / 8000.0 - 1.0) < 0.15, (kind, got)
    rho = 0.7
    x = ec.ar1(np.random.default_rng(1), 400, 256, [rho], ties=False)
    theory = 400 * 256 * (1 - rho) / (1 + rho)
    got = {kind: es.ess(x, kind)[0] for kind in es.KINDS}
    for kind in ('mean', 'bulk'):
        assert abs(got[kind] / theory - 1.0) < 0.15, (kind, got[kind], theory)
    assert got['tail'] > got['bulk']                             # an indicator series mixes faster than the value
    sd = np.std(x.reshape(-1), ddof=1)
    np.testing.assert_allclose(es.mcse_mean(x), [sd / np.sqrt(got['mean'])], rtol=1e-14)


# -- the condition on the inputs of the GPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.COVER, ids=ec.cover_id)
def test_cover_cases_sit_on_no_rounding_tie(case):
    E, Wp, ndim, n = case[:4]
    for split in (True, False):
        val, gs, ge, lags = ec.cover_reference(case, 'mean', split)
        assert val.shape == (E, ndim) and np.isfinite(val).all()
        ec.assert_margins(gs, ge, (case, split))
        if n == 2001:                                           # rho = 0 stops at once, rho = 0.99 outruns a round of lags
            Lr = es.round_lags(n, E, Wp, ndim, split)
            assert lags[0, 0] <= 5 and lags[0, -1] > Lr + 64 and Lr < n // 2, (lags[0], Lr)


@pytest.mark.parametrize('case', ec.THRESHOLD_COVER, ids=ec.cover_id)
def test_threshold_cases_sit_on_no_rounding_tie(case):
    E, Wp, ndim, n = case[:4]
    for split in (True, False):
        val, gs, ge, _ = ec.cover_threshold_reference(case, split)
        ec.assert_margins(gs, ge, (case, split))
        S = (n // 2 * 2 if split else n) * Wp
        want_nan = np.zeros((4, E, ndim), dtype=bool)
        want_nan[0, E - 1, ndim - 1] = want_nan[3, 0, 0] = True
        np.testing.assert_array_equal(np.isnan(val), want_nan)
        assert np.all(val[2:][~want_nan[2:]] == S)              # below and above every sample: constant indicators
        for kind in ('bulk', 'tail'):
            _, gs, ge, _ = ec.cover_reference(case, kind, split)
            ec.assert_margins(gs, ge, (case, kind, split))


def test_hand_built_chain_by_the_definition():
    x, nan_all, nan_ranked = ec.hand_built()
    E, ndim = nan_all.shape
    Wp = x.shape[1] // E
    for split in (True, False):
        for kind in es.KINDS:
            val, gs, ge, _ = ec.definition(x, E, kind, split)
            ec.assert_margins(gs, ge, (kind, split))
            want_nan = nan_all if kind == 'mean' and split else nan_ranked
            np.testing.assert_array_equal(np.isnan(val), want_nan, err_msg=f'{kind} {split}')
            for e in range(E):
                np.testing.assert_array_equal(val[e], es.ess(x[:, e * Wp:(e + 1) * Wp], kind, split))
            L = x.shape[0] // 2 if split else x.shape[0]
            assert val[E - 1, ndim - 1] == L * (2 if split else 1) * Wp      # the constant parameter: S


# -- plumbing ---------------------------------------------------------------------------------------------------------------
NAMES = ('bisip_chain_ess_dev', 'bisip_chain_ess_workspace', 'bisip_chain_rank_normalize_dev',
         'bisip_chain_rank_normalize_workspace')


def test_entry_points_exist(hip_lib):
    from __graft_entry__ import header_abi_version
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    for name in NAMES:
        assert hasattr(hip_lib, name)
        assert re.search(r'\b%s\(' % name, header)
        assert re.search(r'\b%s;' % name, exports)
        assert callable(getattr(_hip, name[len('bisip_'):]))
    assert hip_lib.bisip_abi_version() == header_abi_version() == 6          # symbols were only added


def a256(x):
    return (x + 255) // 256 * 256


def test_workspaces():
    from bisip_amd import _hip
    # the rank pass: two copies of the columns and the sort's scratch, as include/bisip_hip.h states
    for n, E, Wp, ndim in [(500, 8, 256, 7), (5, 3, 2, 2), (1, 1, 1, 1)]:
        items = n * E * Wp * ndim
        want = 2 * a256(8 * items) + a256(a256(8 * items) + 16 * E * ndim + 65536)
        assert _hip.chain_rank_normalize_workspace(n, E, Wp, ndim) == want
    for bad in ((0, 1, 8, 3), (4, 0, 8, 3), (4, 1, 0, 3), (4, 1, 8, 17), (4, 1, 8, 0), (1 << 31, 1, 8, 3), (1 << 16, 1 << 11, 1, 16)):
        assert _hip.chain_rank_normalize_workspace(*bad) == 0, bad
    # the ESS: three doubles per series, the round's lags per series and per (pair, chain group), the scan's state
    for n, E, Wp, ndim, split, T in [(500, 512, 256, 7, True, 0), (2001, 1, 300, 16, False, 0), (65, 3, 300, 7, True, 2),
                                     (4, 1, 1, 1, True, 0), (1000, 1, 2, 1, False, 8)]:
        Z, C, P = max(1, T) * (2 if split else 1), E * Wp * ndim, max(1, T) * E * ndim
        Lr, G = es.round_lags(n, E, Wp, ndim, split, T), -(-(2 if split else 1) * Wp // 256)
        want = 3 * a256(8 * Z * C) + a256(8 * Z * C * Lr) + a256(8 * P * G * Lr) + a256(64 * P) + a256(8 * P) + a256(4 * P)
        assert _hip.chain_ess_workspace(n, E, Wp, ndim, 2 if split else 1, T) == want, (n, E, Wp, ndim, split, T)
    assert es.round_lags(500, 512, 256, 7) == 64 and es.round_lags(5000, 1, 32, 7) == 2560 and es.round_lags(4, 1, 2, 1) == 64
    base = _hip.chain_ess_workspace(500, 512, 256, 7, 2)
    assert 0 < base < _hip.chain_ess_workspace(500, 512, 256, 7, 2, 2)
    assert _hip.chain_ess_workspace(4, 1, 1, 1, 2) > 0 and _hip.chain_ess_workspace(2, 1, 1, 1, 1) > 0
    for bad in ((3, 1, 8, 3, 2), (1, 1, 8, 3, 1), (4, 0, 8, 3, 2), (4, 1, 0, 3, 2), (4, 1, 8, 17, 2), (4, 1, 8, 0, 2),
                (4, 1, 8, 3, 3), (4, 1, 8, 3, 0), (4, 1, 8, 3, 2, 9), (4, 1, 8, 3, 2, -1)):
        assert _hip.chain_ess_workspace(*bad) == 0, bad


def test_entry_points_check_their_arguments():
    from bisip_amd import _hip
    # the pointers are never dereferenced: every call below is refused on the host
    ok = dict(chain=4096, n=8, stride=8 * 3, E=1, Wp=8, ndim=3, splits=2, thr=0, T=0, out=4096, work=4096, nbytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        _hip.chain_ess_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['splits'], a['thr'], a['T'],
                           a['out'], a['work'], a['nbytes'], 0)

    for name in ('chain', 'out', 'work'):
        with pytest.raises(ValueError, match='null'):
            call(**{name: 0})
    with pytest.raises(ValueError, match='ndim'):
        call(ndim=17, stride=8 * 17)
    with pytest.raises(ValueError, match='splits'):
        call(splits=3)
    with pytest.raises(ValueError, match='n_threshold'):
        call(T=1)                                               # thresholds counted, none given
    with pytest.raises(ValueError, match='n_threshold'):
        call(thr=4096, T=0)
    with pytest.raises(ValueError, match='n_threshold'):
        call(thr=4096, T=9)
    with pytest.raises(ValueError, match='2 samples'):
        call(n=3)
    with pytest.raises(ValueError, match='bad chain shape'):
        call(E=0)
    with pytest.raises(ValueError, match='sample_stride'):
        call(stride=23)
    with pytest.raises(ValueError, match='workspace'):
        call(nbytes=_hip.chain_ess_workspace(8, 1, 8, 3, 2) - 1)

    def rank(**kw):
        a = dict(ok, **kw)
        _hip.chain_rank_normalize_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['out'], a['work'],
                                      a['nbytes'], 0)

    for name in ('chain', 'out', 'work'):
        with pytest.raises(ValueError, match='null'):
            rank(**{name: 0})
    with pytest.raises(ValueError, match='ndim'):
        rank(ndim=0)
    with pytest.raises(ValueError, match='bad chain shape'):
        rank(Wp=0)
    with pytest.raises(ValueError, match='sample_stride'):
        rank(stride=23)
    with pytest.raises(RuntimeError, match='2\\^31'):
        rank(n=1 << 20, E=1 << 10, stride=(1 << 10) * 8 * 3)
    with pytest.raises(ValueError, match='workspace'):
        rank(nbytes=_hip.chain_rank_normalize_workspace(8, 1, 8, 3) - 1)


@pytest.mark.parametrize('kw', [dict(), dict(discard=11, thin=3)])
def test_inversion_methods_with_the_host_sampler(kw):
    m = fitted_on_host(60)
    chain, lp = m.get_chain(**kw), m._sampler.get_log_prob(**kw)
    for kind in es.KINDS:
        for split in (True, False):
            want = es.ess(chain, kind, split)
            assert want.shape == (4,) and np.isfinite(want).all()
            np.testing.assert_array_equal(m.get_ess(kind, split=split, **kw), want)
            np.testing.assert_array_equal(m.get_ess(kind, chain=chain, split=split), want)
            got = m.get_log_prob_ess(kind, split=split, **kw)
            assert isinstance(got, float) and got == es.ess(lp[:, :, None], kind, split)[0]
    np.testing.assert_array_equal(m.get_ess(**kw), es.ess(chain, 'bulk', True))          # the defaults
    np.testing.assert_array_equal(m.get_mcse_mean(**kw), es.mcse_mean(chain))
    np.testing.assert_array_equal(m.get_mcse_mean(chain=chain), es.mcse_mean(chain))
    want = np.std(chain.reshape(-1, 4), axis=0, ddof=1) / np.sqrt(es.ess(chain, 'mean'))
    np.testing.assert_allclose(m.get_mcse_mean(**kw), want, rtol=1e-15)


@pytest.mark.parametrize('method', ['get_ess', 'get_mcse_mean', 'get_log_prob_ess'])
def test_inversion_refusals(method):
    m = fitted_on_host(60)
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=60)
    with pytest.raises(TypeError, match='flat'):
        f(flat=True)
    with pytest.raises(TypeError, match='unexpected keyword'):
        f(bins=3)
    with pytest.raises(ValueError, match='4 used samples'):
        f(discard=57)                                           # 3 used samples: halves of one
    if method != 'get_log_prob_ess':
        with pytest.raises(ValueError, match='unflattened'):
            f(chain=m.get_chain(flat=True))                     # an explicit 2-D chain
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=m.get_chain(), discard=5)
    if method != 'get_mcse_mean':
        with pytest.raises(ValueError, match='kind'):
            f(kind='median')


class _HostChainSampler:
    """What SpectraBatch asks of its sampler, answered from a host chain (n, E, Wp, ndim) by the definitions."""

    def __init__(self, chain, lp):
        self.chain, self.lp = chain, lp

    def param_ess(self, kind='bulk', discard=0, thin=1, split=True):
        c = self.chain[discard + thin - 1::thin]
        return np.stack([es.ess(c[:, e], kind, split) for e in range(c.shape[1])])

    def param_mcse_mean(self, discard=0, thin=1):
        c = self.chain[discard + thin - 1::thin]
        return np.stack([es.mcse_mean(c[:, e]) for e in range(c.shape[1])])

    def log_prob_ess(self, kind='bulk', discard=0, thin=1, split=True):
        lp = self.lp[discard + thin - 1::thin]
        return np.stack([es.ess(lp[:, e, :, None], kind, split)[0] for e in range(lp.shape[1])])


def test_spectra_batch_methods_on_a_host_chain():
    from bisip_amd.batch import SpectraBatch
    rng = np.random.default_rng(8)
    chain, lp = rng.normal(size=(30, 3, 6, 4)), rng.normal(size=(30, 3, 6))
    b = SpectraBatch.__new__(SpectraBatch)
    b._fitted = lambda: _HostChainSampler(chain, lp)
    kw = dict(discard=4, thin=2)
    used = chain[5::2]
    assert b.get_ess(**kw).shape == (3, 4) and b.get_mcse_mean(**kw).shape == (3, 4)
    np.testing.assert_array_equal(b.get_ess('tail', split=False, **kw)[1], es.ess(used[:, 1], 'tail', split=False))
    np.testing.assert_array_equal(b.get_ess(**kw)[2], es.ess(used[:, 2], 'bulk'))
    assert b.get_log_prob_ess('mean', **kw).shape == (3,)
