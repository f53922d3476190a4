"""bisip_amd.convergence on the host: the definitions of the per-walker moments and the (split) Gelman-Rubin R-hat
against independent arithmetic, their NaN / inf rules, their behaviour on seeded chains, the NumPy restatement of the
device's summation order, and the methods of every model and of SpectraBatch on host chains."""
import os
import re

import numpy as np
import pytest

from bisip_amd import convergence as cv
from convergence_bounds import LD, assert_within_bounds, hand_built_chain, reference_and_bounds
from fitted import fitted_on_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rhat_ld(x, split=True):
    """R-hat in long double, written out from the formulas (no call into the module)."""
    x = np.asarray(x, dtype=LD)
    n = x.shape[0]
    if split:
        h = n // 2
        x = np.concatenate([x[:h], x[n - h:]], axis=1)
    L = x.shape[0]
    m = x.sum(axis=0) / L
    v = ((x - m) ** 2).sum(axis=0) / (L - 1)
    Wn = v.sum(axis=0) / v.shape[0]
    Bn = ((m - m.sum(axis=0) / m.shape[0]) ** 2).sum(axis=0) / (m.shape[0] - 1)
    return np.sqrt(LD(L - 1) / LD(L) + Bn / Wn)


# -- the definitions ------------------------------------------------------------------------------------------------
def test_hand_computed_case():
    """4 samples, 2 walkers, 1 parameter.  Split: chains (1, 3), (2, 2), (5, 7), (4, 8); means 2, 2, 6, 6; variances 2, 0,
    2, 8.  Wn = 3, Bn = var(2, 2, 6, 6) = 16 / 3, L = 2: R-hat = sqrt(1 / 2 + 16 / 9).  Unsplit: chains (1, 3, 5, 7) and
    (2, 2, 4, 8): means 4, 4; variances 20 / 3, 8; Bn = 0: R-hat = sqrt(3 / 4)."""
    x = np.array([[1.0, 2.0], [3.0, 2.0], [5.0, 4.0], [7.0, 8.0]])[:, :, None]
    c = cv.split_chains(x)
    assert c.shape == (2, 4, 1)
    np.testing.assert_array_equal(c[:, :, 0], [[1, 2, 5, 4], [3, 2, 7, 8]])
    mean, var = cv.walker_moments(c)
    np.testing.assert_array_equal(mean[:, 0], [2, 2, 6, 6])
    np.testing.assert_array_equal(var[:, 0], [2, 0, 2, 8])
    np.testing.assert_allclose(cv.gelman_rubin(mean, var, 2), [np.sqrt(0.5 + 16.0 / 9.0)], rtol=1e-15)
    np.testing.assert_allclose(cv.rhat(x), [np.sqrt(0.5 + 16.0 / 9.0)], rtol=1e-15)
    np.testing.assert_allclose(cv.rhat(x, split=False), [np.sqrt(0.75)], rtol=1e-15)
    mean, var = cv.walker_moments(x)
    np.testing.assert_array_equal(mean[:, 0], [4, 4])
    np.testing.assert_allclose(var[:, 0], [20.0 / 3.0, 8.0], rtol=1e-15)


@pytest.mark.parametrize('shape', [(4, 2, 1), (9, 5, 3), (50, 8, 7), (51, 3, 2)])
@pytest.mark.parametrize('split', [True, False])
def test_definitions_against_long_double(shape, split):
    rng = np.random.default_rng(sum(shape))
    x = rng.normal(size=shape) * 10.0 ** rng.integers(-3, 3, shape[2]) + rng.normal(size=shape[1:])
    np.testing.assert_allclose(cv.rhat(x, split), rhat_ld(x, split).astype(np.float64), rtol=1e-12)
    mean, var = cv.walker_moments(x)
    assert mean.shape == var.shape == shape[1:]
    xl = x.astype(LD)
    np.testing.assert_allclose(mean, (xl.sum(axis=0) / shape[0]).astype(np.float64), rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(var, (((xl - xl.mean(axis=0)) ** 2).sum(axis=0) / (shape[0] - 1)).astype(np.float64), rtol=1e-12)


def test_odd_n_drops_the_middle_sample():
    x = np.random.default_rng(2).normal(size=(7, 3, 2))
    c = cv.split_chains(x)
    assert c.shape == (3, 6, 2)
    np.testing.assert_array_equal(c[:, :3], x[:3])
    np.testing.assert_array_equal(c[:, 3:], x[4:])
    y = x.copy()
    y[3] = 1e9                                           # the middle sample belongs to neither half
    np.testing.assert_array_equal(cv.rhat(y), cv.rhat(x))
    assert cv.split_chains(x, split=False) is x
    assert cv.rhat(x, split=False).shape == (2,)


def test_value_errors():
    rng = np.random.default_rng(3)
    with pytest.raises(ValueError, match='2 per chain'):
        cv.split_chains(rng.normal(size=(3, 4, 2)))             # halves of one sample
    with pytest.raises(ValueError, match='2 per chain'):
        cv.split_chains(rng.normal(size=(1, 4, 2)), split=False)
    with pytest.raises(ValueError, match='2 chains'):
        cv.split_chains(rng.normal(size=(5, 1, 2)), split=False)
    assert cv.split_chains(rng.normal(size=(4, 1, 2))).shape == (2, 2, 2)      # one walker, two halves
    with pytest.raises(ValueError, match='unflattened'):
        cv.rhat(rng.normal(size=(10, 3)))
    with pytest.raises(ValueError, match='2 per chain'):
        cv.rhat(rng.normal(size=(3, 4, 2)))
    with pytest.raises(ValueError, match='2 per chain'):
        cv.ordered_rhat(rng.normal(size=(3, 4, 2)))
    with pytest.raises(ValueError, match='2 chains'):
        cv.ordered_rhat(rng.normal(size=(4, 1, 2)), split=False)
    with pytest.raises(ValueError, match='divide'):
        cv.ordered_rhat(rng.normal(size=(4, 5, 2)), n_ensembles=2)


# -- NaN / inf ------------------------------------------------------------------------------------------------------
def test_nan_and_inf_rules():
    x = np.random.default_rng(4).normal(size=(10, 4, 3))
    x[:, :, 2] = 0.25                                    # an all-constant parameter: 0 / 0
    x[:, 1, 0] = 0.25                                    # one constant walker among moving ones
    r = cv.rhat(x)
    assert np.isnan(r[2]) and np.isfinite(r[:2]).all()
    mean, var = cv.walker_moments(x)
    assert var[1, 0] == 0.0 and mean[1, 0] == 0.25
    assert np.isinf(cv.gelman_rubin(np.array([[0.0], [1.0]]), np.zeros((2, 1)), 5))[0]      # only Wn is 0
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 2, 1] = bad
        r = cv.rhat(y)
        assert not np.isfinite(r[1]) and np.isfinite(r[0])
        mean, var = cv.walker_moments(y)
        assert not np.isfinite(var[2, 1]) and np.isfinite(np.delete(var[:, 1], 2)).all()
        o = cv.ordered_rhat(y)
        assert not np.isfinite(o[2][0, 1]) and np.isfinite(o[2][0, 0]) and np.isnan(o[2][0, 2])


# -- known behaviour on seeded chains -----------------------------------------------------------------------------
def test_behaviour_on_seeded_chains():
    """The spread of R-hat over i.i.d. normal walkers is taken from the definition itself (200 seeds, written out in
    long double here), not from a constant; the module's value is that definition's."""
    n, W, seeds = 400, 64, 200
    iid = np.empty(seeds)
    for s in range(seeds):
        x = np.random.default_rng(s).normal(size=(n, W, 1))
        iid[s] = rhat_ld(x)[0]
        np.testing.assert_allclose(cv.rhat(x)[0], iid[s], rtol=1e-13)
    lo, hi = iid.min(), iid.max()
    print(f'i.i.d. split R-hat over {seeds} seeds: {lo:.5f} ... {hi:.5f}')
    assert lo >= np.sqrt((n // 2 - 1) / (n // 2)) and hi > lo          # Bn / Wn >= 0: R-hat cannot go below sqrt((L - 1) / L)
    # one walker of 32 moved by 10 sigma: above the i.i.d. value of every seed
    for s in range(5):
        x = np.random.default_rng(1000 + s).normal(size=(n, 32, 1))
        x[:, 5, 0] += 10.0
        assert cv.rhat(x)[0] > hi and cv.rhat(x, split=False)[0] > hi
    # a drift of 1 sigma over the run: the split form sees it, the unsplit one essentially does not
    for s in range(5):
        x = np.random.default_rng(2000 + s).normal(size=(n, W, 1))
        base_split, base_whole = cv.rhat(x)[0], cv.rhat(x, split=False)[0]
        y = x + np.linspace(0.0, 1.0, n)[:, None, None]
        assert cv.rhat(y)[0] > hi and cv.rhat(y)[0] > base_split + 0.02
        assert abs(cv.rhat(y, split=False)[0] - base_whole) < 5e-3


# -- the device's order, restated -----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(4, 1, 2, 1), (5, 3, 2, 2), (7, 2, 65, 7), (67, 1, 5, 3), (200, 2, 9, 3)])
@pytest.mark.parametrize('split', [True, False])
def test_ordered_rhat_against_the_definition(shape, split):
    n, E, Wp, ndim = shape
    x, _, _ = hand_built_chain(*shape)
    mean, var, r = cv.ordered_rhat(x, split, n_ensembles=E)
    splits = 2 if split else 1
    assert mean.shape == var.shape == (splits, E, Wp, ndim) and r.shape == (E, ndim)
    ref = reference_and_bounds(x, E, split)
    worst = assert_within_bounds(mean, var, r, ref, label=str(shape))
    print(f'{shape} split={split}: error at most {worst:.3f} of its bound')
    # and the definitions in float64 agree with it where all is finite
    for e in range(E):
        xe = x[:, e * Wp:(e + 1) * Wp]
        want = cv.rhat(xe, split)
        fin = np.isfinite(want)
        np.testing.assert_array_equal(np.isfinite(r[e]), fin)
        np.testing.assert_allclose(r[e][fin], want[fin], rtol=1e-7)


def test_segment_plan():
    assert cv.segment_plan(250, 512 * 256 * 7, 2) == (250, 1)          # a survey: one segment per half
    assert cv.segment_plan(100, 32768 * 7, 2) == (100, 1)
    seg, nseg = cv.segment_plan(2500, 32 * 7, 2)                       # the quickstart: cut to fill the chip
    assert seg == 32 and nseg == 79
    assert cv.segment_plan(32, 10, 2) == (32, 1) and cv.segment_plan(33, 10, 2) == (32, 2)
    assert cv.segment_plan(300, 64 * 64 * 7, 2) == (75, 4)


# -- plumbing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(discard=5, thin=3)])
def test_inversion_methods_with_the_host_sampler(kw):
    m = fitted_on_host()
    chain = m.get_chain(**kw)
    for split in (True, False):
        want = cv.rhat(chain, split)
        assert want.shape == (4,)
        np.testing.assert_array_equal(m.get_rhat(split=split, **kw), want)
        np.testing.assert_array_equal(m.get_rhat(chain=chain, split=split), want)
        lp = m._sampler.get_log_prob(**kw)
        got = m.get_log_prob_rhat(split=split, **kw)
        assert isinstance(got, float) and got == cv.rhat(lp[:, :, None], split)[0]
    np.testing.assert_array_equal(m.get_walker_mean(**kw), np.mean(chain, axis=0))
    np.testing.assert_array_equal(m.get_walker_std(**kw), np.std(chain, axis=0, ddof=1))
    np.testing.assert_array_equal(m.get_walker_std(chain=chain), np.std(chain, axis=0, ddof=1))
    assert m.get_walker_mean(**kw).shape == (8, 4)


@pytest.mark.parametrize('method', ['get_rhat', 'get_walker_mean', 'get_walker_std', 'get_log_prob_rhat'])
def test_inversion_refusals(method):
    m = fitted_on_host()
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=20)
    with pytest.raises(TypeError, match='flat'):
        f(flat=True)
    with pytest.raises(TypeError, match='unexpected keyword'):
        f(bins=3)
    if method != 'get_log_prob_rhat':
        with pytest.raises(ValueError, match='unflattened'):
            f(chain=m.get_chain(flat=True))
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=m.get_chain(), discard=5)
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=m.get_chain(), thin=2)
    if method in ('get_rhat', 'get_log_prob_rhat'):
        with pytest.raises(ValueError, match='2 per chain'):
            f(discard=17)                                # 3 used samples: halves of one
    import bisip_amd
    unfitted = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=8)
    with pytest.raises(AssertionError, match='not fitted'):
        getattr(unfitted, method)()


class _HostChainSampler:
    """What SpectraBatch asks of its sampler, answered from a host chain (n, E, Wp, ndim) by the definitions."""

    def __init__(self, chain, lp):
        self.chain, self.lp = chain, lp

    def _used(self, a, discard, thin):
        return a[discard + thin - 1::thin]

    def split_rhat(self, discard=0, thin=1, split=True):
        c = self._used(self.chain, discard, thin)
        return np.stack([cv.rhat(c[:, e], split) for e in range(c.shape[1])])

    def walker_moments(self, discard=0, thin=1):
        c = self._used(self.chain, discard, thin)
        return np.mean(c, axis=0), np.var(c, axis=0, ddof=1)

    def log_prob_rhat(self, discard=0, thin=1, split=True):
        lp = self._used(self.lp, discard, thin)
        return np.stack([cv.rhat(lp[:, e, :, None], split)[0] for e in range(lp.shape[1])])


def test_spectra_batch_methods_on_a_host_chain():
    from bisip_amd.batch import SpectraBatch
    rng = np.random.default_rng(8)
    chain, lp = rng.normal(size=(30, 3, 6, 4)), rng.normal(size=(30, 3, 6))
    b = SpectraBatch.__new__(SpectraBatch)
    b._fitted = lambda: _HostChainSampler(chain, lp)
    kw = dict(discard=4, thin=2)
    used = chain[5::2]
    assert b.get_rhat(**kw).shape == (3, 4)
    np.testing.assert_array_equal(b.get_rhat(split=False, **kw)[1], cv.rhat(used[:, 1], split=False))
    assert b.get_walker_mean(**kw).shape == (3, 6, 4)
    np.testing.assert_array_equal(b.get_walker_mean(**kw), used.mean(axis=0))
    np.testing.assert_array_equal(b.get_walker_std(**kw), used.std(axis=0, ddof=1))
    assert b.get_log_prob_rhat(**kw).shape == (3,)


def test_entry_points_exist(hip_lib):
    from __graft_entry__ import header_abi_version
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in ('bisip_chain_rhat_dev', 'bisip_chain_rhat_workspace'):
        assert hasattr(hip_lib, name)
        assert re.search(r'\b%s\(' % name, header)
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    assert 'bisip_*' in exports                                # every bisip_ symbol leaves the library
    assert hip_lib.bisip_abi_version() == header_abi_version() == 6


def test_workspace_follows_the_plan():
    from bisip_amd import _hip
    assert _hip.chain_rhat_workspace(500, 512, 256, 7, 2) == 0          # a survey needs none
    assert _hip.chain_rhat_workspace(500, 512, 256, 7, 1) == 0
    for n, E, Wp, ndim, splits in [(5000, 1, 32, 7, 2), (600, 64, 64, 7, 2), (7, 2, 65, 7, 2), (64, 255, 3, 2, 1)]:
        C, L = E * Wp * ndim, n // splits
        nseg = cv.segment_plan(L, C, splits)[1]
        assert _hip.chain_rhat_workspace(n, E, Wp, ndim, splits) == 8 * (2 * splits * C + (2 * splits * nseg * C if nseg > 1 else 0))
    for bad in ((3, 1, 8, 3, 2), (1, 1, 8, 3, 1), (4, 1, 1, 3, 1), (4, 0, 8, 3, 2), (4, 1, 0, 3, 2), (4, 1, 8, 17, 2),
                (4, 1, 8, 0, 2), (4, 1, 8, 3, 3), (4, 1, 8, 3, 0)):
        assert _hip.chain_rhat_workspace(*bad) < 0
    assert _hip.chain_rhat_workspace(4, 1, 1, 3, 2) >= 0                # one walker, two halves


def test_entry_point_checks_its_arguments():
    from bisip_amd import _hip
    ok = dict(n=8, stride=8 * 3, E=1, Wp=8, ndim=3, splits=2, mean=4096, var=4096, rhat=4096, chain=4096, work=4096,
              nbytes=1 << 20)
    # the pointers are never dereferenced: every call below is refused on the host

    def call(**kw):
        a = dict(ok, **kw)
        _hip.chain_rhat_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['splits'], a['mean'], a['var'],
                            a['rhat'], a['work'], a['nbytes'], 0)

    with pytest.raises(ValueError, match='ndim'):
        call(ndim=17, stride=8 * 17)
    with pytest.raises(ValueError, match='splits'):
        call(splits=3)
    with pytest.raises(ValueError, match='sample_stride'):
        call(stride=23)
    with pytest.raises(ValueError, match='2 samples'):
        call(n=3)
    with pytest.raises(ValueError, match='2 samples'):
        call(n=1, splits=1)
    with pytest.raises(ValueError, match='2 chains'):
        call(Wp=1, splits=1, stride=3)
    with pytest.raises(ValueError, match='bad chain shape'):
        call(E=0)
    with pytest.raises(ValueError, match='null'):
        call(chain=0)
    with pytest.raises(ValueError, match='none of'):
        call(mean=0, var=0, rhat=0)
    with pytest.raises(ValueError, match='workspace'):
        call(work=0)
    with pytest.raises(ValueError, match='workspace'):
        call(nbytes=8)
