"""bisip_amd.covariance on the host: the definitions of the posterior covariance, the correlation and the best sample
against NumPy's own, the NumPy restatement of the device's summation order against the long-double reference, the plans,
the refusals of the two entry points, and the methods of every model and of SpectraBatch on host chains."""
import os
import re

import numpy as np
import pytest

from bisip_amd import covariance as cv
from convergence_bounds import hand_built_chain
from covariance_bounds import assert_within, reference_and_bounds, rows_of
from fitted import fitted_on_host, gaussian_logp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definitions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 3])
@pytest.mark.parametrize('ndim', [1, 4, 7])
def test_flat_cov_and_corr_against_numpy(E, ndim):
    rng = np.random.default_rng(10 * E + ndim)
    x = rng.normal(size=(40, E * 6, ndim)) @ rng.normal(size=(ndim, ndim)) + rng.normal(size=ndim) * 100
    mean, cov = cv.flat_cov(x, E)
    assert mean.shape == (E, ndim) and cov.shape == (E, ndim, ndim)
    corr = cv.corr_from_cov(cov)
    for e in range(E):
        rows = rows_of(x, E)[e]
        np.testing.assert_array_equal(rows, x[:, e * 6:(e + 1) * 6].reshape(-1, ndim))      # get_chain(flat=True)'s order
        np.testing.assert_array_equal(cov[e], np.atleast_2d(np.cov(rows.T, ddof=1)))
        # (np.corrcoef of ONE variable returns c / c = 1 without taking its steps)
        v = np.cov(rows.T, ddof=1)
        want = np.corrcoef(rows.T) if ndim > 1 else np.clip(v / np.sqrt(v) / np.sqrt(v), -1, 1).reshape(1, 1)
        np.testing.assert_array_equal(corr[e], want)
        np.testing.assert_array_equal(mean[e], rows.mean(axis=0))
    if E == 1:
        flat = x.reshape(-1, ndim)
        np.testing.assert_array_equal(cv.flat_cov(flat)[1], cov)


def test_corr_of_a_constant_parameter_is_nan():
    x = np.random.default_rng(1).normal(size=(30, 4, 3))
    x[:, :, 1] = 0.25
    mean, cov = cv.flat_cov(x)
    assert (cov[0, 1] == 0).all() and (cov[0, :, 1] == 0).all()
    corr = cv.corr_from_cov(cov)
    assert np.isnan(corr[0, 1]).all() and np.isnan(corr[0, :, 1]).all()
    assert abs(corr[0, 0, 0] - 1.0) < 4e-16 and abs(corr[0, 2, 2] - 1.0) < 4e-16 and np.isfinite(corr[0, 0, 2])
    assert np.abs(cv.corr_from_cov(np.array([[1.0, 1.0 + 1e-15], [1.0 + 1e-15, 1.0]]))).max() == 1.0      # clipped


def test_value_errors():
    rng = np.random.default_rng(3)
    with pytest.raises(ValueError, match='2 rows'):
        cv.flat_cov(rng.normal(size=(1, 1, 2)))
    with pytest.raises(ValueError, match='2 rows'):
        cv.ordered_cov(rng.normal(size=(1, 3, 2)), n_ensembles=3)
    with pytest.raises(ValueError, match='divide'):
        cv.flat_cov(rng.normal(size=(4, 5, 2)), n_ensembles=2)
    with pytest.raises(ValueError, match='one ensemble'):
        cv.flat_cov(rng.normal(size=(10, 2)), n_ensembles=2)
    with pytest.raises(ValueError, match='expected a chain'):
        cv.flat_cov(rng.normal(size=(10,)))
    with pytest.raises(ValueError, match='log-probability of shape'):
        cv.best_sample(rng.normal(size=(4, 5, 2)), rng.normal(size=(4, 4)))


# -- the device's order, restated -----------------------------------------------------------------------------------
# (n, E, Wp, ndim): one segment; two segments, the second of one row (205 * 5 = 1025 rows); T = 64 slots; several ensembles
@pytest.mark.parametrize('shape', [(1, 1, 2, 1), (5, 3, 2, 2), (7, 2, 65, 7), (204, 1, 5, 3), (205, 1, 5, 3),
                                   (30, 2, 40, 9), (3, 256, 3, 2), (70, 1, 33, 16)])
def test_ordered_cov_against_the_definition(shape):
    n, E, Wp, ndim = shape
    x, _, _ = hand_built_chain(*shape)
    mean, cov = cv.ordered_cov(x, n_ensembles=E)
    assert mean.shape == (E, ndim) and cov.shape == (E, ndim, ndim)
    np.testing.assert_array_equal(cov.view(np.uint64), cov.transpose(0, 2, 1).copy().view(np.uint64))
    ref = reference_and_bounds(x, E)
    worst = max(assert_within(mean, ref, 'mean', str(shape)), assert_within(cov, ref, 'cov', str(shape)),
                assert_within(cv.corr_from_cov(cov), ref, 'corr', str(shape)))
    print(f'{shape}: error at most {worst:.3f} of its bound')
    with np.errstate(all='ignore'):
        rel = ref['dcov'][:, 0, 0] / ref['cov'][:, 0, 0]
    assert rel.max() < 1e-9                                  # parameter 0 is centred at 0: else the inputs are wrong
    fm, fc = cv.flat_cov(x, E)
    fin = np.isfinite(fc)
    np.testing.assert_array_equal(np.isfinite(cov), fin)
    np.testing.assert_allclose(cov[fin], fc[fin], rtol=1e-6, atol=1e-300)


def test_plans():
    assert cv.plan(500, 512, 256, 7) == (128000, 1, 256)               # a survey: one segment per ensemble
    assert cv.plan(9, 256, 3, 2) == (27, 1, 256) and cv.plan(9, 255, 3, 2) == (1024, 1, 256)
    assert cv.plan(5000, 1, 32, 7) == (1024, 157, 256)                 # the quickstart: cut to fill the chip
    assert cv.plan(204, 1, 5, 3)[1] == 1 and cv.plan(205, 1, 5, 3)[1] == 2
    assert cv.plan(2, 1, 1 << 20, 16) == (1024, 2048, 64)              # one big ensemble of two samples
    assert cv.plan(600, 64, 64, 7) == (1200, 32, 256)
    assert cv.best_plan(5000, 1, 32) == (4096, 40) and cv.best_plan(500, 512, 256) == (128000, 1)
    assert cv.best_plan(819, 1, 5) == (4096, 1) and cv.best_plan(820, 1, 5) == (4096, 2)


# -- best sample ------------------------------------------------------------------------------------------------------
def test_best_sample_definition():
    rng = np.random.default_rng(7)
    n, E, Wp, ndim = 6, 3, 4, 2
    x, lp = rng.normal(size=(n, E * Wp, ndim)), rng.normal(size=(n, E * Wp))
    lp[2, 1] = lp[4, 3] = 50.0                          # ensemble 0: a tie, rows 2 * 4 + 1 and 4 * 4 + 3
    lp[0, 4] = np.nan                                   # ensemble 1: a NaN never wins
    lp[3, 6] = 9.0
    lp[:, 8:] = -np.inf                                 # ensemble 2: all -inf
    theta, best, index = cv.best_sample(x, lp, E)
    assert index.dtype == np.int64
    np.testing.assert_array_equal(index, [9, 3 * 4 + 2, 0])
    np.testing.assert_array_equal(best, [50.0, 9.0, -np.inf])
    np.testing.assert_array_equal(theta, [x[2, 1], x[3, 6], x[0, 8]])
    for e in range(E):
        le = lp[:, e * Wp:(e + 1) * Wp].reshape(-1)
        assert index[e] == np.argmax(np.where(np.isnan(le), -np.inf, le))
    lp[:, :4] = np.nan                                  # all NaN: index 0, the stored NaN
    lp[1:, 8:] = np.nan                                 # NaN and -inf mixed
    theta, best, index = cv.best_sample(x, lp, E)
    assert index[0] == 0 and np.isnan(best[0]) and index[2] == 0 and best[2] == -np.inf
    t1, b1, i1 = cv.best_sample(x[:, :4].reshape(-1, ndim), rng.normal(size=n * 4))      # flat, one ensemble
    assert t1.shape == (1, ndim) and b1.shape == i1.shape == (1,)


# -- plumbing -------------------------------------------------------------------------------------------------------
def test_entry_points_exist(hip_lib):
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in ('bisip_chain_cov_dev', 'bisip_chain_cov_workspace', 'bisip_chain_best_sample_dev',
                 'bisip_chain_best_sample_workspace'):
        assert hasattr(hip_lib, name)
        assert re.search(r'\b%s\(' % name, header)
        assert callable(getattr(_hip, name[len('bisip_'):]))
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    assert 'bisip_*' in exports                                # every bisip_ symbol leaves the library


def test_workspace_follows_the_plan():
    from bisip_amd import _hip
    assert _hip.chain_cov_workspace(500, 512, 256, 7) == 0               # a survey needs none
    assert _hip.chain_cov_workspace(9, 256, 3, 2) == 0
    assert _hip.chain_best_sample_workspace(500, 512, 256) == 0
    for n, E, Wp, ndim in [(5000, 1, 32, 7), (600, 64, 64, 7), (205, 1, 5, 3), (2, 1, 1 << 20, 16), (9, 255, 3, 2)]:
        nseg = cv.plan(n, E, Wp, ndim)[1]
        sums = ndim + ndim * (ndim + 1) // 2
        assert _hip.chain_cov_workspace(n, E, Wp, ndim) == (8 * E * nseg * sums if nseg > 1 else 0)
        nseg = cv.best_plan(n, E, Wp)[1]
        assert _hip.chain_best_sample_workspace(n, E, Wp) == (16 * E * nseg if nseg > 1 else 0)
    assert _hip.chain_cov_workspace(1, 1, 2, 1) == 0 and _hip.chain_cov_workspace(204, 1, 5, 3) == 0
    for bad in ((1, 1, 1, 3), (0, 1, 8, 3), (4, 0, 8, 3), (4, 1, 0, 3), (4, 1, 8, 17), (4, 1, 8, 0), (1 << 31, 1, 8, 3),
                (4, 1, 1 << 27, 3)):
        assert _hip.chain_cov_workspace(*bad) < 0
    for bad in ((0, 1, 8), (4, 0, 8), (4, 1, 0), (4, 1, 1 << 27)):
        assert _hip.chain_best_sample_workspace(*bad) < 0
    assert _hip.chain_best_sample_workspace(1, 1, 1) == 0               # one row has a best sample


def test_entry_points_check_their_arguments():
    from bisip_amd import _hip
    # the pointers are never dereferenced: every call below is refused on the host
    ok = dict(chain=4096, n=8, stride=8 * 3, E=1, Wp=8, ndim=3, mean=4096, cov=4096, work=4096, nbytes=1 << 20)

    def cov(**kw):
        a = dict(ok, **kw)
        _hip.chain_cov_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['mean'], a['cov'], a['work'],
                           a['nbytes'], 0)

    with pytest.raises(ValueError, match='2 rows'):
        cov(n=1, Wp=1, stride=3)
    with pytest.raises(ValueError, match='ndim'):
        cov(ndim=0)
    with pytest.raises(ValueError, match='ndim'):
        cov(ndim=17, stride=8 * 17)
    with pytest.raises(ValueError, match='sample_stride'):
        cov(stride=23)
    with pytest.raises(ValueError, match='bad chain shape'):
        cov(E=0)
    with pytest.raises(ValueError, match='null'):
        cov(chain=0)
    with pytest.raises(ValueError, match='null'):
        cov(cov=0)
    with pytest.raises(ValueError, match='workspace'):
        cov(n=300, work=0)                                   # 2400 rows: three segments
    with pytest.raises(ValueError, match='workspace'):
        cov(n=300, nbytes=8)

    okb = dict(chain=4096, cstride=8 * 3, logp=4096, lstride=8, n=8, E=1, Wp=8, ndim=3, theta=4096, best=4096, index=4096,
               work=4096, nbytes=1 << 20)

    def best(**kw):
        a = dict(okb, **kw)
        _hip.chain_best_sample_dev(a['chain'], a['cstride'], a['logp'], a['lstride'], a['n'], a['E'], a['Wp'], a['ndim'],
                                   a['theta'], a['best'], a['index'], a['work'], a['nbytes'], 0)

    with pytest.raises(ValueError, match='none of'):
        best(theta=0, best=0, index=0)
    with pytest.raises(ValueError, match='without a chain'):
        best(chain=0)
    with pytest.raises(ValueError, match='null'):
        best(logp=0)
    with pytest.raises(ValueError, match='ndim'):
        best(ndim=0)
    with pytest.raises(ValueError, match='ndim'):
        best(ndim=17, cstride=8 * 17)
    with pytest.raises(ValueError, match='logp_stride'):
        best(lstride=7)
    with pytest.raises(ValueError, match='chain_stride'):
        best(cstride=23)
    with pytest.raises(ValueError, match='bad chain shape'):
        best(n=0)
    with pytest.raises(ValueError, match='workspace'):
        best(n=1000, work=0)                                 # 8000 rows: two segments


@pytest.mark.parametrize('kw', [dict(), dict(discard=5, thin=3)])
def test_inversion_methods_with_the_host_sampler(kw):
    m = fitted_on_host()
    flat = m.get_chain(flat=True, **kw)
    with pytest.warns(UserWarning, match='No samples were discarded') if not kw else _no_warning():
        got = m.get_param_cov(**kw)
    assert got.shape == (4, 4)
    np.testing.assert_array_equal(got, np.cov(flat.T, ddof=1))
    np.testing.assert_array_equal(m.get_param_cov(chain=flat), np.cov(flat.T, ddof=1))
    np.testing.assert_array_equal(m.get_param_corr(chain=flat), np.corrcoef(flat.T))
    if kw:
        np.testing.assert_array_equal(m.get_param_corr(**kw), np.corrcoef(flat.T))
    with pytest.warns(UserWarning, match='No samples were discarded') if not kw else _no_warning():
        theta, lp = m.get_best_sample(**kw)
    flat_lp = m._sampler.get_log_prob(flat=True, **kw)
    assert theta.shape == (4,) and isinstance(lp, float)
    assert lp == flat_lp.max()
    np.testing.assert_array_equal(theta, flat[np.argmax(flat_lp)])
    assert gaussian_logp(theta[None])[0] == lp


class _no_warning:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_inversion_refusals():
    m = fitted_on_host()
    flat = m.get_chain(flat=True)
    for f in (m.get_param_cov, m.get_param_corr):
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=flat, discard=5)
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=flat, thin=2)
        with pytest.raises(ValueError, match='Flatten'):
            f(chain=m.get_chain())
    with pytest.raises(ValueError, match='no samples'):
        m.get_best_sample(discard=20)
    with pytest.raises(TypeError, match='flat'):
        m.get_best_sample(flat=True)
    import bisip_amd
    unfitted = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=8)
    for name in ('get_param_cov', 'get_param_corr', 'get_best_sample'):
        with pytest.raises(AssertionError, match='not fitted'):
            getattr(unfitted, name)()


class _HostChainSampler:
    """What SpectraBatch asks of its sampler, answered from a host chain (n, E, Wp, ndim) by the definitions."""

    def __init__(self, chain, lp):
        self.chain, self.lp = chain, lp

    def _used(self, a, discard, thin):
        a = a[discard + thin - 1::thin]
        return a.reshape((a.shape[0], a.shape[1] * a.shape[2]) + a.shape[3:])

    def param_cov(self, discard=0, thin=1):
        return cv.flat_cov(self._used(self.chain, discard, thin), self.chain.shape[1])[1]

    def param_corr(self, discard=0, thin=1):
        return cv.corr_from_cov(self.param_cov(discard, thin))

    def best_sample(self, discard=0, thin=1):
        return cv.best_sample(self._used(self.chain, discard, thin), self._used(self.lp, discard, thin), self.chain.shape[1])


def test_spectra_batch_methods_on_a_host_chain():
    from bisip_amd.batch import SpectraBatch
    rng = np.random.default_rng(8)
    chain, lp = rng.normal(size=(30, 3, 6, 4)), rng.normal(size=(30, 3, 6))
    b = SpectraBatch.__new__(SpectraBatch)
    b._fitted = lambda: _HostChainSampler(chain, lp)
    kw = dict(discard=4, thin=2)
    used, used_lp = chain[5::2], lp[5::2]
    cov = b.get_param_cov(**kw)
    assert cov.shape == (3, 4, 4)
    np.testing.assert_array_equal(cov[1], np.cov(used[:, 1].reshape(-1, 4).T, ddof=1))
    np.testing.assert_array_equal(b.get_param_corr(**kw)[2], np.corrcoef(used[:, 2].reshape(-1, 4).T))
    theta, best = b.get_best_sample(**kw)
    assert theta.shape == (3, 4) and best.shape == (3,)
    np.testing.assert_array_equal(best, used_lp.transpose(1, 0, 2).reshape(3, -1).max(axis=1))
    np.testing.assert_array_equal(theta[0], used[:, 0].reshape(-1, 4)[np.argmax(used_lp[:, 0].reshape(-1))])
