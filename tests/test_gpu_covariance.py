"""Posterior covariance and best sample on the device (bisip_chain_cov_dev, bisip_chain_best_sample_dev), from the C entry
points up to the model and SpectraBatch methods.  Mean and covariance are held, bit for bit, to the summation order
include/bisip_hip.h states (bisip_amd.covariance.ordered_cov) and, against the long-double evaluation of the definitions,
to the first-order bound of any summation order that tests/covariance_bounds.py derives and computes per case from the
data.  The best sample is exact: equality with the NumPy definition."""
import functools

import numpy as np
import pytest

import fitted
from chain_harness import SENTINEL, GuardedCall, assert_same_bits, shape_id, store
from convergence_bounds import U, hand_built_chain
from covariance_bounds import assert_within, reference_and_bounds
from moments_bounds import assert_within_bounds as assert_moments_within, reference_and_bounds as moments_reference

pytestmark = pytest.mark.gpu

LP_PAD = 3                         # the log-probability has a padding of its own

# (n, E, Wp, ndim).  Rows N = n * Wp are cut into segments of 1024 at least (covariance.plan) and tiles of T = 256 (ndim
# <= 8) or 64 rows: (204 | 205, 1, 5, q) have 1020 | 1025 rows, one segment | two with the second of one row, for both T;
# (410, 1, 5, 3) has two whole segments and two rows; (256 | 257, 1, 1, 2) and (64 | 65, 1, 1, 9) lie on both sides of one
# tile.  (9, 256, 3, 2) is the first ensemble count that takes one segment whatever N, (9, 255, 3, 2) the last that does
# not; (3, 256, 700, 7) is that path with several tiles that cross samples; (1, 1, 2, 1) the smallest legal shape.
SHAPES = [(1, 1, 2, 1), (5, 3, 2, 2), (40, 1, 1, 2), (7, 2, 63, 7), (7, 2, 64, 7), (7, 2, 65, 7), (6, 5, 9, 3),
          (9, 2, 100, 8), (9, 2, 100, 9), (4, 1, 257, 16), (204, 1, 5, 3), (205, 1, 5, 3), (204, 1, 5, 9), (205, 1, 5, 9),
          (410, 1, 5, 3), (256, 1, 1, 2), (257, 1, 1, 2), (64, 1, 1, 9), (65, 1, 1, 9), (9, 255, 3, 2), (9, 256, 3, 2),
          (3, 256, 700, 7), (5, 256, 128, 16), (5000, 1, 32, 7), (600, 64, 64, 7)]


@functools.lru_cache(maxsize=None)
def case(n, E, Wp, ndim):
    """(store() of the chain, used chain (n, E * Wp, ndim), ordered (mean, cov), reference and bounds)"""
    from bisip_amd import covariance as cv
    x, _, _ = hand_built_chain(n, E, Wp, ndim)
    stored = store(x)
    ordered = cv.ordered_cov(x, n_ensembles=E)
    ref = reference_and_bounds(x, E)
    x.setflags(write=False)
    return stored, x, ordered, ref


def run_cov(stored, n, E, Wp, ndim, mean=True):
    """One call; a mean not asked for stays SENTINEL.  Outputs and workspace are followed by guard bytes."""
    import torch
    from bisip_amd import _hip
    samples, offset, stride = stored
    t = torch.from_numpy(samples).cuda()
    call = GuardedCall()
    m, c = call.out('the mean', (E, ndim), asked=mean), call.out('the covariance', (E, ndim, ndim))
    nbytes = _hip.chain_cov_workspace(n, E, Wp, ndim)
    _hip.chain_cov_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, m, c, call.work(nbytes), nbytes, call.stream)
    return (*call.finish(), nbytes)


@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_cov_entry_point(shape):
    from bisip_amd import covariance as cv
    n, E, Wp, ndim = shape
    stored, x, (om, oc), ref = case(*shape)
    m, c, nbytes = run_cov(stored, n, E, Wp, ndim)
    assert not (m == SENTINEL).any() and not (c == SENTINEL).any()
    nseg = cv.plan(n, E, Wp, ndim)[1]
    assert (nbytes == 0) == (nseg == 1)
    if E >= 256:
        assert nbytes == 0
    if shape == (5000, 1, 32, 7):
        assert nseg > 1                                              # the quickstart is cut into segments
    np.testing.assert_array_equal(c.view(np.uint64), c.transpose(0, 2, 1).copy().view(np.uint64))     # [j, k] is [k, j]
    assert_same_bits(m, om, 'mean')
    assert_same_bits(c, oc, 'cov')
    worst = max(assert_within(m, ref, 'mean', str(shape)), assert_within(c, ref, 'cov', str(shape)),
                assert_within(cv.corr_from_cov(c), ref, 'corr', str(shape)))
    # parameter 0 has its centre at 0: there the bound itself must be small, else the inputs are wrong
    with np.errstate(all='ignore'):
        pos = ref['cov'][:, 0, 0] > 0
        rel = (ref['dcov'][:, 0, 0] / ref['cov'][:, 0, 0])[pos]
    assert pos.any() or (E, Wp) == (1, 1)       # (hand_built_chain holds the last walker of ensemble 0 constant there)
    assert not rel.size or rel.max() < 1e-9, float(rel.max())
    print(f'shape {shape}: error at most {worst:.3f} of its bound; bound on the variance '
          f'{float(rel.max()) if rel.size else 0:.1e} relative; {nseg} segment(s), workspace {nbytes} bytes')
    if ndim > 1:                                # the constant parameter: a row and a column of exact zeros
        assert (c[E - 1, ndim - 1, :] == 0.0).all() and (c[E - 1, :, ndim - 1] == 0.0).all() or \
            not np.isfinite(ref['cov'][E - 1, ndim - 1].astype(np.float64)).all()
    assert np.isfinite(c[:, 0, 0]).all() and (c[:, 0, 0] >= 0).all()


@pytest.mark.parametrize('shape', [(7, 2, 65, 7), (205, 1, 5, 9), (9, 256, 3, 2)], ids=shape_id)
def test_cov_null_mean_and_repeat(shape):
    n, E, Wp, ndim = shape
    stored = case(*shape)[0]
    m, c, _ = run_cov(stored, n, E, Wp, ndim)
    m0, c0, _ = run_cov(stored, n, E, Wp, ndim, mean=False)
    assert (m0 == SENTINEL).all()
    np.testing.assert_array_equal(c0.view(np.uint64), c.view(np.uint64))
    m1, c1, _ = run_cov(stored, n, E, Wp, ndim)
    np.testing.assert_array_equal(c1.view(np.uint64), c.view(np.uint64))
    np.testing.assert_array_equal(m1.view(np.uint64), m.view(np.uint64))


@pytest.mark.parametrize('shape', [(50, 2, 8, 4), (300, 2, 8, 4), (40, 2, 8, 10)], ids=shape_id)
def test_cov_known_answers(shape):
    """A constant parameter: exact zeros and NaN correlation.  A parameter that is twice another (its shift too): twice
    the sums, bit for bit.  A NaN in one parameter of one ensemble: that row and column of that ensemble and nothing else."""
    from bisip_amd import covariance as cv
    n, E, Wp, ndim = shape
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, E * Wp, ndim)) * 0.01 + rng.normal(size=ndim)
    x[:, :Wp, 1] = 0.25
    x[:, :, 3] = 2.0 * x[:, :, 2]
    m, c, _ = run_cov(store(x), n, E, Wp, ndim)
    assert (c[0, 1, :] == 0.0).all() and (c[0, :, 1] == 0.0).all() and (m[0, 1] == 0.25)
    corr = cv.corr_from_cov(c)
    assert np.isnan(corr[0, 1, :]).all() and np.isnan(corr[0, :, 1]).all()
    assert np.isfinite(corr[1]).all() and np.isfinite(np.delete(np.delete(corr[0], 1, 0), 1, 1)).all()
    np.testing.assert_array_equal(c[:, 2, 3], 2.0 * c[:, 2, 2])
    np.testing.assert_array_equal(c[:, 3, 3], 4.0 * c[:, 2, 2])
    ref = reference_and_bounds(x, E)
    assert (np.abs(corr[:, 2, 3] - 1.0) <= ref['dcorr'][:, 2, 3]).all()
    assert_within(corr, ref, 'corr')
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[n // 2, Wp + 3, 2] = bad
        _, cb, _ = run_cov(store(y), n, E, Wp, ndim)
        spoilt = np.zeros((E, ndim, ndim), dtype=bool)
        spoilt[1, 2, :] = spoilt[1, :, 2] = True
        np.testing.assert_array_equal(~np.isfinite(cb), spoilt)
        np.testing.assert_array_equal(cb[~spoilt].view(np.uint64), c[~spoilt].view(np.uint64))


def test_cov_of_a_device_tensor():
    import torch
    from bisip_amd import covariance as cv
    x = np.random.default_rng(5).normal(size=(40, 6, 3))
    for E in (1, 2):
        mean, cov = cv.flat_cov(torch.from_numpy(x).cuda(), E)
        om, oc = cv.ordered_cov(x, E)
        np.testing.assert_array_equal(cov, oc)
        np.testing.assert_array_equal(mean, om)
        np.testing.assert_allclose(cov, cv.flat_cov(x, E)[1], rtol=1e-12, atol=1e-15)
    flat = x.reshape(-1, 3)
    np.testing.assert_array_equal(cv.flat_cov(torch.from_numpy(flat).cuda())[1], cv.ordered_cov(flat)[1])
    lp = np.random.default_rng(6).normal(size=(40, 6))
    for got, want in zip(cv.best_sample(torch.from_numpy(x).cuda(), torch.from_numpy(lp).cuda(), 2), cv.best_sample(x, lp, 2)):
        np.testing.assert_array_equal(got, want)


# -- best sample ------------------------------------------------------------------------------------------------------
_uploaded = {}


def run_best(x, lp, E, theta=True, best=True, index=True):
    """x (n, E * Wp, ndim), lp (n, E * Wp) through their own strides and paddings; outputs not asked for stay SENTINEL
    (the index: -7)."""
    import torch
    from bisip_amd import _hip
    n, W, ndim = x.shape
    Wp = W // E
    if _uploaded.get('id') != id(x):                    # (the chain of a test goes up once)
        _uploaded.clear()
        stored, offset, stride = store(x)
        _uploaded.update(id=id(x), x=x, chain=(torch.from_numpy(stored).cuda(), offset, stride))
    tx, coffset, cstride = _uploaded['chain']
    sl, loffset, lstride = store(lp, pad=LP_PAD)
    tl = torch.from_numpy(sl).cuda()
    call = GuardedCall()
    th, b = call.out('theta', (E, ndim), asked=theta), call.out('the log-probability', (E,), asked=best)
    ix = call.out('the index', (E,), torch.int64, asked=index)
    nbytes = _hip.chain_best_sample_workspace(n, E, Wp)
    _hip.chain_best_sample_dev(tx.data_ptr() + 8 * coffset if theta else 0, cstride, tl.data_ptr() + 8 * loffset, lstride,
                               n, E, Wp, ndim, th, b, ix, call.work(nbytes), nbytes, call.stream)
    return tuple(call.finish())


def numpy_best(x, lp, E):
    """The definition, written out: argmax of every ensemble's values in row order with NaN read as -inf."""
    n, W, ndim = x.shape
    Wp = W // E
    lpr = lp.reshape(n, E, Wp).transpose(1, 0, 2).reshape(E, n * Wp)
    index = np.array([np.argmax(np.where(np.isnan(v), -np.inf, v)) for v in lpr], dtype=np.int64)
    e = np.arange(E)
    return x[index // Wp, e * Wp + index % Wp], lpr[e, index], index


def assert_best(x, lp, E, label=''):
    theta, best, index = run_best(x, lp, E)
    wt, wb, wi = numpy_best(x, lp, E)
    np.testing.assert_array_equal(index, wi, err_msg=label)
    np.testing.assert_array_equal(best.view(np.uint64), wb.view(np.uint64), err_msg=label)
    np.testing.assert_array_equal(theta.view(np.uint64), wt.view(np.uint64), err_msg=label)
    return index


BEST_SHAPES = [(1, 1, 1, 1), (7, 2, 65, 7), (819, 1, 5, 3), (820, 1, 5, 3), (9, 255, 3, 2), (9, 256, 3, 2), (4, 1, 257, 16),
               (5000, 1, 32, 7), (600, 64, 64, 7), (2100, 1, 128, 2)]
# (2100, 1, 128, 2): 268,800 rows in 66 segments of 4096 -- more than the 64 lanes of the wave that merges the segments'
# keys (k_best_merge), whose lanes 0 and 1 then take a second segment each


@pytest.mark.parametrize('shape', BEST_SHAPES, ids=shape_id)
def test_best_sample_entry_point(shape):
    from bisip_amd import covariance as cv
    n, E, Wp, ndim = shape
    rng = np.random.default_rng(sum(shape))
    x, lp = rng.normal(size=(n, E * Wp, ndim)), -rng.exponential(size=(n, E * Wp))
    N = n * Wp
    seg_rows, nseg = cv.best_plan(n, E, Wp)
    assert_best(x, lp, E, 'random')
    for got, want in zip(cv.best_sample(x, lp, E), numpy_best(x, lp, E)):
        np.testing.assert_array_equal(got, want)
    if shape == (2100, 1, 128, 2):
        assert nseg == 66
    # the maximum at the first, the last and a middle row, on both sides of EVERY segment boundary, in the middle of the
    # last segment, and on both sides of the rows one pass of a workgroup takes (256)
    where = {0, N - 1, N // 2, 255, 256, 257, (nseg - 1) * seg_rows + (N - (nseg - 1) * seg_rows) // 2}
    for g in range(1, nseg):
        where |= {g * seg_rows - 1, g * seg_rows}
    e = E // 2
    for r in sorted(w for w in where if 0 <= w < N):
        y = lp.copy()
        y[r // Wp, e * Wp + r % Wp] = 1.0
        assert assert_best(x, y, E, f'row {r}')[e] == r
    if N >= 3:
        # the same maximum twice: the lowest index wins; a NaN "larger than" everything is ignored
        y = lp.copy()
        for r in (N - 1, N // 2):
            y[r // Wp, e * Wp + r % Wp] = 2.0
        y[0, e * Wp] = np.nan
        assert assert_best(x, y, E, 'tie')[e] == N // 2
        y[(N // 3) // Wp, e * Wp + (N // 3) % Wp] = 2.0
        assert assert_best(x, y, E, 'tie of three')[e] == N // 3
    y = lp.copy()
    y[:, e * Wp:(e + 1) * Wp] = -np.inf                 # all -inf: index 0
    assert assert_best(x, y, E, 'all -inf')[e] == 0
    y[:, e * Wp:(e + 1) * Wp] = np.nan                  # all NaN: index 0, the stored NaN
    assert assert_best(x, y, E, 'all NaN')[e] == 0


@pytest.mark.parametrize('shape', [(7, 2, 65, 7), (820, 1, 5, 3)], ids=shape_id)
def test_best_sample_null_outputs(shape):
    n, E, Wp, ndim = shape
    rng = np.random.default_rng(3)
    x, lp = rng.normal(size=(n, E * Wp, ndim)), rng.normal(size=(n, E * Wp))
    full = run_best(x, lp, E)
    for k in range(1, 8):
        ask = [bool(k & 1), bool(k & 2), bool(k & 4)]
        got = run_best(x, lp, E, *ask)
        for a, g, f, fill in zip(ask, got, full, (SENTINEL, SENTINEL, -7)):
            if a:
                np.testing.assert_array_equal(g, f)
            else:
                assert (g == fill).all()


# -- through the layers ---------------------------------------------------------------------------------------------
KW = dict(discard=20, thin=2)


fitted_model = functools.lru_cache(maxsize=None)(fitted.fitted_model)


def check_layers(chain, lp, cov, corr, std, theta, best, logp_of, E):
    """chain (n, E * Wp, ndim), lp (n, E * Wp) against the methods' values (leading axis E)."""
    n, W, ndim = chain.shape
    N = n * (W // E)
    ref = reference_and_bounds(chain, E)
    assert_within(cov, ref, 'cov')
    assert_within(corr, ref, 'corr')
    flat = chain.reshape(n, E, W // E, ndim).transpose(1, 0, 2, 3).reshape(E, N, ndim)
    for e in range(E):
        np.testing.assert_allclose(cov[e], np.cov(flat[e].T), rtol=1e-9, atol=0)
    # get_param_std is the population's (ddof = 0), from two passes: its square is held to the bound that
    # tests/moments_bounds.py derives, delta^2 + (N + c) u (var + delta^2) with delta the bound of the mean (c = 7 covers
    # NumPy's std of a host chain as well as the device's fma).  On these data it is the tighter one of it and the
    # (N + 8) u var + (N u max|x|)^2 that stood here before: asserted, so that nothing is held to less than it was
    var_p = np.diagonal(ref['cov'], axis1=1, axis2=2) * (N - 1) / N
    mref = moments_reference(chain, E, c=7)
    assert mref['checked'].all()
    dstd2 = mref['dvar']
    assert (dstd2 <= (N + 8) * U * var_p + (N * U * np.abs(flat).max(axis=1)) ** 2).all()
    dcov = np.diagonal(ref['dcov'], axis1=1, axis2=2) * (N - 1) / N + 2 * U * var_p
    got = np.diagonal(cov, axis1=1, axis2=2) * (N - 1) / N
    assert (np.abs(got - std ** 2) <= dcov + dstd2).all()
    assert_moments_within(None, std, mref)
    lpf = lp.reshape(n, E, W // E).transpose(1, 0, 2).reshape(E, N)
    for e in range(E):
        i = np.argmax(lpf[e])
        assert best[e] == lpf[e, i]
        np.testing.assert_array_equal(theta[e], flat[e, i])
    again = logp_of(theta)
    assert (np.abs(again - best) <= 6e-12 * np.maximum(1.0, np.abs(best))).all(), (again, best)


@pytest.mark.parametrize('where', ['device', 'host'])
def test_model_methods(where):
    m = fitted_model(where)
    chain, lp = m.get_chain(**KW), m._sampler.get_log_prob(**KW)
    cov, corr = m.get_param_cov(**KW), m.get_param_corr(**KW)
    assert cov.shape == corr.shape == (m.ndim, m.ndim)
    theta, best = m.get_best_sample(**KW)
    assert theta.shape == (m.ndim,) and isinstance(best, float)
    check_layers(chain, lp, cov[None], corr[None], m.get_param_std(**KW)[None], theta[None],
                 np.array([best]), lambda t: np.atleast_1d(m.log_prob(t[0])), 1)
    flat = m.get_chain(flat=True, **KW)
    np.testing.assert_array_equal(m.get_param_cov(chain=flat), np.cov(flat.T))
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_param_cov(chain=flat, discard=5)
    with pytest.raises(ValueError, match='no samples'):
        m.get_param_cov(discard=120)
    with pytest.warns(UserWarning, match='No samples were discarded'):
        m.get_param_cov()
    with pytest.warns(UserWarning, match='No samples were discarded'):
        m.get_param_corr()
    with pytest.warns(UserWarning, match='No samples were discarded'):
        m.get_best_sample()


def test_model_device_and_host_chain_give_the_same_bits():
    d, h = fitted_model('device'), fitted_model('host')
    np.testing.assert_array_equal(d.get_chain(**KW), h.get_chain(**KW))
    np.testing.assert_array_equal(d.get_param_cov(**KW).view(np.uint64), h.get_param_cov(**KW).view(np.uint64))
    np.testing.assert_array_equal(d.get_best_sample(**KW)[0], h.get_best_sample(**KW)[0])
    assert d.get_best_sample(**KW)[1] == h.get_best_sample(**KW)[1]


@functools.lru_cache(maxsize=None)
def fitted_batch(where):
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    spectra = [bisip_amd.DataFiles()['SIP-K389175']] + [synthetic_columns(20, i) for i in range(2)]
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=16, nsteps=60, poly_deg=2)
    np.random.seed(5)
    b.fit(seed=11, chain=where)
    return b


@pytest.mark.parametrize('where', ['device', 'host'])
def test_spectra_batch_methods(where):
    b = fitted_batch(where)
    E, Wp = 3, 16
    chain, lp = b.get_chain(**KW), b.get_log_prob(**KW)              # (n, E, Wp, ndim), (n, E, Wp)
    n = chain.shape[0]
    cov, corr = b.get_param_cov(**KW), b.get_param_corr(**KW)
    assert cov.shape == corr.shape == (E, b.ndim, b.ndim)
    theta, best = b.get_best_sample(**KW)
    assert theta.shape == (E, b.ndim) and best.shape == (E,)
    check_layers(chain.reshape(n, E * Wp, b.ndim), lp.reshape(n, E * Wp), cov, corr,
                 b.get_param_std(**KW), theta, best, lambda t: b.log_prob(t[:, None, :])[:, 0], E)
    np.testing.assert_array_equal(b.gather(cov), cov)                 # a single process gets its input back
    with pytest.raises(ValueError, match='no samples'):
        b.get_param_cov(discard=60)


def test_spectra_batch_device_and_host_chain_give_the_same_bits():
    d, h = fitted_batch('device'), fitted_batch('host')
    np.testing.assert_array_equal(d.get_param_cov(**KW).view(np.uint64), h.get_param_cov(**KW).view(np.uint64))
    for a, c in zip(d.get_best_sample(**KW), h.get_best_sample(**KW)):
        np.testing.assert_array_equal(a, c)
