"""bisip_amd.fitquality on the host: the definitions against brute-force loops, the NumPy restatement of the fit-quality
kernel's order against the long-double definitions within the bound of tests/fit_quality_bounds.py -- on the inputs that
break a naive kernel too --, WAIC and compare_waic on hand-built arrays, the new entry points and the surface of the models
and of SpectraBatch."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from bisip_amd import fitquality as fq
from fit_quality_bounds import K_NUMPY, assert_all_within, data_for, inverse_variance, reference_and_bounds
from response_bounds import responses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definitions ------------------------------------------------------------------------------------------------
def test_definitions_against_loops():
    rng = np.random.default_rng(3)
    R, N = 7, 3
    Z = rng.normal(size=(R, 2, N))
    y = rng.normal(size=(2, N))
    err = rng.uniform(0.1, 2.0, size=(2, N))
    iv = fq.inverse_variance(err)
    q = fq.pointwise_q(Z, y, iv)
    ll = fq.pointwise_log_lik(Z, y, err)
    mean_q, var_q, lmeh = fq.fit_sums(q)
    assert q.shape == ll.shape == (R, 2, N) and mean_q.shape == var_q.shape == lmeh.shape == (2, N)
    for p in range(2):
        for j in range(N):
            assert iv[p, j] == float(1 / (np.longdouble(err[p, j]) * np.longdouble(err[p, j])))
            col = []
            for s in range(R):
                d = y[p, j] - Z[s, p, j]
                t = d * d
                assert q[s, p, j] == t * iv[p, j]
                assert ll[s, p, j] == pytest.approx(-0.5 * q[s, p, j] - math.log(err[p, j] ** 2), rel=1e-15)
                col.append(q[s, p, j])
            mean = sum(col) / R
            assert mean_q[p, j] == pytest.approx(mean, rel=1e-14)
            assert var_q[p, j] == pytest.approx(sum((c - mean) ** 2 for c in col) / (R - 1), rel=1e-13)
            assert lmeh[p, j] == pytest.approx(math.log(sum(math.exp(-c / 2) for c in col) / R), rel=1e-13)
    # the sum of the pointwise log-likelihoods is the reference's _log_likelihood
    sigma2 = err ** 2
    want = [-0.5 * np.sum((y - Z[s]) ** 2 / sigma2 + 2 * np.log(sigma2)) for s in range(R)]
    np.testing.assert_allclose(ll.sum(axis=(1, 2)), want, rtol=1e-13)
    # WAIC from the three sums is WAIC of the pointwise log-likelihoods
    a, b = fq.waic(ll), fq.waic_from_sums(var_q, lmeh, np.log(sigma2))
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-11, atol=1e-12, err_msg=k)
    one = fq.fit_sums(q[:1])
    assert np.isnan(one[1]).all() and (one[0] == q[0]).all()
    np.testing.assert_allclose(one[2], -q[0] / 2, rtol=1e-15)
    with pytest.raises(ValueError, match='2, N'):
        fq.pointwise_q(np.zeros((4, 3, 5)), 0.0, 1.0)


def test_waic_of_a_hand_built_array():
    ell = np.array([[-1.0, -2.0, -0.5, -3.0]] * 5)                    # five identical rows of four points
    w = fq.waic(ell)
    np.testing.assert_allclose(w['lppd'], ell[0], rtol=1e-15)
    assert (w['p_waic_i'] == 0).all() and w['p_waic'] == 0.0 and w['n_high'] == 0
    assert w['elpd_waic'] == pytest.approx(-6.5) and w['waic'] == pytest.approx(13.0)
    assert w['se'] == pytest.approx(math.sqrt(4 * np.var(ell[0])))
    # two rows, one point: l = log 1 and log 3 -> lppd = log 2, p_waic = var = (log 3)^2 / 2
    w = fq.waic(np.log(np.array([[1.0], [3.0]])))
    assert w['lppd'][0] == pytest.approx(math.log(2.0)) and w['p_waic'] == pytest.approx(math.log(3.0) ** 2 / 2)
    assert w['n_high'] == 1 and w['elpd_waic'] == pytest.approx(math.log(2.0) - math.log(3.0) ** 2 / 2)
    assert w['se'] == 0.0
    # per spectrum: leading axes stay
    v = np.array([[[0.4, 2.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]])
    b = fq.waic_from_sums(v, np.zeros((2, 2, 2)), np.full((2, 2, 2), 1.0))
    assert b['elpd_waic'].shape == (2,) and list(b['n_high']) == [1, 0]
    np.testing.assert_allclose(b['elpd_waic'], [-4.6, -4.0])
    np.testing.assert_allclose(b['p_waic'], [0.6, 0.0])


def test_dic_by_hand():
    d = fq.dic(-10.0, -8.5)
    assert d == dict(dic=23.0, p_d=3.0, mean_deviance=20.0, deviance_at_mean=17.0)
    d = fq.dic(np.array([-10.0, -1.0]), np.array([-8.5, -1.0]))
    np.testing.assert_array_equal(d['dic'], [23.0, 2.0])
    np.testing.assert_array_equal(d['p_d'], [3.0, 0.0])


def test_compare_waic():
    rng = np.random.default_rng(0)
    ll = {name: rng.normal(loc, 0.3, size=(50, 2, 6)) for name, loc in (('a', -1.0), ('b', -0.5), ('c', -2.0))}
    res = {name: fq.waic(v) for name, v in ll.items()}
    rows = fq.compare_waic(res)
    assert [r['name'] for r in rows] == ['b', 'a', 'c']
    assert [r['elpd_waic'] for r in rows] == sorted((r['elpd_waic'] for r in rows), reverse=True)
    assert rows[0]['d_elpd'] == 0.0 and rows[0]['d_se'] == 0.0
    for r in rows[1:]:
        assert r['d_elpd'] == pytest.approx(res['b']['elpd_waic'] - res[r['name']]['elpd_waic']) and r['d_elpd'] > 0
        diff = res[r['name']]['elpd_i'] - res['b']['elpd_i']
        assert r['d_se'] == pytest.approx(math.sqrt(12 * np.var(diff)))
        assert r['waic'] == res[r['name']]['waic'] and r['se'] == res[r['name']]['se']
    same = fq.compare_waic({'x': res['a'], 'y': res['a']})
    assert all(r['d_elpd'] == 0.0 and r['d_se'] == 0.0 for r in same)
    with pytest.raises(ValueError, match='shape'):
        fq.compare_waic({'a': res['a'], 'other': fq.waic(ll['a'][:, :, :5])})
    with pytest.raises(ValueError, match='nothing'):
        fq.compare_waic({})


# -- the device's order, restated -----------------------------------------------------------------------------------
# (E, rows, N): as tests/test_response.py -- rows on both sides of a run of 64 slots and of the 256 slots, one row, one
# above the segment minimum, two ragged segments and a third; E = 256 is the first count that takes one segment
SHAPES = [(1, 1, 4), (1, 63, 4), (1, 64, 4), (1, 65, 4), (3, 65, 5), (1, 255, 2), (1, 256, 2), (1, 257, 3), (1, 1024, 2),
          (1, 1025, 3), (3, 1025, 2), (1, 2500, 2), (256, 27, 2), (256, 1, 1)]


def check_ordered(Z, y, err, what, n_spectra=None):
    iv = inverse_variance(err)
    np.testing.assert_array_equal(iv, fq.inverse_variance(err))
    got = fq.ordered_fit_sums(Z, y, iv, n_spectra)
    ref = reference_and_bounds(Z, y, iv, n_spectra, K_NUMPY)
    worst = assert_all_within(got, ref, what)
    print(f'{what}: mean_q, var_q, lmeh at most {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f} of their bounds')
    return got, ref


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ordered_sums_against_the_definition(shape):
    E, R, N = shape
    Z = responses(E, R, N)
    y, err = data_for(Z)
    (mean_q, var_q, lmeh), ref = check_ordered(Z, y, err, str(shape))
    assert mean_q.shape == var_q.shape == lmeh.shape == (E, 2, N)
    assert (ref['q_max'] < 1e4).all()                         # q of order 1: else the inputs would be wrong
    if R > 1:
        assert (var_q >= 0).all()
        d = fq.fit_sums(fq.pointwise_q(np.moveaxis(Z, 1, 0), y, inverse_variance(err)))
        np.testing.assert_allclose(mean_q, d[0], rtol=1e-11)
        np.testing.assert_allclose(lmeh, d[2], rtol=1e-11, atol=1e-13)
        assert (var_q[E - 1, :, 0] == 0.0).all()              # the response that does not vary (response_bounds.responses)
    else:
        assert np.isnan(var_q).all()
    if E == 1:
        for a, b in zip(fq.ordered_fit_sums(Z[0], y[0], inverse_variance(err[0])), (mean_q, var_q, lmeh)):
            np.testing.assert_array_equal(a, b)


def special_inputs(which, R=700, N=3):
    """Z (1, R, 2, N), y, err of one spectrum whose q breaks a naive kernel at point (0, 1); elsewhere q is of order 1."""
    Z = responses(1, R, N, seed=5)
    y, err = data_for(Z, seed=5)
    if which == 'all above 1500':                 # the error of one point shrunk: exp(-q / 2) underflows to 0
        y[0, 0, 1] = Z[0, :, 0, 1].min() - 0.1
        err[0, 0, 1] = 1e-3
    elif which == 'first row far out':            # a shift by the first row overflows: exp(+750)
        y[0, 0, 1] = np.median(Z[0, :, 0, 1])
        err[0, 0, 1] = 1e-3 * np.abs(y[0, 0, 1])
        Z[0, 0, 0, 1] = y[0, 0, 1] + 50 * err[0, 0, 1]
    elif which == 'decreasing':                   # q falls from row to row: a rescale at every row of every slot
        Z[0, :, 0, 1] = y[0, 0, 1] + err[0, 0, 1] * np.linspace(9.0, 0.5, R)
    elif which == 'all rows equal':
        Z[0, :] = Z[0, 0]
    return Z, y, err


def test_every_q_above_1500():
    Z, y, err = special_inputs('all above 1500')
    (mean_q, var_q, lmeh), ref = check_ordered(Z, y, err, 'q > 1500')
    assert ref['q_min'][0, 0, 1] > 1500                              # a condition on the input
    assert np.isfinite(lmeh).all() and lmeh[0, 0, 1] < -750
    with np.errstate(all='ignore'):
        assert np.log(np.mean(np.exp(-fq.pointwise_q(Z[0], y[0], inverse_variance(err[0])) / 2), axis=0))[0, 1] == -np.inf


def test_first_row_far_out():
    Z, y, err = special_inputs('first row far out')
    (mean_q, var_q, lmeh), ref = check_ordered(Z, y, err, 'first row far out')
    q = fq.pointwise_q(Z[0], y[0], inverse_variance(err[0]))[:, 0, 1]
    assert q[0] - ref['q_min'][0, 0, 1] > 1500                       # a condition on the input
    assert np.isfinite(lmeh).all()


def test_q_decreasing_along_every_slot():
    Z, y, err = special_inputs('decreasing')
    q = fq.pointwise_q(Z[0], y[0], inverse_variance(err[0]))[:, 0, 1]
    assert (np.diff(q) < 0).all()
    check_ordered(Z, y, err, 'decreasing')


def test_all_rows_equal():
    Z, y, err = special_inputs('all rows equal')
    (mean_q, var_q, lmeh), ref = check_ordered(Z, y, err, 'all rows equal')
    q0 = fq.pointwise_q(Z[0, 0], y[0], inverse_variance(err[0]))
    assert (var_q == 0.0).all() and (mean_q[0] == q0).all()
    assert (np.abs(lmeh[0] - (-q0 / 2)) <= ref['dlmeh'][0].astype(np.float64)).all()


def test_a_nan_row_stays_in_its_spectrum():
    Z = responses(3, 300, 4)
    y, err = data_for(Z)
    clean = fq.ordered_fit_sums(Z, y, inverse_variance(err))
    Z[1, 17] = np.nan
    got = fq.ordered_fit_sums(Z, y, inverse_variance(err))
    for a, b in zip(got, clean):
        assert np.isnan(a[1]).all()
        np.testing.assert_array_equal(a[[0, 2]], b[[0, 2]])
    Z[1, 17] = Z[1, 16]
    Z[1, 0] = np.nan                                                  # the row of the shift itself
    assert all(np.isnan(a[1]).all() and np.isfinite(a[[0, 2]]).all() for a in fq.ordered_fit_sums(Z, y, inverse_variance(err)))


# -- plumbing -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ('bisip_fit_quality_workspace', 'bisip_fit_quality_dev')


def test_entry_points_exist(hip_lib):
    import __graft_entry__ as entry
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in NEW_ENTRIES:
        assert hasattr(hip_lib, name) and name in _hip.SYMBOLS
        assert re.search(r'\b%s\(' % name, header)
    assert _hip.SYMBOLS['bisip_fit_quality_dev'][1] == [
        c for c in _hip.SYMBOLS['bisip_response_moments_dev'][1][:7]] + [_hip.ctypes.c_void_p] * 4 + [
        _hip.ctypes.c_int64, _hip.ctypes.c_void_p]
    assert _hip.SYMBOLS['bisip_fit_quality_workspace'] == _hip.SYMBOLS['bisip_response_moments_workspace']
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6
    assert _hip.RESPONSE_KINDS == {'ri': 0, 'pa': 1}             # an entry point of its own, not a third kind
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    assert 'bisip_*' in exports                                # every bisip_ symbol leaves the library
    for method in ('fit_quality_workspace', 'fit_quality_dev'):
        assert callable(getattr(_hip.HipContext, method))


def test_signatures():
    import bisip_amd
    from bisip_amd.summaries import DeviceChainSummaries
    sig = lambda f: str(inspect.signature(f))
    assert sig(DeviceChainSummaries.fit_quality) == '(self, discard=0, thin=1)'
    assert sig(fq.device_fit_quality) == '(view, ctx, first_spectrum=0)'
    assert sig(fq.ordered_fit_sums) == '(Z, y, iv, n_spectra=None)'
    for cls in (bisip_amd.PolynomialDecomposition, bisip_amd.PeltonColeCole, bisip_amd.Dias2000, bisip_amd.Shin2015):
        assert issubclass(cls, fq.ModelFitQuality)
        for name in ('get_pointwise_misfit', 'get_waic', 'get_dic'):
            assert sig(getattr(cls, name)) == '(self, chain=None, **kwargs)'
            assert name not in vars(cls) and name not in vars(bisip_amd.utils.utils)
    B = bisip_amd.SpectraBatch
    assert issubclass(B, fq.BatchFitQuality)
    for name in ('get_pointwise_misfit', 'get_waic', 'get_dic'):
        assert sig(getattr(B, name)) == '(self, discard=0, thin=1)' and name not in vars(B)
    assert 'compare_waic' in fq.__all__ and not hasattr(bisip_amd, 'compare_waic')


def test_errors_of_an_unfitted_model_and_of_chain_with_discard():
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389175']
    m = bisip_amd.PeltonColeCole(path, n_modes=1, nwalkers=8, nsteps=5)
    calls = (m.get_pointwise_misfit, m.get_waic, m.get_dic)
    for call in calls:
        with pytest.raises(AssertionError, match='not fitted'):
            call()
    chain = np.tile(0.5 * (m.param_bounds[0] + m.param_bounds[1]), (6, 1))
    for call in calls:
        with pytest.raises(ValueError, match='Do not pass both'):
            call(chain=chain, discard=2)
        with pytest.raises(ValueError, match='Flatten chain'):
            call(chain=chain.reshape(3, 2, -1))
