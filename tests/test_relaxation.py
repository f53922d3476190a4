"""The relaxation descriptors of PolynomialDecomposition on the host (bisip_amd.decomposition, "Relaxation
descriptors"): the RTD's peak and the cumulative relaxation times log_tau_q.  The definition in NumPy
(``rtd_descriptors``) and the library's row function on the CPU (bisip_rtd_descriptors_host -- the arithmetic the kernel
runs, tests/test_gpu_relaxation.py) against the long-double yardstick and the derived bound of
tests/relaxation_bounds.py, the cases whose answers are exact, and the checks the public methods make before any device
work."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from bisip_amd import decomposition
from bisip_amd.decomposition import DESCRIPTOR_NAMES, host_rtd_descriptors, rtd, rtd_descriptors
from conftest import ROOT
from fitted import fitted_on_host
from relaxation_bounds import assert_descriptors_within, descriptor_bounds, descriptors_yardstick
from test_decomposition import bounds, grid, prior_rows, tutorial_rows

Q = (0.1, 0.5, 0.9)
N_ROWS = 20000


def family(name):
    """(rows, log_tau) of the three families the definition was measured on, 20,000 rows each."""
    if name == 'box5':
        return prior_rows(np.random.default_rng(5), N_ROWS, 5), grid(64, -7.0, 3.0)
    if name == 'box4':
        return prior_rows(np.random.default_rng(4), N_ROWS, 4), grid(40)
    return tutorial_rows(np.random.default_rng(40), N_ROWS), grid(40)


def host_rows(rows, lt, q=Q):
    return host_rtd_descriptors(rows[None], lt, q)[0]


def test_names():
    assert DESCRIPTOR_NAMES() == DESCRIPTOR_NAMES(Q) == ('log_tau_peak', 'm_peak', 'log_tau_10', 'log_tau_50', 'log_tau_90')
    assert DESCRIPTOR_NAMES([0.025, 0.6, 1.0]) == ('log_tau_peak', 'm_peak', 'log_tau_2.5', 'log_tau_60', 'log_tau_100')
    import bisip_amd
    assert bisip_amd.rtd_descriptors is rtd_descriptors and bisip_amd.DESCRIPTOR_NAMES is DESCRIPTOR_NAMES


@pytest.mark.parametrize('name', ['box5', 'box4', 'tutorial'])
def test_definitions_meet_the_bounds(name):
    rows, lt = family(name)
    ys = descriptors_yardstick(rows, lt, Q)
    bound, fragile = descriptor_bounds(rows, lt, Q, ys)
    nan_share = 1.0 - ys['valid'].mean()
    assert nan_share == 0.0 if name == 'tutorial' else 0.0 < nan_share < 0.2       # the box has rows with no positive RTD
    for what, got in (('numpy', rtd_descriptors(rows, lt, Q)), ('host entry', host_rows(rows, lt))):
        assert got.shape == (N_ROWS, 5)
        worst, share = assert_descriptors_within(got, ys, bound, fragile, lt, f'{name}: {what}')
        print(f'{name}: {what}: worst error {worst:.2e}, fragile share {share:.2e}, NaN rows {nan_share:.3f}, '
              f'smallest c_k / total {float(ys["share"][ys["valid"]].min()):.2e}')


def test_degree_zero_is_exact():
    """a_0 = 1 on 10 points: g_l = l + 1 and total = 10, all exact.  t = 5 = g_4 gives x_4; q = 1 gives x_9; q = 0.1
    gives t = 1 = g_0: x_0; the peak of a constant RTD is its first point."""
    lt = grid(10)
    theta = np.array([1.0, 1.0])
    for f in (lambda t, q: rtd_descriptors(t, lt, q), lambda t, q: host_rows(t[None], lt, q)[0]):
        np.testing.assert_array_equal(f(theta, [0.5, 1.0, 0.1]), [lt[0], 1.0, lt[4], lt[9], lt[0]])
        # t = 4.5 lies half way between g_3 = 4 and g_4 = 5
        np.testing.assert_array_equal(f(theta, [0.45])[2:], [lt[3] + 0.5 * (lt[4] - lt[3])])
        for a0 in (0.0, -1.0):
            assert np.isnan(f(np.array([1.0, a0]), Q)).all()


def test_one_point_grid_gives_that_point():
    lt = np.array([-2.5])
    q = [0.01, 0.3, 1.0]
    rows = prior_rows(np.random.default_rng(1), 50, 3)
    for got in (rtd_descriptors(rows, lt, q), host_rows(rows, lt, q)):
        pos = rtd(rows, lt)[:, 0] > 0
        assert pos.any() and not pos.all()
        assert np.isnan(got[~pos]).all()
        np.testing.assert_array_equal(got[pos][:, [0, 2, 3, 4]], -2.5)


def test_inner_stretch():
    """m = 1 - x**2 on -2 ... 2 is positive strictly inside (-1, 1): every log_tau_q lies on that stretch and q = 1 gives
    its last positive point -- f = 1 there, and fma(1, x_k - x_{k-1}, x_{k-1}) is x_k up to the rounding of the step, an
    ulp of x_k; the first points, where c = 0, take nothing.  The sum to x_k is met AT x_k (the weight of a point lies on
    the cell that ends there), so the median of this even RTD is half a step below 0."""
    lt = np.linspace(-2.0, 2.0, 41)
    theta = np.array([1.0, 1.0, 0.0, -1.0])
    q = [1e-6, 0.1, 0.5, 0.9, 1.0]
    m = rtd(theta, lt)
    pos = np.flatnonzero(m > 0)
    assert pos[0] > 0 and pos[-1] < 40
    for got in (rtd_descriptors(theta, lt, q), host_rows(theta[None], lt, q)[0]):
        assert got[0] == 0.0 and got[1] == 1.0
        last, ulp = lt[pos[-1]], np.spacing(lt[pos[-1]])
        assert np.all(got[2:] > lt[pos[0] - 1]) and np.all(got[2:] <= last + ulp)
        assert abs(got[-1] - last) <= ulp
        assert abs(got[4] + 0.05) <= 1e-12
        assert np.all(np.diff(got[2:]) >= 0)


def test_nan_coefficient_gives_nan():
    lt = grid(40)
    rows = prior_rows(np.random.default_rng(2), 6, 4)
    rows[:, 1] = np.abs(rows[:, 1]) + 1.0
    clean = rtd_descriptors(rows, lt)
    for p in range(1, 6):
        bad = rows.copy()
        bad[p, p] = np.nan
        for got in (rtd_descriptors(bad, lt), host_rows(bad, lt)):
            assert np.isnan(got[p]).all()
            keep = np.arange(6) != p
            assert np.isfinite(got[keep]).all()
        np.testing.assert_array_equal(rtd_descriptors(bad, lt)[keep], clean[keep])


@pytest.mark.parametrize('P', [1, 4, 5])
def test_peak_is_the_largest_rtd_value(P):
    """m_peak is the largest of the Horner values and log_tau_peak its grid point: NumPy's against its own Horner exactly,
    the library's (fma) and the power form of ``rtd`` within the bound of m_l."""
    rng = np.random.default_rng(P)
    lt = grid(40)
    rows = prior_rows(rng, 500, P)
    a = rows[:, 1:]
    m = np.repeat(a[:, -1:], 40, axis=1)
    for p in range(P - 1, -1, -1):
        m = m * lt + a[:, p, None]
    got, lib = rtd_descriptors(rows, lt), host_rows(rows, lt)
    ok = ~np.isnan(got[:, 0])
    assert 0 < ok.sum() < 500
    np.testing.assert_array_equal(got[ok, 1], m.max(axis=1)[ok])
    np.testing.assert_array_equal(got[ok, 0], lt[m.argmax(axis=1)][ok])
    bm = bounds(rows, lt, 1.0)[1].max(axis=1).astype(np.float64)
    for other in (lib[:, 1], rtd(rows, lt).max(axis=1)):
        assert np.all(np.abs(other[ok] - got[ok, 1]) <= 2 * bm[ok])


def test_monotone_in_q():
    rows, lt = family('box5')
    q = [0.01, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0]
    for got in (rtd_descriptors(rows[:3000], lt, q), host_rows(rows[:3000], lt, q)):
        ok = ~np.isnan(got[:, 0])
        # t <= g_k = fl(g_{k-1} + c_k) allows t - g_{k-1} <= c_k + u total, so f <= (1 + u total / c_k)(1 + 2u), and the
        # step h is rounded: a value may pass x_k, and with it the next fraction's value, by h (u total / c_k + 4u) + u |x_k|
        c = np.where(rtd(rows[:3000], lt) > 0, rtd(rows[:3000], lt), np.inf)[ok]
        total = np.where(np.isfinite(c), c, 0.0).sum(axis=1)
        slack = np.max(np.diff(lt)) * 2 * 2.0 ** -53 * total / c.min(axis=1) + 8 * 2.0 ** -53 * np.max(np.abs(lt))
        assert np.all(np.diff(got[ok, 2:], axis=1) >= -slack[:, None])
        assert np.all(got[ok, 2] >= lt[0]) and np.all(got[ok, -1] <= lt[-1] + slack)
    # the order in which the fractions are given does not matter
    shuffled = [0.9, 0.01, 1.0, 0.5]
    a, b = host_rows(rows[:300], lt, shuffled), host_rows(rows[:300], lt, sorted(shuffled))
    np.testing.assert_array_equal(a[:, 2:][:, np.argsort(shuffled)].view(np.int64), b[:, 2:].view(np.int64))


def test_host_entry_reads_offset_and_stride():
    from bisip_amd import _hip
    from chain_harness import store
    lt = grid(40)
    x = prior_rows(np.random.default_rng(3), 4 * 6, 4).reshape(4, 6, 6)
    stored, off, stride = store(x, filler=np.nan)
    got = _hip.rtd_descriptors_host(stored, 4, stride, 2, 3, 6, lt, Q, offset=off)
    np.testing.assert_array_equal(got.view(np.int64), host_rtd_descriptors(x, lt, Q, n_ensembles=2).view(np.int64))
    with pytest.raises(ValueError, match='outside the chain'):
        _hip.rtd_descriptors_host(stored, 5, stride, 2, 3, 6, lt, Q, offset=off)


def test_abi_version_and_symbols(hip_lib):
    import __graft_entry__ as entry
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6          # symbols were only added
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in ('bisip_rtd_descriptors_dev', 'bisip_rtd_descriptors_host'):
        assert hasattr(hip_lib, name)
        assert name in exports and f'int {name}(' in header


def test_entry_point_argument_checks(hip_lib):
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    chain, lt, q, out = np.ones((1, 2, 3)), grid(4), np.array([0.5]), np.empty((1, 2, 10))
    p = lambda a: a.ctypes.data_as(dp)
    call = lambda n=1, stride=6, E=1, Wp=2, ndim=3, L=4, nq=1, c=chain: hip_lib.bisip_rtd_descriptors_host(
        None if c is None else p(c), n, stride, E, Wp, ndim, p(lt), L, p(q), nq, p(out))
    assert call() == 0
    for kw in (dict(nq=0), dict(nq=9), dict(L=0), dict(ndim=1), dict(ndim=17), dict(n=0), dict(E=0), dict(Wp=0),
               dict(stride=5), dict(c=None)):
        assert call(**kw) == -1, kw
        assert hip_lib.bisip_last_error()


@pytest.mark.parametrize('bad', [[], [0.1] * 9, [0.0, 0.5], [-0.1], [0.5, 1.0000001], [0.5, np.nan], [[0.1, 0.5]]])
def test_fractions_are_checked(bad):
    m = fitted_on_host()
    theta = np.array([1.0, 0.5, 0.0, 0.0])
    for f in (lambda: rtd_descriptors(theta, m.log_tau, bad), lambda: DESCRIPTOR_NAMES(bad),
              lambda: host_rtd_descriptors(theta[None, None], m.log_tau, bad), lambda: m.relaxation_descriptors(theta, q=bad),
              lambda: m.get_relaxation_mean(q=bad), lambda: m.get_relaxation_chain(q=bad),
              lambda: m.get_relaxation_percentile(50, q=bad), lambda: m.get_relaxation_hdi(q=bad)):
        with pytest.raises(ValueError, match='fraction'):
            f()


@pytest.mark.parametrize('bad', [[0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [1.0, np.nan], [], [[0.0, 1.0]]])
def test_grid_must_ascend(bad):
    theta = np.array([1.0, 0.5, 0.0])
    with pytest.raises(ValueError, match='strictly ascending'):
        rtd_descriptors(theta, bad)
    with pytest.raises(ValueError, match='strictly ascending'):
        host_rtd_descriptors(theta[None, None], bad)


def test_model_host_method():
    m = fitted_on_host()
    theta = m.get_chain(flat=True)
    got = m.relaxation_descriptors(theta, q=[0.5])
    assert got.shape == (theta.shape[0], 3) and m.relaxation_descriptors(theta[0]).shape == (5,)
    np.testing.assert_array_equal(got, rtd_descriptors(theta, m.log_tau, [0.5]))
    none = ~np.any(m.rtd(theta) > 0, axis=1)             # a_0 = 0.01 +- 0.01: some samples have no positive RTD
    assert 0 < none.sum() < none.size
    np.testing.assert_array_equal(np.isnan(got), np.broadcast_to(none[:, None], got.shape))


@pytest.mark.parametrize('method', ['get_relaxation_chain', 'get_relaxation_mean', 'get_relaxation_std',
                                    'get_relaxation_percentile', 'get_relaxation_hdi'])
def test_argument_checks(method):
    """The discard / thin / chain errors of get_integrating_mean, raised before any device work."""
    m = fitted_on_host()
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=20)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=5, thin=0)
    with pytest.raises(ValueError, match='Do not pass both'):
        f(chain=m.get_chain(flat=True), discard=5)
    with pytest.raises(ValueError, match='Flatten'):
        f(chain=m.get_chain())


@pytest.mark.parametrize('method', ['relaxation_descriptors', 'get_relaxation_chain', 'get_relaxation_mean',
                                    'get_relaxation_std', 'get_relaxation_percentile', 'get_relaxation_hdi'])
def test_spectra_batch_of_another_model_refuses(method):
    from bisip_amd import SpectraBatch
    b = SpectraBatch.__new__(SpectraBatch)       # the check comes before the device context is touched
    b.model, b._sampler = 'PeltonColeCole', None
    with pytest.raises(ValueError, match='belong to PolynomialDecomposition, not PeltonColeCole'):
        f = getattr(b, method)
        f(np.zeros((1, 2, 7))) if method == 'relaxation_descriptors' else f()


def test_signatures():
    import inspect
    from bisip_amd import PolynomialDecomposition, SpectraBatch
    sig = lambda c, m: str(inspect.signature(getattr(c, m)))
    assert sig(PolynomialDecomposition, 'get_relaxation_mean') == '(self, chain=None, q=(0.1, 0.5, 0.9), **kwargs)'
    assert sig(PolynomialDecomposition, 'get_relaxation_percentile') == \
        '(self, p=[2.5, 50, 97.5], chain=None, q=(0.1, 0.5, 0.9), **kwargs)'
    assert sig(PolynomialDecomposition, 'get_relaxation_hdi') == '(self, mass=0.95, chain=None, q=(0.1, 0.5, 0.9), **kwargs)'
    assert sig(SpectraBatch, 'get_relaxation_chain') == '(self, discard=0, thin=1, flat=False, q=(0.1, 0.5, 0.9))'
    assert sig(SpectraBatch, 'get_relaxation_percentile') == '(self, p=(2.5, 50, 97.5), discard=0, thin=1, q=(0.1, 0.5, 0.9))'
    assert sig(SpectraBatch, 'get_relaxation_hdi') == '(self, mass=0.95, discard=0, thin=1, q=(0.1, 0.5, 0.9))'
    assert decomposition.MAX_FRACTIONS == 8


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_row_function_under_asan_ubsan(tmp_path):
    """The row function is plain C++ in a header: a stand-alone program of its own runs it, every ndim, L and number of
    fractions on buffers of the exact size, under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / 'sanitize_rtd_descriptors'
    build = subprocess.run(['g++', '-std=gnu++17', '-O1', '-g', '-fno-omit-frame-pointer', '-ffp-contract=off',
                            '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe),
                            os.path.join(ROOT, 'tests', 'native', 'sanitize_rtd_descriptors.cpp')],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'sanitize_rtd_descriptors: ok' in run.stdout
