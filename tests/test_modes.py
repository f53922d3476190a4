"""bisip_amd.modes on the CPU: the ordering of the modes of a Cole-Cole row against a brute-force statement of it, the host
entry point (bisip_mode_order_host, the row function the kernel shares) against the NumPy definition bit for bit, the two
relaxation times against the long-double yardstick within the bound of tests/mode_bounds.py and against known answers that pin
their formulas, the edge and refusal behaviour, the evidence over one labelling against targets of known evidence, and the row
function under AddressSanitizer + UBSan in a program of its own."""
import functools
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import mode_bounds as mb
from bisip_amd import evidence as ev
from bisip_amd import modes
from chain_harness import store
from conftest import ROOT

KS = (1, 2, 3, 4, 5)
BYS = ('m', 'log_tau', 'c')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits_or_nan(got, want):
    """The same bits, but for a NaN: there a NaN (which NaN an addition of NaNs or of opposite infinities gives is the
    machine's: IEEE leaves the sign and the payload open)."""
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])


def key_before(a, b):
    """The order of the definition on two keys: -1, 0 (a tie), 1."""
    less = lambda x, y: x < y or (x == x and y != y)
    return -1 if less(a, b) else 1 if less(b, a) else 0


def brute_force_perm(key):
    """The stable order of the keys of one row, by comparisons alone (list.sort is stable)."""
    return sorted(range(len(key)), key=functools.cmp_to_key(lambda i, j: key_before(key[i], key[j])))


def tied_rows(rng, n, K):
    """Rows of the default box whose keys come from a handful of values: ties in every group."""
    x = mb.box_rows(rng, n, K)
    pick = rng.integers(0, 3, (n, 3 * K))
    x[:, 1:] = np.where(rng.random((n, 3 * K)) < 0.6, pick * 0.25, x[:, 1:])
    return x


def hostile_rows(K, by):
    """Rows whose key group holds ties, signed zeros, infinities, one NaN, all NaN; one row with a NaN in another group."""
    g = modes.KEY_GROUPS[by]
    x = mb.box_rows(np.random.default_rng(K), 8, K)
    key = x[:, 1 + g * K:1 + (g + 1) * K]              # (a view)
    key[0] = 0.5
    key[1] = [(-0.0, 0.0)[j % 2] for j in range(K)]
    key[2, 0] = np.inf
    key[3, -1] = -np.inf
    key[4, 0] = np.nan
    key[5] = np.nan
    key[6] = [(np.inf, np.nan, -np.inf, 0.0, -0.0)[j % 5] for j in range(K)]
    other = (g + 1) % 3
    x[7, 1 + other * K] = np.nan
    return x


# -- ordering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
def test_order_modes_against_brute_force(K):
    for by in BYS:
        g = modes.KEY_GROUPS[by]
        x = np.concatenate([tied_rows(np.random.default_rng([K, g]), 300, K), hostile_rows(K, by)])
        o, perm, moved = modes.order_modes(x, K, by), modes.mode_permutation(x, K, by), modes.modes_moved(x, K, by)
        assert o.shape == x.shape and perm.shape == (x.shape[0], K)
        np.testing.assert_array_equal(bits(o[:, 0]), bits(x[:, 0]))
        for r in range(x.shape[0]):
            want = brute_force_perm(x[r, 1 + g * K:1 + (g + 1) * K])
            assert perm[r].tolist() == want                                     # stable: ties keep their order
            for grp in range(3):                                                # whole modes move, bits and all
                np.testing.assert_array_equal(bits(o[r, 1 + grp * K:1 + (grp + 1) * K]), bits(x[r, 1 + grp * K + np.array(want)]))
            k = o[r, 1 + g * K:1 + (g + 1) * K]
            assert all(key_before(k[j], k[j + 1]) <= 0 for j in range(K - 1))    # non-decreasing
            assert moved[r] == (want != list(range(K)))
        assert K == 1 or 0 < moved.sum() < moved.size


def test_hostile_keys_in_words():
    x = np.array([1.0, 0.1, 0.2, 0.3, np.nan, np.inf, -np.inf, 0.7, 0.8, 0.9])
    np.testing.assert_array_equal(modes.order_modes(x, 3), [1.0, 0.3, 0.2, 0.1, -np.inf, np.inf, np.nan, 0.9, 0.8, 0.7])
    x = np.array([1.0, 0.1, 0.2, 0.0, -0.0, 0.7, 0.8])
    assert not modes.modes_moved(x, 2) and not modes.modes_moved(x[[0, 1, 2, 4, 3, 5, 6]], 2)      # signed zeros tie
    x = np.array([1.0, 0.1, 0.2, np.nan, np.nan, 0.7, 0.8])
    assert not modes.modes_moved(x, 2) and modes.modes_moved(x, 2, 'c') == False and modes.modes_moved(x[[0, 2, 1, 3, 4, 5, 6]], 2, 'm')


def test_one_mode_orders_nothing():
    x = np.concatenate([mb.box_rows(np.random.default_rng(1), 50, 1), hostile_rows(1, 'log_tau')])
    for by in BYS:
        np.testing.assert_array_equal(bits(modes.order_modes(x, 1, by)), bits(x))
        assert not modes.modes_moved(x, 1, by).any()
        o, d, mv = modes.host_mode_order(x[None], 1, by)
        np.testing.assert_array_equal(bits(o[0]), bits(x))
        assert not mv.any() and d.shape == (1, x.shape[0], 3)
    modes.check_exchangeable(mb.default_bounds(1) + [[0.0], [1.0]], 1)


@pytest.mark.parametrize('K', KS)
def test_host_entry_point_is_the_numpy_definition(K):
    """Behind an offset, a stride and padding, for every key group and every combination of asked outputs: ordered, moved and
    m_total bit for bit; the relaxation times within the bound (the C library's log1p against NumPy's)."""
    from bisip_amd import _hip
    n, E, Wp, ndim = 4, 2, 3, 1 + 3 * K
    for by in BYS:
        g = modes.KEY_GROUPS[by]
        x = np.concatenate([tied_rows(np.random.default_rng([K, g, 5]), n * E * Wp - 8, K), hostile_rows(K, by)]).reshape(n, E * Wp, ndim)
        stored, off, stride = store(x, filler=np.nan)
        wo, wd, wm = modes.order_modes(x, K, by), modes.mode_descriptors(x, K, by), modes.modes_moved(x, K, by)
        for asked in itertools.product((False, True), repeat=3):
            if not any(asked):
                with pytest.raises(ValueError, match='no output asked for'):
                    _hip.mode_order_host(stored, n, stride, E, Wp, K, g, *asked, offset=off)
                continue
            o, d, mv = _hip.mode_order_host(stored, n, stride, E, Wp, K, g, *asked, offset=off)
            assert [a is not None for a in (o, d, mv)] == list(asked)
            if o is not None:
                np.testing.assert_array_equal(bits(o), bits(wo))
            if mv is not None:
                assert mv.dtype == bool
                np.testing.assert_array_equal(mv, wm)
            if d is not None:
                same_bits_or_nan(d[..., 0], wd[..., 0])
                np.testing.assert_array_equal(np.isfinite(d), np.isfinite(wd))
                np.testing.assert_array_equal(np.isnan(d), np.isnan(wd))
        same = modes.host_mode_order(x, K, by, n_ensembles=E)
        np.testing.assert_array_equal(bits(same[0]), bits(wo))
        with pytest.raises(ValueError, match='outside the chain'):
            _hip.mode_order_host(stored, n + 1, stride, E, Wp, K, g, offset=off)


# -- the bound of the two relaxation times -----------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
def test_relaxation_times_within_the_bound(K):
    for name, rows in mb.families(K, 20000 // K).items():
        own = mb.log1p_own_error(rows, K)
        assert own <= mb.LOG1P_OWN, f'{name}: NumPy\'s own log1p error {own:.3e} is above the figure written down'
        for by in BYS:
            worst_np = mb.assert_within(modes.mode_descriptors(rows, K, by), rows, K, by, f'NumPy K={K} {name} by {by}')
            host = modes.host_mode_order(rows[None], K, by, ordered=False, moved=False)[1][0]
            worst = mb.assert_within(host, rows, K, by, f'host K={K} {name} by {by}')
        print(f'K={K} {name}: own log1p error {own:.3e}; of the bound: NumPy {worst_np:.3f}, host entry point {worst:.3f}')


def test_the_figure_written_down_is_the_measured_one():
    """LOG1P_OWN over the families and seeds mode_bounds.py names: not above it, and not below it by more than its rounding."""
    worst = max(mb.log1p_own_error(rows, K) for seed in range(4) for K in (1, 5)
                for rows in mb.families(K, 200000 // K, seed).values())
    print(f'NumPy\'s own worst relative log1p error: {worst:.4e}')
    assert 1.0e-16 <= worst <= mb.LOG1P_OWN == 1.25e-16 and mb.FACTOR == 16


# -- known answers that pin the two formulas -----------------------------------------------------------------------------------
def pelton(theta, w):
    """Z of one-mode Pelton rows theta (n, 4) at w (N,), complex (n, N): r0 [1 - m (1 - 1 / (1 + (i w tau)^c))]."""
    r0, m, lt, c = (theta[:, k, None] for k in range(4))
    X = np.exp(c * (np.log(w) + lt) + 1j * c * np.pi / 2)
    return r0 * (1 - m * (1 - 1 / (1 + X)))


def interior_rows(rng, n):
    return rng.uniform([0.9, 0.1, -12.0, 0.2], [1.1, 0.9, 2.0, 0.9], (n, 4))


def test_cole_cole_conversion():
    """1 / Z of the Pelton row is the conductivity-form Cole-Cole model with tau_cc of mode_descriptors, on 64 frequencies."""
    theta = interior_rows(np.random.default_rng(17), 16)
    d = modes.mode_descriptors(theta, 1)
    w = np.exp(np.linspace(np.log(1e-3), np.log(1e6), 64))
    r0, m, c = theta[:, 0, None], theta[:, 1, None], theta[:, 3, None]
    Xcc = np.exp(c * (np.log(w) + d[:, 1, None]) + 1j * c * np.pi / 2)
    sigma = (1 / r0) * (1 + m / (1 - m) * (1 - 1 / (1 + Xcc)))
    got = 1 / pelton(theta, w)
    assert np.max(np.abs(got - sigma) / np.abs(sigma)) <= 1e-12
    np.testing.assert_array_equal(d[:, 0], theta[:, 1])                          # m_total of one mode is m


def test_phase_peak():
    """-phase of the model is largest at the grid point nearest w = exp(-log_tau_peak): 20,001 log-spaced frequencies."""
    theta = interior_rows(np.random.default_rng(18), 32)
    d = modes.mode_descriptors(theta, 1)
    logw = np.linspace(-12.0, 32.0, 20001)
    phase = -np.angle(pelton(theta, np.exp(logw)))
    assert np.all((-d[:, 2] > logw[100]) & (-d[:, 2] < logw[-100]))
    np.testing.assert_array_equal(np.argmax(phase, axis=1), np.argmin(np.abs(logw[None, :] + d[:, 2, None]), axis=1))
    np.testing.assert_allclose(d[:, 2], 0.5 * (theta[:, 2] + d[:, 1]), rtol=0, atol=1e-14)     # the geometric mean of the two


# -- edge behaviour and interface ----------------------------------------------------------------------------------------------
def test_box_edges_give_what_ieee_gives():
    x = np.array([[1.0, 1.0, 0.5, -3.0, -1.0, 0.5, 0.5],       # m = 1: log1p(-1) = -inf
                  [1.0, 0.5, 0.5, -3.0, -1.0, 0.0, 0.5],       # c = 0: l / 0 = -inf
                  [1.0, 0.0, 0.5, -3.0, -1.0, 0.0, 0.5],       # m = 0 and c = 0: -0 / 0 = NaN
                  [1.0, 0.2, 0.5, -3.0, -1.0, 0.5, 0.5]])
    want_first = [-np.inf, -np.inf, np.nan, -3.0 + np.log1p(-0.2) / 0.5]
    for d in (modes.mode_descriptors(x, 2), modes.host_mode_order(x[None], 2)[1][0]):
        np.testing.assert_array_equal(d[:, 1], want_first)
        np.testing.assert_array_equal(d[:3, 3], want_first[:3])
        assert np.isfinite(d[:, [0, 2, 4]]).all()
    d = modes.mode_descriptors(x, 2)
    with np.errstate(invalid='ignore'):
        assert np.isneginf(d[[0, 1, 3], 1].mean()) and np.isnan(d[:, 1].mean()) and np.isfinite(d[:, 2].mean())


def cole_cole(n_modes=2, **kw):
    import bisip_amd
    return bisip_amd.PeltonColeCole(bisip_amd.DataFiles()['SIP-K389175'], n_modes=n_modes, **kw)


def test_bounds_that_are_not_exchangeable_are_refused():
    m = cole_cole(3)
    theta = mb.box_rows(np.random.default_rng(2), 5, 3)
    np.testing.assert_array_equal(m.order_modes(theta), modes.order_modes(theta, 3))
    np.testing.assert_array_equal(m.mode_descriptors(theta, by='c'), modes.mode_descriptors(theta, 3, 'c'))
    assert m.order_modes(theta[0]).shape == (10,) and m.mode_descriptors(theta[0]).shape == (7,)
    m.params['c3'] = [0.0, 0.9]
    m.params['log_tau2'] = [-10, 5]
    for f in (lambda: m.order_modes(theta), lambda: m.mode_descriptors(theta), lambda: m.get_ordered_mean(),
              lambda: m.get_mode_chain(), lambda: m.get_mode_switch_rate(), lambda: m.get_evidence(order_modes='log_tau')):
        with pytest.raises(ValueError, match='not exchangeable: the bounds of log_tau2 '):
            f()
    with pytest.raises(ValueError, match='the bounds of c2 '):
        modes.check_exchangeable(np.array([[0.9, 0, 0, -15, -15, 0, 0.1], [1.1, 1, 1, 5, 5, 1, 1]]), 2)
    one = cole_cole(1)
    one.params['log_tau1'] = [-10, 5]
    assert one.order_modes(np.array([1.0, 0.5, -3.0, 0.5])).shape == (4,)          # K = 1: nothing to exchange
    with pytest.raises(ValueError, match="by must be 'log_tau', 'm' or 'c'"):
        cole_cole(2).order_modes(theta[:, :7], by='tau')
    with pytest.raises(ValueError, match='7 values'):
        modes.order_modes(theta, 2)
    with pytest.raises(ValueError, match='out of range'):
        modes.MODE_NAMES(6)
    assert modes.MODE_NAMES(2) == ('m_total', 'log_tau_cc1', 'log_tau_cc2', 'log_tau_peak1', 'log_tau_peak2')


def test_other_models_have_no_modes_to_order():
    import bisip_amd
    m = bisip_amd.Dias2000(bisip_amd.DataFiles()['SIP-K389175'])
    assert not hasattr(m, 'get_ordered_mean') and not hasattr(bisip_amd.PolynomialDecomposition, 'get_mode_mean')
    with pytest.raises(ValueError, match='order_modes belongs to PeltonColeCole'):
        m.get_evidence(order_modes='log_tau')


BATCH_METHODS = ['order_modes', 'mode_descriptors'] + [f'get_{a}_{b}' for a in ('ordered', 'mode')
                                                       for b in ('chain', 'mean', 'std', 'percentile', 'hdi')] + ['get_mode_switch_rate']


@pytest.mark.parametrize('method', BATCH_METHODS + ['get_evidence'])
def test_spectra_batch_of_another_model_refuses(method):
    from bisip_amd import SpectraBatch
    b = SpectraBatch.__new__(SpectraBatch)       # the check comes before the device context is touched
    b.model, b._sampler, b.n_modes = 'PolynomialDecomposition', object(), 1
    if method == 'get_evidence':
        with pytest.raises(ValueError, match='order_modes belongs to PeltonColeCole'):
            b.get_evidence(order_modes='log_tau')
        return
    with pytest.raises(ValueError, match='belong to PeltonColeCole, not PolynomialDecomposition'):
        f = getattr(b, method)
        f(np.zeros((1, 2, 7))) if method in ('order_modes', 'mode_descriptors') else f()


def test_signatures_and_exports():
    import inspect
    import bisip_amd
    from bisip_amd import PeltonColeCole, SpectraBatch
    sig = lambda c, m: str(inspect.signature(getattr(c, m)))
    assert sig(PeltonColeCole, 'order_modes') == "(self, theta, by='log_tau')"
    assert sig(PeltonColeCole, 'get_ordered_mean') == sig(PeltonColeCole, 'get_mode_std') == "(self, chain=None, by='log_tau', **kwargs)"
    assert sig(PeltonColeCole, 'get_mode_percentile') == "(self, p=[2.5, 50, 97.5], chain=None, by='log_tau', **kwargs)"
    assert sig(PeltonColeCole, 'get_ordered_hdi') == "(self, mass=0.95, chain=None, by='log_tau', **kwargs)"
    assert sig(PeltonColeCole, 'get_mode_switch_rate') == "(self, by='log_tau', chain=None, **kwargs)"
    assert sig(SpectraBatch, 'get_ordered_chain') == sig(SpectraBatch, 'get_mode_chain') == "(self, discard=0, thin=1, flat=False, by='log_tau')"
    assert sig(SpectraBatch, 'get_mode_percentile') == "(self, p=(2.5, 50, 97.5), discard=0, thin=1, by='log_tau')"
    assert sig(SpectraBatch, 'get_mode_switch_rate') == "(self, by='log_tau', discard=0, thin=1)"
    assert 'order_modes=None' in sig(PeltonColeCole, 'get_evidence') and 'order_modes=None' in sig(SpectraBatch, 'get_evidence')
    assert 'order=None' in str(inspect.signature(ev.bridge_evidence)) and 'order=None' in str(inspect.signature(ev.device_evidence))
    assert bisip_amd.order_modes is modes.order_modes and bisip_amd.mode_descriptors is modes.mode_descriptors
    assert bisip_amd.MODE_NAMES is modes.MODE_NAMES and modes.MAX_MODES == 5 and modes.KEY_GROUPS == {'m': 0, 'log_tau': 1, 'c': 2}
    for cls in (bisip_amd.PolynomialDecomposition, PeltonColeCole, bisip_amd.Dias2000):
        assert cls._decomposition_samples is bisip_amd.Inversion._decomposition_samples


def test_abi_version_and_symbols(hip_lib):
    import __graft_entry__ as entry
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6          # symbols were only added
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in ('bisip_mode_order_dev', 'bisip_mode_order_host'):
        assert hasattr(hip_lib, name)
        assert name in exports and f'int {name}(' in header


def test_entry_point_argument_checks(hip_lib):
    """Both entry points refuse the same arguments with the same texts, the device one before it touches the device."""
    import ctypes
    chain, o, d, mv = np.ones((1, 2, 7)), np.empty((1, 2, 7)), np.empty((1, 2, 5)), np.empty((1, 2), dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def host(n=1, stride=14, E=1, Wp=2, K=2, g=1, c=chain, outs=(o, d, mv)):
        dp, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte)
        cast = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return hip_lib.bisip_mode_order_host(cast(c, dp), n, stride, E, Wp, K, g, cast(outs[0], dp), cast(outs[1], dp), cast(outs[2], bp))

    def dev(n=1, stride=14, E=1, Wp=2, K=2, g=1, c=chain, outs=(o, d, mv)):
        return hip_lib.bisip_mode_order_dev(p(c), n, stride, E, Wp, K, g, p(outs[0]), p(outs[1]), p(outs[2]), None)

    assert host() == 0 and host(outs=(None, None, mv)) == 0 and host(outs=(o, None, None)) == 0
    texts = {}
    too_many = dict(E=1 << 20, Wp=1 << 20, stride=1 << 62)
    for kw in (dict(K=0), dict(K=6), dict(g=-1), dict(g=3), dict(n=0), dict(E=0), dict(Wp=0), dict(stride=13), dict(c=None),
               dict(outs=(None, None, None)), too_many):
        for call in (host, dev):
            assert call(**kw) == (-4 if kw is too_many else -1), kw           # BISIP_EUNSUPPORTED, BISIP_EINVAL
            texts.setdefault(str(kw), []).append(hip_lib.bisip_last_error())
    assert all(t[0] == t[1] and t[0] for t in texts.values())
    assert b'n_modes=6 out of range [1, 5]' in texts[str(dict(K=6))][0] and b'no output asked for' in texts[str(dict(outs=(None, None, None)))][0]
    assert b'exceed 2^31' in texts[str(dict(E=1 << 20, Wp=1 << 20, stride=1 << 62))][0]


# -- the evidence over one labelling ------------------------------------------------------------------------------------------
FAMILIES = {'K=2 sep=1': (2, 1.0), 'K=2 sep=3': (2, 3.0), 'K=3 sep=2': (3, 2.0)}
SEEDS = range(24)
SD, LOG_Z = 0.4, 1.75


def symmetric_target(K, sep):
    """A permutation-symmetric mixture of K! normals (sd 0.4) of ndim = 1 + 3K whose mode means lie ``sep`` apart in log_tau:
    ``(draw(rng, shape) -> rows, logp(theta))`` with ``integral exp(logp) = exp(LOG_Z)``."""
    ndim = 1 + 3 * K
    perms = np.array(list(itertools.permutations(range(K))))
    means = np.zeros((len(perms), ndim))
    means[:, 1 + K:1 + 2 * K] = perms * sep

    def draw(rng, shape):
        pick = rng.integers(0, len(perms), shape)
        return means[pick] + SD * rng.normal(size=shape + (ndim,))

    def logp(theta):
        z = (np.asarray(theta)[..., None, :] - means) / SD
        e = -0.5 * (z * z).sum(axis=-1)
        top = e.max(axis=-1)
        lse = top + np.log(np.exp(e - top[..., None]).sum(axis=-1))
        return lse - math.log(len(perms)) - ndim * (math.log(SD) + 0.5 * math.log(2 * math.pi)) + LOG_Z
    return draw, logp


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_ordered_evidence_of_a_symmetric_mixture(family):
    """240 iid samples x 16 walkers, ``neff=None``: the estimate over the ordered labelling plus log K! against the known
    evidence, by the rule of tests/test_evidence.py over 24 seeds: every error within 4 reported standard errors, their rms
    within a factor 2 of the rms standard error."""
    K, sep = FAMILIES[family]
    draw, logp = symmetric_target(K, sep)
    errors, ses, its = [], [], []
    for seed in SEEDS:
        x = draw(np.random.default_rng([seed, 11]), (240, 16))
        res = ev.bridge_evidence(x, logp(x), logp, seed=seed, neff=None, order=(K, 'log_tau'))
        assert res['log_symmetry'] == math.log(math.factorial(K)) and list(res)[-1] == 'log_symmetry'
        assert res['log_evidence'] == res['log_ml'] and (res['frac_outside'] > 0 or sep > 1)
        errors.append(res['log_ml'] - LOG_Z)
        ses.append(res['se'])
        its.append(res['iterations'])
    errors, ses = np.array(errors), np.array(ses)
    worst, ratio = (np.abs(errors) / ses).max(), np.sqrt(np.mean(errors ** 2)) / np.sqrt(np.mean(ses ** 2))
    print(f'{family}: worst |error| / se {worst:.2f}, rms error / rms se {ratio:.2f}, rms se {np.sqrt(np.mean(ses ** 2)):.3e}, '
          f'passes at most {max(its)}')
    assert worst <= 4 and 0.5 <= ratio <= 2 and max(its) < 100


def test_ordered_evidence_masks_the_draws_and_orders_the_samples():
    """The same estimate from the existing bridge_evidence with the samples ordered and the draws masked by hand."""
    K = 2
    draw, logp = symmetric_target(K, 1.0)
    x = draw(np.random.default_rng(3), (120, 8))
    res = ev.bridge_evidence(x, logp(x), logp, seed=5, neff=None, order=(K, 'log_tau'))
    masked = lambda t: np.where(modes.modes_moved(t, K), -np.inf, logp(t))
    by_hand = ev.bridge_evidence(modes.order_modes(x, K), logp(x), masked, seed=5, neff=None)
    assert res['log_ml'] == by_hand['log_ml'] + math.log(2) and res['se'] == by_hand['se']
    assert res['frac_outside'] == by_hand['frac_outside'] and res['iterations'] == by_hand['iterations']
    np.testing.assert_array_equal(res['proposal_mean'], by_hand['proposal_mean'])


def test_without_order_nothing_changes():
    """``order=None``: the keys and the bits of the estimate restated from the module's own pieces, for a Gaussian of d = 7."""
    from bisip_amd.covariance import flat_cov
    d, n, Wp = 7, 250, 8
    rng = np.random.default_rng(21)
    A = rng.normal(size=(d, d))
    x = rng.normal(size=(n, Wp, d)) @ A.T
    P = np.linalg.inv(A @ A.T)
    logp = lambda t: -0.5 * np.einsum('...i,ij,...j->...', t, P, t)
    res = ev.bridge_evidence(x, logp(x), logp, seed=4, neff=None, order=None)
    assert list(res) == ['log_evidence', 'log_ml', 'se', 'iterations', 'n1', 'n2', 'neff', 'tau_f2', 'frac_outside',
                         'gaussian_offset', 'proposal_mean', 'proposal_cov']
    plain = ev.bridge_evidence(x, logp(x), logp, seed=4, neff=None)
    assert list(plain) == list(res) and all(np.array_equal(plain[k], res[k], equal_nan=True) for k in res)
    n0, n1 = ev.halves(n, Wp, d)
    mu, L, c = ev.proposal_factor(*flat_cov(x[:n0]))
    l1 = (logp(x[n0:]) - ev.log_g(x[n0:], mu[0], L[0], float(c[0]))).reshape(-1)
    theta2, lg2 = ev.host_draws(mu[0], L[0], float(c[0]), n1 * Wp, 4, 0, 0)
    lstar, a1, a2 = ev.bridge_terms(l1, logp(theta2) - lg2)
    it = ev.bridge_iterate(a1, a2, 0.5)
    assert res['log_ml'] == it['log_r'] + float(lstar) == res['log_evidence'] and res['iterations'] == it['iterations']


# -- sanitizers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_row_function_under_asan_ubsan(tmp_path):
    """The row function is plain C++ in a header: a stand-alone program of its own runs it, every mode count, key group and
    combination of outputs on buffers of the exact size, under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / 'sanitize_mode_order'
    build = subprocess.run(['g++', '-std=gnu++17', '-O1', '-g', '-fno-omit-frame-pointer', '-ffp-contract=off',
                            '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe),
                            os.path.join(ROOT, 'tests', 'native', 'sanitize_mode_order.cpp')],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'sanitize_mode_order: ok' in run.stdout
