"""Integrated autocorrelation time on the host (bisip_amd.autocorr): emcee's algorithm against a direct
O(n_t * k) evaluation, known answers of AR(1) chains, the convergence test, and the host sampler's
get_autocorr_time."""

import numpy as np
import pytest

from bisip_amd.autocorr import AutocorrError, auto_window, function_1d, integrated_time
from bisip_amd.sampler import EnsembleSampler


def ar1(rng, n_t, n_w, rho, n_d=None):
    """AR(1) series x_t = rho x_{t-1} + e_t started in the stationary law; rho scalar or (n_d,)."""
    rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    n_d = rho.size if n_d is None else n_d
    rho = np.broadcast_to(rho, (n_d,))
    x = np.empty((n_t, n_w, n_d))
    x[0] = rng.standard_normal((n_w, n_d)) / np.sqrt(1.0 - rho ** 2)
    e = rng.standard_normal((n_t, n_w, n_d))
    for t in range(1, n_t):
        x[t] = rho * x[t - 1] + e[t]
    return x


def direct_time(x, c=5.0):
    """emcee's integrated_time written out: every lag as a direct sum, walkers in order, np.cumsum."""
    n_t, n_w, n_d = x.shape
    tau, win = np.empty(n_d), np.empty(n_d, dtype=int)
    for d in range(n_d):
        f = np.zeros(n_t)
        for w in range(n_w):
            y = x[:, w, d] - x[:, w, d].mean()
            acf = np.array([np.dot(y[:n_t - k], y[k:]) for k in range(n_t)])
            with np.errstate(invalid='ignore', divide='ignore'):
                f += acf / acf[0]
        f /= n_w
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(n_t) < c * taus
        win[d] = np.argmin(m) if m.any() else n_t - 1
        tau[d] = taus[win[d]]
    return tau, win


def host_windows(x, c=5.0):
    out = []
    for d in range(x.shape[2]):
        f = np.mean([function_1d(x[:, w, d]) for w in range(x.shape[1])], axis=0)
        out.append(auto_window(2.0 * np.cumsum(f) - 1.0, c))
    return np.array(out)


@pytest.mark.parametrize('n_t,n_w,rho', [(1, 3, 0.5), (2, 4, 0.0), (3, 5, 0.3), (17, 6, 0.5), (100, 4, 0.9),
                                         (257, 3, 0.98), (1000, 2, 0.0), (3000, 2, 0.7)])
def test_integrated_time_equals_direct_sums(n_t, n_w, rho):
    rng = np.random.default_rng(n_t * 7 + n_w)
    x = ar1(rng, n_t, n_w, [rho, rho / 2, 0.0])
    want, want_win = direct_time(x)
    got = integrated_time(x, quiet=True) if n_t > 1 else integrated_time(x, tol=0)
    assert np.array_equal(host_windows(x), want_win)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if n_t == 1:
        assert np.isnan(got).all()          # the centred series is 0: 0/0, as emcee
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    assert (err <= 1e-11).all(), err


@pytest.mark.parametrize('rho', [0.0, 0.5, 0.9])
def test_long_ar1_chains_have_the_known_time(rho):
    x = ar1(np.random.default_rng(1), 20000, 8, rho, n_d=2)
    tau = integrated_time(x)
    exact = (1 + rho) / (1 - rho)
    assert np.all(np.abs(tau - exact) <= 0.1 * exact), (tau, exact)


def test_short_chain_raises_with_every_estimate():
    x = ar1(np.random.default_rng(2), 200, 4, [0.0, 0.95])
    with pytest.raises(AutocorrError) as err:
        integrated_time(x)
    assert err.value.tau.shape == (2,)
    with pytest.warns(UserWarning, match='shorter than 50 times'):
        quiet = integrated_time(x, quiet=True)
    np.testing.assert_array_equal(quiet, err.value.tau)
    np.testing.assert_array_equal(integrated_time(x, tol=1), quiet)


def test_shapes_as_emcee_reads_them():
    x = ar1(np.random.default_rng(3), 500, 1, [0.3])
    t3 = integrated_time(x, tol=0)
    np.testing.assert_array_equal(integrated_time(x[:, 0, 0], tol=0), t3)                   # (n_t,)
    np.testing.assert_array_equal(integrated_time(x[:, :, 0], tol=0), t3)                   # (n_t, n_w)
    np.testing.assert_array_equal(integrated_time(x[:, 0, :], has_walkers=False, tol=0), t3)
    with pytest.raises(ValueError):
        integrated_time(np.zeros((2, 2, 2, 2)))


@pytest.mark.parametrize('c', [0.0, -1.0, np.inf, np.nan])
def test_window_factor_must_be_positive_and_finite(c):
    with pytest.raises(ValueError, match='finite and > 0'):
        integrated_time(np.random.default_rng(0).standard_normal((50, 2, 1)), c=c)


def test_a_constant_walker_gives_nan():
    x = ar1(np.random.default_rng(4), 300, 6, [0.2, 0.4])
    x[:, 3, 1] = 1.0              # the mean is exact: the centred series is 0
    tau = integrated_time(x, tol=0)
    assert np.isfinite(tau[0]) and np.isnan(tau[1])
    assert host_windows(x)[1] == 299


def gaussian_logp(theta):
    return -0.5 * np.sum(theta ** 2 / np.array([1.0, 4.0, 0.25]), axis=1)


@pytest.mark.filterwarnings('ignore:The chain is shorter')
@pytest.mark.parametrize('discard,thin', [(0, 1), (100, 1), (50, 3)])
def test_host_sampler_get_autocorr_time(discard, thin):
    np.random.seed(5)
    s = EnsembleSampler(16, 3, gaussian_logp)
    s.run_mcmc(np.random.randn(16, 3), 600)
    want = thin * integrated_time(s.get_chain(discard=discard, thin=thin), quiet=True)
    got = s.get_autocorr_time(discard=discard, thin=thin, quiet=True)
    np.testing.assert_array_equal(got, want)
    with pytest.raises(AutocorrError):
        s.get_autocorr_time(discard=discard, thin=thin, tol=1000)


def test_autocorr_error_is_exported():
    import bisip_amd
    assert bisip_amd.AutocorrError is AutocorrError and issubclass(AutocorrError, Exception)
