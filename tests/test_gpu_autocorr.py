"""Integrated autocorrelation time on the device (bisip_chain_autocorr_time_dev) against emcee's algorithm
on the host (bisip_amd.autocorr), from the C entry point up to the samplers and SpectraBatch."""

import warnings

import numpy as np
import pytest

from bisip_amd.autocorr import AutocorrError, _acf, auto_window, integrated_time
from chain_harness import GuardedCall, used_window

pytestmark = pytest.mark.gpu

TAU_RTOL = 1e-10
MARGIN = 1e-9


def ar1(rng, n_t, n_walkers, rho):
    """AR(1) chains (n_t, n_walkers, len(rho)) with per-parameter rho, offsets and scales (std >= 1e-6 |mean|)."""
    rho = np.asarray(rho, dtype=np.float64)
    n_d = rho.size
    x = np.empty((n_t, n_walkers, n_d))
    x[0] = rng.standard_normal((n_walkers, n_d)) / np.sqrt(1.0 - rho ** 2)
    e = rng.standard_normal((n_t, n_walkers, n_d))
    for t in range(1, n_t):
        x[t] = rho * x[t - 1] + e[t]
    return x * rng.uniform(0.1, 10.0, n_d) + rng.uniform(-50.0, 50.0, n_d)


def host_reference(x, E, c=5.0):
    """emcee's tau, window and the margin min_{m <= window} |m - c taus_m| per (ensemble, parameter) of a chain
    (n_t, E * Wp, ndim)."""
    n_t, W, ndim = x.shape
    Wp = W // E
    tau, win, margin = np.empty((E, ndim)), np.empty((E, ndim), dtype=np.int64), np.empty((E, ndim))
    for e in range(E):
        for d in range(ndim):
            f = _acf(x[:, e * Wp:(e + 1) * Wp, d]).sum(axis=1) / Wp
            taus = 2.0 * np.cumsum(f) - 1.0
            w = auto_window(taus, c)
            win[e, d], tau[e, d] = w, taus[w]
            with np.errstate(invalid='ignore'):
                margin[e, d] = np.min(np.abs(np.arange(w + 1) - c * taus[:w + 1]))
    return tau, win, margin


def assert_tau_close(got, want, margin=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    if margin is not None:
        fin = np.isfinite(margin)
        assert np.all(margin[fin] > MARGIN), 'a case sits on a rounding tie of the window test'
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    assert err.size == 0 or err.max() <= TAU_RTOL, err.max()


def entry_point(t, n, first, stride, E, Wp, ndim, c=5.0):
    """tau and windows from the C entry point on a device tensor, by pointer offset and stride (doubles).  Outputs and
    workspace are followed by guard values."""
    import torch
    from bisip_amd import _hip
    call = GuardedCall()
    tau, win = call.out('tau', (E, ndim)), call.out('the windows', (E, ndim), torch.int64)
    work = call.work(_hip.chain_autocorr_time_workspace(n, E, Wp, ndim))
    _hip.chain_autocorr_time_dev(t.data_ptr() + 8 * first, n, stride, E, Wp, ndim, c, tau, win, work, call.stream)
    return tuple(call.finish())


# a covering set of E in {1, 3, 64}, Wp in {2, 31, 256}, ndim in {1, 7, 12}, n_t in {1, 2, 3, 64, 1000, 5000}
@pytest.mark.parametrize('E,Wp,ndim,n_t,discard,thin', [
    (1, 2, 1, 1, 0, 1),
    (3, 31, 7, 2, 1, 2),
    (64, 2, 12, 3, 0, 1),
    (1, 256, 12, 64, 5, 3),
    (3, 256, 1, 1000, 0, 1),
    (64, 31, 7, 64, 2, 1),
    (1, 31, 7, 5000, 0, 1),
    (3, 2, 12, 1000, 10, 2),
    (64, 256, 1, 1000, 0, 1),
    (1, 2, 7, 5000, 3, 1),
])
def test_entry_point_against_emcee(E, Wp, ndim, n_t, discard, thin):
    import torch
    rng = np.random.default_rng(E * 1000 + Wp * 10 + ndim)
    rho = np.linspace(0.0, 0.95, ndim)
    full = ar1(rng, discard + n_t * thin, E * Wp, rho)
    t = torch.from_numpy(full).cuda()
    offset, stride, n = used_window(full.shape[0], E * Wp * ndim, discard, thin)
    used = full[discard + thin - 1::thin]
    assert used.shape[0] == n == n_t
    tau, win = entry_point(t, n_t, offset, stride, E, Wp, ndim)
    want, want_win, margin = host_reference(used, E)
    assert_tau_close(tau, want, margin)
    assert np.array_equal(win, want_win)


def test_ensembles_of_very_different_times_stop_each_at_its_window():
    """White noise next to rho = 0.99 at n_t = 1000 in a batch wide enough for rounds of 64 lags: every
    (ensemble, parameter) stops at its own window, from the first round to the last."""
    import torch
    E, Wp, ndim, n_t = 64, 256, 2, 1000
    rng = np.random.default_rng(7)
    parts = [ar1(rng, n_t, Wp, [0.0, 0.5] if e % 2 == 0 else [0.99, 0.0]) for e in range(E)]
    full = np.concatenate(parts, axis=1)
    t = torch.from_numpy(full).cuda()
    tau, win = entry_point(t, n_t, 0, E * Wp * ndim, E, Wp, ndim)
    want, want_win, margin = host_reference(full, E)
    assert_tau_close(tau, want, margin)
    assert np.array_equal(win, want_win)
    assert want_win[0::2, 0].max() < 64 and want_win[1::2, 0].min() > 5 * 64    # first round vs. late rounds
    from bisip_amd import _hip
    assert _hip.chain_autocorr_time_workspace(n_t, E, Wp, ndim) < 8 * E * Wp * ndim * n_t // 4


def test_repeatable_and_refuses_bad_arguments():
    import torch
    from bisip_amd import _hip
    E, Wp, ndim, n_t = 5, 64, 7, 700
    full = ar1(np.random.default_rng(3), n_t, E * Wp, np.linspace(0, 0.9, ndim))
    t = torch.from_numpy(full).cuda()
    a = entry_point(t, n_t, 0, E * Wp * ndim, E, Wp, ndim)
    b = entry_point(t, n_t, 0, E * Wp * ndim, E, Wp, ndim)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])
    n = E * Wp * ndim
    nbytes = _hip.chain_autocorr_time_workspace(n_t, E, Wp, ndim)
    work = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    tau = torch.empty((E, ndim), dtype=torch.float64, device='cuda')
    ok = (t.data_ptr(), n_t, n, E, Wp, ndim, 5.0, tau.data_ptr(), 0, work.data_ptr(), 0)
    bad = [dict(c=0.0), dict(c=-1.0), dict(c=float('nan')), dict(c=float('inf')), dict(ndim=0), dict(ndim=17),
           dict(n=0), dict(E=0), dict(Wp=0), dict(stride=n - 1), dict(chain=0), dict(tau=0), dict(work=0)]
    names = ('chain', 'n', 'stride', 'E', 'Wp', 'ndim', 'c', 'tau', 'win', 'work', 'stream')
    for change in bad:
        args = dict(zip(names, ok))
        args.update(change)
        with pytest.raises(ValueError):
            _hip.chain_autocorr_time_dev(*(args[k] for k in names))
    assert _hip.chain_autocorr_time_workspace(0, E, Wp, ndim) == 0
    assert _hip.chain_autocorr_time_workspace(n_t, E, Wp, 17) == 0
    with pytest.raises(ValueError):
        integrated_time(t.reshape(n_t, E * Wp, ndim), c=0)


def test_integrated_time_of_a_device_tensor():
    import torch
    x = ar1(np.random.default_rng(4), 3000, 32, [0.0, 0.6, 0.9])
    want = integrated_time(x)
    got = integrated_time(torch.from_numpy(x).cuda())
    _, _, margin = host_reference(x, 1)
    assert_tau_close(got, want, margin[0])
    with pytest.raises(AutocorrError) as err:
        integrated_time(torch.from_numpy(x[:300]).cuda())
    with pytest.warns(UserWarning):
        quiet = integrated_time(torch.from_numpy(x[:300]).cuda(), quiet=True)
    assert np.array_equal(err.value.tau, quiet)


@pytest.mark.parametrize('cls_name,kw', [('PolynomialDecomposition', {}), ('PeltonColeCole', dict(n_modes=2))])
@pytest.mark.parametrize('chain', ['device', 'host'])
def test_fitted_sampler_get_autocorr_time(cls_name, kw, chain):
    import bisip_amd
    np.random.seed(21)
    model = getattr(bisip_amd, cls_name)(bisip_amd.DataFiles()['SIP-K389175'], nwalkers=32, nsteps=1500, **kw)
    model.fit(chain=chain)
    for discard, thin in ((0, 1), (500, 1), (300, 4)):
        got = model.sampler.get_autocorr_time(discard=discard, thin=thin, tol=0)
        x = model.get_chain(discard=discard, thin=thin)
        want = thin * integrated_time(x, tol=0)
        _, _, margin = host_reference(x, 1)
        assert_tau_close(got, want, margin[0])
        np.testing.assert_array_equal(model.get_autocorr_time(discard=discard, thin=thin, tol=0), got)
    with pytest.raises(AutocorrError) as err:
        model.sampler.get_autocorr_time(discard=500, tol=1000)
    assert err.value.tau.shape == (model.ndim,)


@pytest.mark.parametrize('chain', ['device', 'host'])
def test_spectra_batch_get_autocorr_time(chain):
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    E, Wp = 6, 32
    rng = np.random.RandomState(11)
    centre = np.array([1.0, 0.15, 0.5, -1.5, -12.0, 0.45, 0.6])
    p0 = centre + 1e-3 * rng.randn(E, Wp, 7)
    b = bisip_amd.SpectraBatch('PeltonColeCole', [synthetic_columns(32, i) for i in range(E)], nwalkers=Wp,
                               nsteps=600, n_modes=2)
    b.fit(p0, seed=5, chain=chain)
    for discard, thin in ((100, 1), (200, 3)):
        got = b.get_autocorr_time(discard=discard, thin=thin, tol=0)
        assert got.shape == (E, 7)
        ch = b.get_chain(discard=discard, thin=thin)             # (n, E, Wp, ndim)
        for e in range(E):
            x = ch[:, e]
            _, _, margin = host_reference(x, 1)
            assert_tau_close(got[e], thin * integrated_time(x, tol=0), margin[0])
    with pytest.raises(AutocorrError) as err:
        b.get_autocorr_time(discard=500)                         # 100 samples: too short for tol = 50
    assert err.value.tau.shape == (E, 7)
    with pytest.warns(UserWarning, match='ensembles'):
        quiet = b.get_autocorr_time(discard=500, quiet=True)
    assert np.array_equal(quiet, err.value.tau)
    np.testing.assert_array_equal(b.gather(quiet), quiet)


def test_cfg5_slice_full_size():
    """512 spectra x 256 walkers x 7 parameters, 1000 stored samples, discard 500: every tau finite, eight
    random spectra against the host function."""
    import torch
    from bisip_amd.autocorr import device_integrated_time
    from bisip_amd.chainview import ChainView
    E, Wp, ndim, n_total, discard = 512, 256, 7, 1000, 500
    g = torch.Generator(device='cuda').manual_seed(0)
    rho = torch.linspace(0.0, 0.97, E * ndim, dtype=torch.float64, device='cuda').reshape(E, 1, ndim)
    rho = rho.expand(E, Wp, ndim).reshape(E * Wp, ndim)
    chain = torch.empty((n_total, E * Wp, ndim), dtype=torch.float64, device='cuda')
    chain[0] = torch.randn((E * Wp, ndim), generator=g, dtype=torch.float64, device='cuda') / torch.sqrt(1 - rho * rho)
    for s in range(1, n_total):
        chain[s] = rho * chain[s - 1] + torch.randn((E * Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
    W = E * Wp
    tau, win = device_integrated_time(ChainView(chain, n_total - discard, E, Wp, ndim, offset=discard * W * ndim,
                                                stride=W * ndim), 5.0)
    assert np.isfinite(tau).all() and (win >= 1).all()
    for e in np.random.default_rng(0).choice(E, 8, replace=False):
        x = chain[discard:, e * Wp:(e + 1) * Wp].cpu().numpy()
        want, want_win, margin = host_reference(x, 1)
        assert_tau_close(tau[e], want[0], margin[0])
        assert np.array_equal(win[e], want_win[0])
    del chain


def test_constant_walker_makes_its_ensemble_nan():
    import torch
    E, Wp, ndim, n_t = 3, 31, 4, 400
    full = ar1(np.random.default_rng(9), n_t, E * Wp, [0.1, 0.3, 0.5, 0.7])
    full[:, 1 * Wp + 5, 2] = 1.0          # exact mean: the centred series is 0, its acf 0/0
    t = torch.from_numpy(full).cuda()
    tau, win = entry_point(t, n_t, 0, E * Wp * ndim, E, Wp, ndim)
    assert np.isnan(tau[1, 2]) and win[1, 2] == n_t - 1
    nan = np.zeros((E, ndim), dtype=bool)
    nan[1, 2] = True
    assert np.array_equal(np.isnan(tau), nan)
    want, want_win, _ = host_reference(full, E)
    assert_tau_close(tau, want)
    assert np.array_equal(win, want_win)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.isnan(integrated_time(full[:, Wp:2 * Wp], tol=0)[2])
