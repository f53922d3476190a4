"""Integrated autocorrelation time of MCMC chains, with emcee's names and semantics
(emcee 3.1, ``emcee/autocorr.py``).

``integrated_time`` given a NumPy array runs emcee's algorithm on the host, the walkers of a parameter at
once; given a float64 torch tensor on the GPU it runs ``bisip_chain_autocorr_time_dev`` where the chain
lies.  The one difference from emcee: ``c`` must be finite and positive (emcee accepts any ``c`` and then
returns a window that means nothing).
"""

import warnings

import numpy as np

__all__ = ('AutocorrError', 'function_1d', 'auto_window', 'integrated_time')


class AutocorrError(Exception):
    """Raised when the chain is too short to estimate the autocorrelation time reliably; ``tau`` holds
    every estimate."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super().__init__(*args, **kwargs)


def next_pow_two(n):
    i = 1
    while i < n:
        i = i << 1
    return i


def function_1d(x):
    """Normalised autocorrelation function of a 1-D series (zero-padded FFT, as emcee)."""
    x = np.atleast_1d(x)
    if len(x.shape) != 1:
        raise ValueError('invalid dimensions for 1D autocorrelation function')
    return _acf(x[:, np.newaxis])[:, 0]


def _acf(x):
    """function_1d of every column of x (n_t, k)."""
    n_t = x.shape[0]
    n = next_pow_two(n_t)
    f = np.fft.fft(x - np.mean(x, axis=0), n=2 * n, axis=0)
    acf = np.fft.ifft(f * np.conjugate(f), axis=0)[:n_t].real
    with np.errstate(invalid='ignore', divide='ignore'):     # a constant series: 0/0 = NaN, as emcee
        acf /= acf[0]
    return acf


def auto_window(taus, c):
    """emcee's automated windowing procedure (Sokal 1989)."""
    m = np.arange(len(taus)) < c * taus
    if np.any(m):
        return np.argmin(m)
    return len(taus) - 1


def check_c(c):
    c = float(c)
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f'c={c!r}: the window factor must be finite and > 0')
    return c


def check_tol(tau, n_t, tol, quiet, what='parameter(s)'):
    """integrated_time's convergence test: ``tol * tau > n_t`` anywhere raises AutocorrError carrying all of
    ``tau`` (``quiet``: warns instead).  Returns ``tau``."""
    flag = tol * tau > n_t
    if np.any(flag):
        msg = (f'The chain is shorter than {tol} times the integrated autocorrelation time for '
               f'{int(np.sum(flag))} {what}. Use this estimate with caution and run a longer chain!\n'
               f'N/{tol} = {n_t / tol:.0f};\ntau: {tau}')
        if not quiet:
            raise AutocorrError(tau, msg)
        warnings.warn(msg, UserWarning, stacklevel=3)
    return tau


def _as_3d(x, has_walkers):
    if x.ndim == 1:
        x = x[:, None, None]
    if x.ndim == 2:
        x = x[:, None, :] if not has_walkers else x[:, :, None]
    if x.ndim != 3:
        raise ValueError('invalid dimensions')
    return x


def _is_device_tensor(x):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda


def integrated_time(x, c=5, tol=50, quiet=False, has_walkers=True):
    """Integrated autocorrelation time of every parameter of a chain ``x`` (n_t, n_walkers, n_dim) (1-D and
    2-D as emcee reads them).  Raises AutocorrError when ``tol * tau > n_t`` for any parameter (``quiet``:
    warns and returns).  A float64 torch tensor on the GPU is estimated there."""
    c = check_c(c)
    if _is_device_tensor(x):
        from .chainview import ChainView
        view = ChainView.of_tensor(_as_3d(x, has_walkers))
        tau, _ = device_integrated_time(view, c)
        return check_tol(tau[0], view.n, tol, quiet)
    x = _as_3d(np.atleast_1d(np.asarray(x)), has_walkers)
    n_t, n_w, n_d = x.shape
    tau_est = np.empty(n_d)
    for d in range(n_d):
        f = _acf(x[:, :, d]).sum(axis=1) / n_w
        taus = 2.0 * np.cumsum(f) - 1.0
        tau_est[d] = taus[auto_window(taus, c)]
    return check_tol(tau_est, n_t, tol, quiet)


def device_integrated_time(view, c):
    """tau and windows ``(n_ensembles, ndim)`` (NumPy) of the samples of a ChainView (bisip_amd.chainview).  No tol
    check."""
    import torch
    from . import _hip
    c = check_c(c)
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    nbytes = _hip.chain_autocorr_time_workspace(n, E, Wp, ndim)
    if nbytes <= 0:
        raise ValueError(f'chain shape ({n}, {E} x {Wp}, {ndim}) not supported')
    work = view.empty((nbytes,), torch.uint8)
    tau = view.empty((E, ndim), torch.float64)
    win = view.empty((E, ndim), torch.int64)
    _hip.chain_autocorr_time_dev(view.ptr, n, view.stride, E, Wp, ndim, c, tau.data_ptr(), win.data_ptr(),
                                 work.data_ptr(), view.stream)
    view.synchronize()
    return tau.cpu().numpy(), win.cpu().numpy()
