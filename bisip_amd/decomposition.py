"""Relaxation time distribution (RTD) and integrating parameters of PolynomialDecomposition.

The reference's decomposition tutorial (docs/tutorials/decomposition.ipynb, the ``get_m`` cell and the RTD plots
after it) computes them by hand from the posterior mean.  Here they are taken per posterior sample, so their
mean, std and percentiles are a real posterior (the mean relaxation time is nonlinear in the parameters: the
mean of the parameters does not give its mean).

Definitions, for a row ``theta = (r0, a_0, ..., a_P)`` (ascending powers) on the model's grid ``log_tau`` (L):

* ``m_l = sum_p a_p * log_tau_l**p`` -- the RTD, ``(L,)`` per row;
* ``m_total = sum_l m_l`` -- the tutorial's ``np.sum(m)``;
* ``log_tau_mean = sum_l m_l * log_tau_l / m_total`` -- log10 of the chargeability-weighted mean relaxation time
  (Keery et al., 2012), plain IEEE division;
* ``m_norm = m_total / (r0 * norm_factor)`` -- the normalised chargeability, rho_0 in the data's units.

``rtd`` and ``integrating_params`` evaluate them on the host in NumPy.  The ``device_*`` functions run
``bisip_rtd_integrals_dev`` / ``bisip_rtd_columns_dev`` on a ChainView (bisip_amd.chainview) on the GPU; the
derived chain is summarised there as any chain is (device_moments, device_percentiles).
"""

import numpy as np

__all__ = ('INTEGRATING_NAMES', 'rtd', 'integrating_params', 'power_sums', 'device_integrating_chain',
           'device_rtd_percentiles')

INTEGRATING_NAMES = ('m_total', 'log_tau_mean', 'm_norm')

# device bytes of columns per pass of get_rtd_percentile and of SpectraBatch.get_model_percentile: ensembles go in
# passes that stay under it
RTD_PASS_BYTES = 8 << 30


def _theta(theta):
    theta = np.asarray(theta, dtype=np.float64)
    if theta.ndim < 1 or theta.shape[-1] < 2:
        raise ValueError(f'theta must end in (r0, a_0, ..., a_P), got shape {theta.shape}')
    return theta


def rtd(theta, log_tau):
    """``m_l = sum_p a_p * log_tau_l**p`` for every row of ``theta`` (..., P + 2): (..., L)."""
    theta = _theta(theta)
    log_tau = np.asarray(log_tau, dtype=np.float64)
    m = 0
    for p in range(theta.shape[-1] - 1):
        m = m + theta[..., 1 + p, None] * log_tau ** p
    return m


def integrating_params(theta, log_tau, norm_factor):
    """``(m_total, log_tau_mean, m_norm)`` of every row of ``theta`` (..., P + 2): (..., 3).  ``norm_factor``
    broadcasts against the rows (one per spectrum: shape ``(E, 1)`` for theta ``(E, n, P + 2)``)."""
    theta = _theta(theta)
    log_tau = np.asarray(log_tau, dtype=np.float64)
    m = rtd(theta, log_tau)
    total = np.sum(m, axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.sum(m * log_tau, axis=-1) / total
        norm = total / (theta[..., 0] * np.asarray(norm_factor, dtype=np.float64))
    return np.stack([total, mean, norm], axis=-1)


def power_sums(log_tau, ndim):
    """``S_k = sum_l log_tau_l**k`` for k = 0 ... ndim - 1, accumulated in long double and rounded once."""
    lt = np.asarray(log_tau, dtype=np.float64).astype(np.longdouble)
    x = np.ones_like(lt)
    out = np.empty(int(ndim))
    for k in range(int(ndim)):
        out[k] = np.float64(np.sum(x))
        x = x * lt
    return out


def device_integrating_chain(view, log_tau, norm_factor):
    """``(m_total, log_tau_mean, m_norm)`` of the samples of a ChainView (bisip_amd.chainview): a new device
    tensor ``(n, n_ensembles * walkers_per_ensemble, 3)``, summarised through ``view.derived`` of it.
    ``norm_factor``: scalar or one per ensemble.  Asynchronous."""
    import torch
    from . import _hip
    E, Wp, ndim = view.n_ensembles, view.walkers_per_ensemble, view.ndim
    nf = np.broadcast_to(np.asarray(norm_factor, dtype=np.float64), (E,))
    S = view.upload(power_sums(log_tau, ndim))
    d_nf = view.upload(nf)
    out = view.empty((view.n, E * Wp, 3), torch.float64)
    _hip.rtd_integrals_dev(view.ptr, view.n, view.stride, E, Wp, ndim, S.data_ptr(), d_nf.data_ptr(), out.data_ptr(),
                           view.stream)
    return out


def device_rtd_percentiles(view, p, log_tau):
    """np.percentile of the RTD over every ensemble's samples of a ChainView: ``(len(p), n_ensembles, L)`` (NumPy).
    The m_l go column by column (bisip_rtd_columns_dev), ensembles in passes whose columns stay under
    ``RTD_PASS_BYTES``."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    lt = np.ascontiguousarray(log_tau, dtype=np.float64)
    L = lt.size
    d_lt = view.upload(lt)
    rows = n * Wp
    G = int(min(E, max(1, RTD_PASS_BYTES // (rows * L * 8))))
    out = np.empty((p.size, E, L))
    for g0 in range(0, E, G):
        k = min(E, g0 + G) - g0
        cols = view.empty((k * L, rows), torch.float64)
        _hip.rtd_columns_dev(view.ptr, n, view.stride, E, Wp, ndim, g0, k, d_lt.data_ptr(), L, cols.data_ptr(),
                             view.stream)
        res = view.empty((p.size, k * L), torch.float64)
        _hip.columns_percentiles_dev(cols.data_ptr(), k * L, rows, p, res.data_ptr(), view.stream)
        view.synchronize()
        out[:, g0:g0 + k] = res.cpu().numpy().reshape(p.size, k, L)
        del cols, res
    return out
