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
``bisip_rtd_integrals_dev`` / ``bisip_rtd_columns_dev`` on a float64 chain tensor on the GPU and summarise the
result there with the chain kernels (moments, percentiles).
"""

import numpy as np

__all__ = ('INTEGRATING_NAMES', 'rtd', 'integrating_params', 'power_sums', 'device_integrating_chain',
           'device_integrating_moments', 'device_integrating_percentiles', 'device_rtd_percentiles')

INTEGRATING_NAMES = ('m_total', 'log_tau_mean', 'm_norm')

# device bytes of RTD columns per pass of get_rtd_percentile: ensembles go in passes that stay under it
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


def _device(backend, like):
    """(empty, stream, synchronize) of a HipStretchBackend, else of torch's current stream on ``like``'s device."""
    import torch
    if backend is not None:
        return backend.empty, backend.stream(), backend.synchronize
    dev = like.device

    def empty(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)
    st = torch.cuda.current_stream(dev)
    return empty, st.cuda_stream, st.synchronize


def _upload(a, empty):
    import torch
    a = np.array(a, dtype=np.float64, order='C')          # (a writable copy: broadcast views are read-only)
    t = empty(a.shape, torch.float64)
    t.copy_(torch.from_numpy(a))
    return t


def _check_chain(chain, n_samples, sample_stride, row, offset):
    import torch
    if not isinstance(chain, torch.Tensor) or not chain.is_cuda or chain.dtype != torch.float64:
        raise TypeError('the chain must be a float64 tensor on the GPU')
    if n_samples < 1:
        raise ValueError('no samples')
    if sample_stride is None:
        if not chain.is_contiguous():
            raise ValueError('a chain that is not contiguous needs an explicit sample_stride')
        sample_stride = row
    if sample_stride < row or offset < 0 or offset + (n_samples - 1) * sample_stride + row > chain.numel():
        raise ValueError('the samples asked for lie outside the chain tensor')
    return int(sample_stride)


def device_integrating_chain(chain, n_samples, n_ensembles, walkers_per_ensemble, ndim, log_tau, norm_factor,
                             offset=0, sample_stride=None, backend=None):
    """``(m_total, log_tau_mean, m_norm)`` of samples ``offset``, ``offset + sample_stride``, ... (in doubles) of a
    float64 device tensor ``chain`` whose samples hold ``(n_ensembles * walkers_per_ensemble, ndim)`` rows: a new
    device tensor ``(n_samples, n_ensembles * walkers_per_ensemble, 3)``.  ``norm_factor``: scalar or one per
    ensemble.  ``backend``: a HipStretchBackend (its stream and allocator), else torch's.  Asynchronous."""
    import torch
    from . import _hip
    E, Wp, ndim = int(n_ensembles), int(walkers_per_ensemble), int(ndim)
    stride = _check_chain(chain, int(n_samples), sample_stride, E * Wp * ndim, int(offset))
    empty, stream, _ = _device(backend, chain)
    nf = np.broadcast_to(np.asarray(norm_factor, dtype=np.float64), (E,))
    S = _upload(power_sums(log_tau, ndim), empty)
    d_nf = _upload(nf, empty)
    out = empty((int(n_samples), E * Wp, 3), torch.float64)
    _hip.rtd_integrals_dev(chain.data_ptr() + 8 * int(offset), n_samples, stride, E, Wp, ndim, S.data_ptr(),
                           d_nf.data_ptr(), out.data_ptr(), stream)
    return out


def device_integrating_moments(derived, n_ensembles, walkers_per_ensemble, backend=None):
    """Mean and std ``(n_ensembles, 3)`` (NumPy) of a derived chain from device_integrating_chain."""
    import torch
    from . import _hip
    n, E, Wp = int(derived.shape[0]), int(n_ensembles), int(walkers_per_ensemble)
    empty, stream, sync = _device(backend, derived)
    mean, std = empty((E, 3), torch.float64), empty((E, 3), torch.float64)
    work = empty((max(1, _hip.chain_moments_workspace(n, E, 3)),), torch.float64)
    _hip.chain_moments_dev(derived.data_ptr(), n, E * Wp * 3, E, Wp, 3, mean.data_ptr(), std.data_ptr(),
                           work.data_ptr(), stream)
    sync()
    return mean.cpu().numpy(), std.cpu().numpy()


def device_integrating_percentiles(derived, p, n_ensembles, walkers_per_ensemble, backend=None):
    """np.percentile over every ensemble's samples of a derived chain: ``(len(p), n_ensembles, 3)`` (NumPy)."""
    import torch
    from . import _hip
    n, E, Wp = int(derived.shape[0]), int(n_ensembles), int(walkers_per_ensemble)
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    empty, stream, sync = _device(backend, derived)
    nbytes = _hip.chain_percentiles_workspace(n, E, Wp, 3, p.size)
    if nbytes <= 0:
        raise ValueError('chain too large for one device sort (more than 2^31 values); thin it')
    work = empty((nbytes,), torch.uint8)
    out = empty((p.size, E, 3), torch.float64)
    _hip.chain_percentiles_dev(derived.data_ptr(), n, E * Wp * 3, E, Wp, 3, p, out.data_ptr(), work.data_ptr(),
                               nbytes, stream)
    sync()
    return out.cpu().numpy()


def device_rtd_percentiles(chain, p, n_samples, n_ensembles, walkers_per_ensemble, ndim, log_tau, offset=0,
                           sample_stride=None, backend=None):
    """np.percentile of the RTD over every ensemble's used samples (chain conventions of
    device_integrating_chain): ``(len(p), n_ensembles, L)`` (NumPy).  The m_l go column by column
    (bisip_rtd_columns_dev), ensembles in passes whose columns stay under ``RTD_PASS_BYTES``."""
    import torch
    from . import _hip
    n, E, Wp, ndim = int(n_samples), int(n_ensembles), int(walkers_per_ensemble), int(ndim)
    stride = _check_chain(chain, n, sample_stride, E * Wp * ndim, int(offset))
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    empty, stream, sync = _device(backend, chain)
    lt = np.ascontiguousarray(log_tau, dtype=np.float64)
    L = lt.size
    d_lt = _upload(lt, empty)
    rows = n * Wp
    G = int(min(E, max(1, RTD_PASS_BYTES // (rows * L * 8))))
    out = np.empty((p.size, E, L))
    base = chain.data_ptr() + 8 * int(offset)
    for g0 in range(0, E, G):
        k = min(E, g0 + G) - g0
        cols = empty((k * L, rows), torch.float64)
        _hip.rtd_columns_dev(base, n, stride, E, Wp, ndim, g0, k, d_lt.data_ptr(), L, cols.data_ptr(), stream)
        res = empty((p.size, k * L), torch.float64)
        _hip.columns_percentiles_dev(cols.data_ptr(), k * L, rows, p, res.data_ptr(), stream)
        sync()
        out[:, g0:g0 + k] = res.cpu().numpy().reshape(p.size, k, L)
        del cols, res
    return out
