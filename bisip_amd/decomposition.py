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

Relaxation descriptors
----------------------
The relaxation time of the RTD's peak and the cumulative relaxation times (tau_10, tau_50, tau_90 of Nordsiek &
Weller, 2008, and Weigand & Kemna, 2016: the times at which 10, 50 and 90 % of the total chargeability have
accumulated) are nonlinear in ``a_p`` as well, and are taken per posterior sample in the same way.  The kernel
(csrc/chain_rtd_descriptors.hip), the row function it shares with the host entry point (csrc/rtd_descriptors.h),
``rtd_descriptors`` below and the tests all follow this statement.  For a row ``theta = (r0, a_0, ..., a_P)``, the
grid ``x_l = log_tau_l`` (``l = 0 ... L-1``, strictly ascending) and fractions ``q_1 ... q_J`` (``1 <= J <= 8``, every
``0 < q_j <= 1``; by default 0.1, 0.5, 0.9):

1. ``m_l`` by Horner with explicit fma, highest power first, as k_rtd_columns does: ``m = a_P``, then
   ``m = fma(m, x_l, a_p)`` for ``p = P-1 ... 0`` -- the bits of bisip_rtd_columns_dev.  (``rtd_descriptors``, in
   NumPy, has no fma: it rounds the product and the sum, and differs from the library in the last bits.)
2. ``c_l = m_l if m_l > 0 else 0``: chargeability is not negative; a polynomial's negative lobes and a NaN count as 0.
3. Pass 1, ``l`` ascending: ``g_l = g_{l-1} + c_l`` (a plain addition, ``g_{-1} = 0``); ``total = g_{L-1}``.  The
   peak is the first ``l`` with the largest ``m_l``, on the unclipped values: start at ``l = 0``, replace only on a
   strict ``>``.
4. If ``total`` is not finite or not ``> 0``, every output of the row is NaN.
5. Pass 2 recomputes ``g`` by the same additions (the same bits).  For each ``j``: ``t_j = q_j * total`` (one
   multiplication); ``k_j`` is the first ``l`` with ``g_l >= t_j`` (it exists: ``g_{L-1} = total >= t_j``); if
   ``k_j = 0`` the value is ``x_0``; otherwise ``f = (t_j - g_{k-1}) / c_k`` by IEEE division (``c_k > 0`` follows
   from ``g_{k-1} < t_j <= g_k``) and the value is ``fma(f, x_k - x_{k-1}, x_{k-1})``.  (``g_k`` is a rounded sum, so
   ``f`` may exceed 1 by ``u * total / c_k``: a value may pass ``x_k`` by that fraction of the step, and is not clamped.)
6. The row gives ``K = 2 + J`` values ``(log_tau_peak, m_peak, log_tau_q1, ..., log_tau_qJ)``, named by
   ``DESCRIPTOR_NAMES(q)``: ``('log_tau_peak', 'm_peak', 'log_tau_10', 'log_tau_50', 'log_tau_90')`` by default.

``total`` here is the sequential sum of the clipped ``c_l``; it is not ``m_total`` above, which comes from the power
sums of the unclipped polynomial: the two differ by the clipping and by rounding.  A posterior whose used samples
include a row with no positive RTD has NaN in that row, and its mean, std, percentiles and HDI are NaN -- as NumPy's
are on the derived chain.
"""

import numpy as np

__all__ = ('INTEGRATING_NAMES', 'rtd', 'integrating_params', 'power_sums', 'device_integrating_chain',
           'device_rtd_percentiles', 'DEFAULT_FRACTIONS', 'DESCRIPTOR_NAMES', 'rtd_descriptors',
           'device_rtd_descriptors', 'host_rtd_descriptors')

INTEGRATING_NAMES = ('m_total', 'log_tau_mean', 'm_norm')
DEFAULT_FRACTIONS = (0.1, 0.5, 0.9)
MAX_FRACTIONS = 8                  # csrc/rtd_descriptors.h: RTD_MAX_FRACTIONS

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


# -- relaxation descriptors ("Relaxation descriptors" of the module docstring) -----------------------------------------
def checked_fractions(q):
    """``q`` as a float64 array ``(J,)``, ``1 <= J <= 8``, every ``0 < q_j <= 1`` (a NaN is refused)."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= MAX_FRACTIONS:
        raise ValueError(f'q must hold 1 to {MAX_FRACTIONS} fractions, got shape {q.shape}')
    if not np.all((q > 0) & (q <= 1)):
        raise ValueError(f'every fraction q must lie in (0, 1], got {q.tolist()}')
    return q


def checked_grid(log_tau):
    """``log_tau`` as a contiguous float64 array ``(L,)``, ``L >= 1``, strictly ascending."""
    lt = np.ascontiguousarray(log_tau, dtype=np.float64)
    if lt.ndim != 1 or lt.size < 1 or not np.all(lt[1:] > lt[:-1]):
        raise ValueError('log_tau must be one-dimensional and strictly ascending')
    return lt


def DESCRIPTOR_NAMES(q=DEFAULT_FRACTIONS):
    """The names of the outputs of ``rtd_descriptors``: ``('log_tau_peak', 'm_peak', 'log_tau_10', ...)``, the
    fractions in per cent."""
    return ('log_tau_peak', 'm_peak') + tuple(f'log_tau_{100 * v:.10g}' for v in checked_fractions(q))


def rtd_descriptors(theta, log_tau, q=DEFAULT_FRACTIONS):
    """``(log_tau_peak, m_peak, log_tau_q1, ..., log_tau_qJ)`` of every row of ``theta`` (..., P + 2): (..., 2 + J),
    the module docstring's definition in NumPy (Horner without fma).  A row with no positive RTD gives NaN."""
    theta, x, q = _theta(theta), checked_grid(log_tau), checked_fractions(q)
    lead = theta.shape[:-1]
    a = theta.reshape(-1, theta.shape[-1])[:, 1:]
    with np.errstate(all='ignore'):
        m = np.repeat(a[:, -1:], x.size, axis=1)
        for p in range(a.shape[1] - 2, -1, -1):
            m = m * x + a[:, p, None]
        c = np.where(m > 0, m, 0.0)
        g = np.cumsum(c, axis=1)                                     # sequential: g_l = g_{l-1} + c_l
        total = g[:, -1]
        valid = np.isfinite(total) & (total > 0)
        # the first l of the largest m_l; a NaN never replaces and, at l = 0, is never replaced
        peak = np.argmax(np.where(np.isnan(m), -np.inf, m), axis=1)
        peak = np.where(np.isnan(m[:, 0]), 0, peak)
        rows = np.arange(m.shape[0])
        out = np.empty((m.shape[0], 2 + q.size))
        out[:, 0], out[:, 1] = x[peak], m[rows, peak]
        for j, qj in enumerate(q):
            t = qj * total
            k = np.argmax(g >= t[:, None], axis=1)
            k1 = np.minimum(np.maximum(k, 1), x.size - 1)            # (k = 0 takes x_0; L = 1 has no other k)
            f = (t - g[rows, k1 - 1]) / c[rows, k1]
            out[:, 2 + j] = np.where(k == 0, x[0], x[k1 - 1] + f * (x[k1] - x[k1 - 1]))
    out[~valid] = np.nan
    return out.reshape(lead + (2 + q.size,))


def device_rtd_descriptors(view, log_tau, q=DEFAULT_FRACTIONS):
    """The relaxation descriptors of the samples of a ChainView (bisip_rtd_descriptors_dev): a new device tensor
    ``(n, n_ensembles * walkers_per_ensemble, 2 + len(q))``, summarised through ``view.derived`` of it.  A row with no
    positive RTD is NaN there, and so is every summary of an ensemble that has one.  Asynchronous."""
    import torch
    from . import _hip
    lt, q = checked_grid(log_tau), checked_fractions(q)
    E, Wp = view.n_ensembles, view.walkers_per_ensemble
    d_lt, d_q = view.upload(lt), view.upload(q)
    out = view.empty((view.n, E * Wp, 2 + q.size), torch.float64)
    _hip.rtd_descriptors_dev(view.ptr, view.n, view.stride, E, Wp, view.ndim, d_lt.data_ptr(), lt.size, d_q.data_ptr(),
                             q.size, out.data_ptr(), view.stream)
    return out


def host_rtd_descriptors(chain, log_tau, q=DEFAULT_FRACTIONS, n_ensembles=1):
    """The rows of ``device_rtd_descriptors`` by the same row function on the CPU (bisip_rtd_descriptors_host), no
    GPU: ``chain`` (n, rows, ndim) gives ``(n, rows, 2 + len(q))``, bit for bit what the kernel stores."""
    from . import _hip
    lt, q = checked_grid(log_tau), checked_fractions(q)
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    if chain.ndim != 3:
        raise ValueError(f'the chain must be (n, rows, ndim), got {chain.shape}')
    n, rows, ndim = chain.shape
    E = int(n_ensembles)
    if E < 1 or rows % E:
        raise ValueError(f'{rows} rows do not divide into {E} ensembles')
    return _hip.rtd_descriptors_host(chain, n, rows * ndim, E, rows // E, ndim, lt, q)


class DecompositionRelaxation:
    """Mixin of PolynomialDecomposition (``_decomposition_samples`` is its ChainView of the samples to summarise): the
    relaxation descriptors of the posterior, per sample.  ``chain`` / ``discard`` / ``thin`` / ``flat`` as the
    get_integrating_* methods; ``q``: the fractions.  A used sample with no positive RTD makes every summary NaN."""

    def relaxation_descriptors(self, theta, q=DEFAULT_FRACTIONS):
        """``(log_tau_peak, m_peak, log_tau_q...)`` of theta (host, DESCRIPTOR_NAMES(q)): ``(K,)`` or ``(n, K)``."""
        return rtd_descriptors(theta, self.log_tau, q)

    def _relaxation_view(self, q, chain, kwargs):
        q = checked_fractions(q)
        view = self._decomposition_samples(chain, kwargs)
        return view.derived(device_rtd_descriptors(view, self.log_tau, q))

    def get_relaxation_chain(self, chain=None, q=DEFAULT_FRACTIONS, **kwargs):
        """The relaxation descriptors of every sample, computed on the GPU: ``(n', nwalkers, K)`` as get_chain;
        ``(n, K)`` with ``flat=True`` or for a ``chain`` array."""
        flat = bool(kwargs.get('flat', False)) or chain is not None
        out = self._relaxation_view(q, chain, kwargs).tensor.cpu().numpy()
        return out.reshape(-1, out.shape[-1]) if flat else out

    def get_relaxation_mean(self, chain=None, q=DEFAULT_FRACTIONS, **kwargs):
        """Posterior mean of the relaxation descriptors: ``(K,)`` (kwargs as get_param_mean)."""
        from .chainview import device_moments
        return device_moments(self._relaxation_view(q, chain, kwargs))[0][0]

    def get_relaxation_std(self, chain=None, q=DEFAULT_FRACTIONS, **kwargs):
        """Posterior standard deviation of the relaxation descriptors: ``(K,)``."""
        from .chainview import device_moments
        return device_moments(self._relaxation_view(q, chain, kwargs))[1][0]

    def get_relaxation_percentile(self, p=[2.5, 50, 97.5], chain=None, q=DEFAULT_FRACTIONS, **kwargs):
        """Percentiles of the relaxation descriptors: ``(len(p), K)``, ``(K,)`` for a scalar ``p``."""
        from .chainview import device_percentiles
        from .utils import first_if_scalar
        return first_if_scalar(p, device_percentiles(self._relaxation_view(q, chain, kwargs), p)[:, 0, :])

    def get_relaxation_hdi(self, mass=0.95, chain=None, q=DEFAULT_FRACTIONS, **kwargs):
        """The highest-density interval of the relaxation descriptors: ``(2, K)``; ``(len(mass), 2, K)`` for a
        sequence of masses."""
        from .interval import device_hdi
        return device_hdi(self._relaxation_view(q, chain, kwargs), mass)[..., 0, :]


class BatchRelaxation:
    """Mixin of SpectraBatch (``_decomposition_sampler()`` is its sampler, refused for another model): the relaxation
    descriptors of every spectrum's posterior, on the device for ``chain='device'`` and ``'host'`` alike."""

    def relaxation_descriptors(self, theta, q=DEFAULT_FRACTIONS):
        """``(log_tau_peak, m_peak, log_tau_q...)`` of theta ``(E, n, ndim)`` (host): ``(E, n, K)``."""
        self._decomposition()
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[0] != self.n_spectra:
            raise ValueError(f'theta must have shape ({self.n_spectra}, n, {self.ndim})')
        return rtd_descriptors(theta, self.log_tau, q)

    def _relaxation_view(self, q, discard, thin):
        s = self._decomposition_sampler()
        q = checked_fractions(q)
        view = s.used_samples_dev(discard, thin)
        return view.derived(device_rtd_descriptors(view, self.log_tau, q))

    def get_relaxation_chain(self, discard=0, thin=1, flat=False, q=DEFAULT_FRACTIONS):
        """The relaxation descriptors of every sample of every spectrum, computed on the GPU: ``(n', E, Wp, K)`` as
        get_chain, ``(E, n' * Wp, K)`` with ``flat``."""
        d = self._relaxation_view(q, discard, thin).tensor
        ch = d.cpu().numpy().reshape(-1, self.n_spectra, self.nwalkers, d.shape[-1])
        if flat:
            ch = ch.transpose(1, 0, 2, 3).reshape(self.n_spectra, -1, d.shape[-1])
        return ch

    def get_relaxation_mean(self, discard=0, thin=1, q=DEFAULT_FRACTIONS):
        """Posterior mean of the relaxation descriptors per spectrum, ``(E, K)``."""
        from .chainview import device_moments
        return device_moments(self._relaxation_view(q, discard, thin))[0]

    def get_relaxation_std(self, discard=0, thin=1, q=DEFAULT_FRACTIONS):
        """Posterior standard deviation of the relaxation descriptors per spectrum, ``(E, K)``."""
        from .chainview import device_moments
        return device_moments(self._relaxation_view(q, discard, thin))[1]

    def get_relaxation_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1, q=DEFAULT_FRACTIONS):
        """Percentiles of the relaxation descriptors per spectrum, ``(len(p), E, K)`` (``(E, K)`` for a scalar ``p``)."""
        from .chainview import device_percentiles
        from .utils import first_if_scalar
        return first_if_scalar(p, device_percentiles(self._relaxation_view(q, discard, thin), p))

    def get_relaxation_hdi(self, mass=0.95, discard=0, thin=1, q=DEFAULT_FRACTIONS):
        """The highest-density interval of the relaxation descriptors per spectrum, ``(2, E, K)`` (``(len(mass), 2, E,
        K)`` for a sequence of masses)."""
        from .interval import device_hdi
        return device_hdi(self._relaxation_view(q, discard, thin), mass)
