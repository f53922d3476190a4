"""Highest-density intervals of the posterior: the shortest interval that holds a given mass.

The posteriors of Cole-Cole ``m`` and ``c`` pile up against their prior bounds, ``log_tau`` is skewed, the integrating
parameters of the Debye decomposition are ratios: an equal-tailed interval (``get_param_percentile([2.5, 97.5])``) cuts
2.5 % off the side where the density is highest.  The highest-density interval (HDI) is what ArviZ reports by default.

The definition, for one column ``x`` of ``N`` values (one parameter of one ensemble over its flattened used samples) and
``0 < mass < 1``:

* ``s = np.sort(x)``, ``K = int(np.floor(mass * N))``, ``M = N - K``; ValueError unless ``1 <= K <= N - 1``;
* ``width[i] = s[i + K] - s[i]`` for ``i = 0 .. M - 1``, a NaN width (``inf - inf``) read as ``+inf``;
* ``i*`` = the lowest ``i`` of smallest width; the interval is ``(s[i*], s[i* + K])``;
* a column that holds a NaN gives ``(NaN, NaN)`` (and ``i* = 0``), as ``np.percentile`` does.

This is ArviZ's unimodal ``hdi`` with the tie and NaN rules written out.

* ``hdi``, ``windows``: the definition, plain NumPy in float64;
* ``device_hdi`` runs ``bisip_chain_hdi_dev`` on a ChainView (bisip_amd.chainview) where the chain lies: subtractions and
  comparisons of the same doubles, so the same results (the sign of a zero is not pinned);
* ``plan`` is the kernel's choice between its two paths, a function of the shape and the windows alone;
* ``ModelIntervals``, ``DecompositionIntervals`` and ``BatchIntervals`` are the ``get_param_hdi`` method of the models
  (bisip_amd.utils.utils), ``get_integrating_hdi`` of PolynomialDecomposition and the two of SpectraBatch, as mixins.

The rows of an ensemble are numbered ``k * Wp + w`` (sample ``k``, walker ``w``): the order of ``get_chain(flat=True)``.
"""

import os

import numpy as np

from .covariance import _is_device_tensor, _rows, _view_of

__all__ = ('hdi', 'windows', 'plan', 'device_hdi', 'ModelIntervals', 'DecompositionIntervals', 'BatchIntervals')

MAX_WINDOWS = 8                           # chain_hdi.hip: HDI_MAX_WINDOWS
TAILS_SHARE, TAILS_MIN_N = 8, 4096        # chain_hdi.hip: HDI_TAILS_SHARE, HDI_TAILS_MIN_N


def windows(mass, N):
    """``K = int(np.floor(mass * N))`` of every mass, an int64 array ``(len(mass),)`` (``(1,)`` for a scalar): how many
    steps of the sorted column an interval spans.  ValueError unless ``0 < mass < 1`` and ``1 <= K <= N - 1``."""
    m = np.atleast_1d(np.asarray(mass, dtype=np.float64))
    N = int(N)
    if m.ndim != 1 or m.size < 1:
        raise ValueError('mass must be a number or a sequence of numbers')
    if not ((m > 0.0) & (m < 1.0)).all():
        raise ValueError(f'mass must lie strictly between 0 and 1, got {mass}')
    if N < 2:
        raise ValueError(f'an interval needs 2 values, got {N}')
    K = np.floor(m * N).astype(np.int64)
    if (K < 1).any() or (K > N - 1).any():
        raise ValueError(f'mass {mass} of {N} values leaves no interval: floor(mass * N) must lie in [1, {N - 1}]')
    return K


def hdi(x, mass=0.95, n_ensembles=1, index=False):
    """The highest-density interval of every parameter of every ensemble of a chain ``(n, E * Wp, ndim)`` -- or of a flat
    chain ``(N, ndim)``, one ensemble: ``(2, E, ndim)``, lower ends then upper ends, for a scalar ``mass``; ``(len(mass), 2,
    E, ndim)`` for a sequence.  ``index=True``: ``(intervals, i*)`` with ``i*`` int64 of shape ``(E, ndim)`` or ``(len(mass),
    E, ndim)``.  A float64 tensor on the GPU is reduced there (device_hdi)."""
    if _is_device_tensor(x):
        return device_hdi(_view_of(x, n_ensembles), mass, index=index)
    rows = _rows(x, n_ensembles)
    E, N, ndim = rows.shape
    Ks = windows(mass, N)
    s = np.sort(rows, axis=1)
    has_nan = np.isnan(rows).any(axis=1)                       # (E, ndim)
    out = np.empty((Ks.size, 2, E, ndim))
    idx = np.empty((Ks.size, E, ndim), dtype=np.int64)
    e, q = np.meshgrid(np.arange(E), np.arange(ndim), indexing='ij')
    for k, K in enumerate(Ks):
        K = int(K)
        with np.errstate(all='ignore'):
            width = s[:, K:, :] - s[:, :N - K, :]
        width = np.where(np.isnan(width), np.inf, width)
        i = np.where(has_nan, 0, np.argmin(width, axis=1)).astype(np.int64)      # (argmin: the lowest among equals)
        idx[k] = i
        out[k, 0] = np.where(has_nan, np.nan, s[e, i, q])
        out[k, 1] = np.where(has_nan, np.nan, s[e, i + K, q])
    if not np.ndim(mass):
        out, idx = out[0], idx[0]
    return (out, idx) if index else out


def plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, K):
    """``'full'`` or ``'tails'``: the path bisip_chain_hdi_dev takes for the windows ``K`` (include/bisip_hip.h) -- the
    tails when the columns have ``TAILS_MIN_N`` values at least and every window leaves ``M = N - K <= N / TAILS_SHARE``
    (and the tails fit one sort), else the full sort.  The environment variable ``BISIP_HDI_PATH=full|tails`` forces a
    path, here as there."""
    force = os.environ.get('BISIP_HDI_PATH')
    if force in ('full', 'tails'):
        return force
    N, columns = int(n_samples) * int(walkers_per_ensemble), int(n_ensembles) * int(ndim)
    m_max = max(N - int(k) for k in np.atleast_1d(K))
    if N >= TAILS_MIN_N and m_max * TAILS_SHARE <= N and 2 * columns * m_max <= 0x7fffffff:
        return 'tails'
    return 'full'


def device_hdi(view, mass=0.95, index=False):
    """``hdi`` of every ensemble's samples of a ChainView, taken where the chain lies (bisip_chain_hdi_dev): ``(2,
    n_ensembles, ndim)`` or ``(len(mass), 2, n_ensembles, ndim)`` (NumPy); ``index=True`` adds ``i*``."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    Ks = windows(mass, n * Wp)
    out = np.empty((Ks.size, 2, E, ndim))
    idx = np.empty((Ks.size, E, ndim), dtype=np.int64)
    for k0 in range(0, Ks.size, MAX_WINDOWS):
        K = Ks[k0:k0 + MAX_WINDOWS]
        nbytes = _hip.chain_hdi_workspace(n, E, Wp, ndim, K)
        if nbytes < 0:
            raise ValueError('chain too large for one device sort (more than 2^31 values); thin it or use get_chain()')
        work = view.empty((max(1, nbytes),), torch.uint8)
        d_out = view.empty((K.size, 2, E, ndim), torch.float64)
        d_idx = view.empty((K.size, E, ndim), torch.int64) if index else None
        _hip.chain_hdi_dev(view.ptr, n, view.stride, E, Wp, ndim, K, d_out.data_ptr(), d_idx.data_ptr() if index else 0,
                           work.data_ptr(), nbytes, view.stream)
        view.synchronize()
        out[k0:k0 + K.size] = d_out.cpu().numpy()
        if index:
            idx[k0:k0 + K.size] = d_idx.cpu().numpy()
        del work, d_out, d_idx
    if not np.ndim(mass):
        out, idx = out[0], idx[0]
    return (out, idx) if index else out


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelIntervals:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are parse_chain's."""

    def get_param_hdi(self, mass=0.95, chain=None, **kwargs):
        """The highest-density interval of every parameter over the flattened used samples (bisip_amd.interval): ``(2,
        ndim)``, so that ``lo, hi = model.get_param_hdi()``; ``(len(mass), 2, ndim)`` for a sequence of masses.
        ``chain`` / ``discard`` / ``thin`` as parse_chain; a fit with the device sampler is reduced on the GPU
        (``chain='device'``: where the chain lies), an explicit ``chain`` or a host sampler's in NumPy."""
        from .utils import discard_thin
        s = self._device_chain_sampler(chain, kwargs, 'param_hdi')
        if s is not None:
            return s.param_hdi(mass, **discard_thin(kwargs))[..., 0, :]
        return hdi(self.parse_chain(chain, **kwargs), mass)[..., 0, :]


class DecompositionIntervals:
    """Mixin of PolynomialDecomposition (``_integrating_view`` is its ChainView of the integrating parameters)."""

    def get_integrating_hdi(self, mass=0.95, chain=None, **kwargs):
        """The highest-density interval of ``(m_total, log_tau_mean, m_norm)``: ``(2, 3)``, in the order of
        get_integrating_percentile; ``(len(mass), 2, 3)`` for a sequence of masses (kwargs as get_param_mean)."""
        return device_hdi(self._integrating_view(chain, kwargs), mass)[..., 0, :]


class BatchIntervals:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler)."""

    def get_param_hdi(self, mass=0.95, discard=0, thin=1):
        """The highest-density interval of every parameter of every spectrum, ``(2, E, ndim)`` -- ``(len(mass), 2, E,
        ndim)`` for a sequence of masses -- per spectrum ``interval.hdi`` of its flattened used samples, taken on the
        device for ``chain='device'`` and ``'host'`` alike.  A multi-GPU survey joins the ranks' blocks with
        ``gather(np.moveaxis(hdi, -2, 0))``."""
        return self._fitted().param_hdi(mass, discard=discard, thin=thin)

    def get_integrating_hdi(self, mass=0.95, discard=0, thin=1):
        """The highest-density interval of ``(m_total, log_tau_mean, m_norm)`` per spectrum, ``(2, E, 3)`` (``(len(mass),
        2, E, 3)`` for a sequence of masses)."""
        return self._decomposition_sampler().integrating_hdi(mass, self.log_tau, self.norm_factor, discard, thin)
