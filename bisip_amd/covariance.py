"""How the parameters co-vary over the posterior, and the best stored sample.

Cole-Cole ``m`` and ``c``, ``log_tau`` and ``c``, the polynomial coefficients of the Debye decomposition are strongly
correlated; ``get_corner_histograms`` shows it, ``np.cov`` / ``np.corrcoef`` of the flattened used samples say it in
numbers.  The stored sample of largest log-probability is the maximum-a-posteriori point of the run: what is plotted as
"the fit" and compared with the median.

* ``flat_cov``, ``corr_from_cov``, ``best_sample``: the definitions, plain NumPy in float64;
* ``device_cov`` and ``device_best_sample`` run ``bisip_chain_cov_dev`` and ``bisip_chain_best_sample_dev`` on ChainViews
  (bisip_amd.chainview) where the chain lies;
* ``ordered_cov`` restates the order of every sum of the covariance kernel (include/bisip_hip.h) in NumPy: the same bits;
  ``plan`` and ``best_plan`` are the kernels' shape-only plans;
* ``ModelCovariance`` and ``BatchCovariance`` are the ``get_param_cov`` / ``get_param_corr`` / ``get_best_sample`` methods
  of the models (bisip_amd.utils.utils) and of SpectraBatch, as mixins.

The rows of an ensemble are numbered ``k * Wp + w`` (sample ``k``, walker ``w``): the order of ``get_chain(flat=True)``.
"""

import numpy as np

__all__ = ('flat_cov', 'corr_from_cov', 'best_sample', 'plan', 'best_plan', 'ordered_cov', 'device_cov',
           'device_best_sample', 'ModelCovariance', 'BatchCovariance')


def _is_device_tensor(x):
    return type(x).__module__.split('.')[0] == 'torch' and getattr(x, 'is_cuda', False)


def _shape4(shape, n_ensembles):
    """``(n, E, Wp, ndim)`` of a chain ``(n, E * Wp, ndim)`` or, flat, ``(N, ndim)`` with one ensemble."""
    E = int(n_ensembles)
    if len(shape) == 2:
        if E != 1:
            raise ValueError('a flat chain (N, ndim) is one ensemble; pass the unflattened chain (n, nwalkers, ndim)')
        return int(shape[0]), 1, 1, int(shape[1])
    if len(shape) != 3:
        raise ValueError(f'expected a chain (n, nwalkers, ndim) or a flat one (N, ndim), got shape {tuple(shape)}')
    n, W, ndim = (int(s) for s in shape)
    if E < 1 or W % E:
        raise ValueError(f'{W} walkers do not divide into {E} ensembles')
    return n, E, W // E, ndim


def _rows(x, n_ensembles):
    """The rows of every ensemble, ``(E, N, ndim)``, in the order ``k * Wp + w``."""
    x = np.asarray(x, dtype=np.float64)
    n, E, Wp, ndim = _shape4(x.shape, n_ensembles)
    return x.reshape(n, E, Wp, ndim).transpose(1, 0, 2, 3).reshape(E, n * Wp, ndim)


def _view_of(x, n_ensembles):
    from .chainview import ChainView
    n, E, Wp, ndim = _shape4(tuple(x.shape), n_ensembles)
    return ChainView(x.contiguous(), n, E, Wp, ndim)


def flat_cov(x, n_ensembles=1):
    """``(mean (E, ndim), cov (E, ndim, ndim))`` of every ensemble's rows of a chain ``(n, E * Wp, ndim)`` -- or of a flat
    chain ``(N, ndim)``, one ensemble: ``np.mean(rows, axis=0)`` and ``np.cov(rows.T, ddof=1)``.  ValueError with fewer
    than 2 rows.  A float64 tensor on the GPU is reduced there (device_cov)."""
    if _is_device_tensor(x):
        return device_cov(_view_of(x, n_ensembles), mean=True)
    rows = _rows(x, n_ensembles)
    E, N, ndim = rows.shape
    if N < 2:
        raise ValueError(f'a covariance needs 2 rows, got {N}')
    with np.errstate(all='ignore'):
        mean = rows.mean(axis=1)
        cov = np.stack([np.atleast_2d(np.cov(rows[e].T, ddof=1)) for e in range(E)])
    return mean, cov


def corr_from_cov(cov):
    """The correlation matrix of a covariance ``(..., ndim, ndim)`` by np.corrcoef's own steps: divided by the square
    roots of the diagonal, rows then columns, and clipped to [-1, 1].  NaN where a variance is 0."""
    cov = np.asarray(cov, dtype=np.float64)
    with np.errstate(all='ignore'):
        s = np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1))
        c = cov / s[..., :, None]
        c = c / s[..., None, :]
        return np.clip(c, -1.0, 1.0)


def best_sample(x, lp, n_ensembles=1):
    """``(theta (E, ndim), logp (E,), index (E,))``: of every ensemble the stored sample of largest log-probability.
    ``x (n, E * Wp, ndim)`` with ``lp (n, E * Wp)``, or flat ``(N, ndim)`` with ``(N,)``.  ``index = np.argmax`` of the
    ensemble's values in row order with NaN read as -inf: a NaN never wins, the lowest index wins among equals, 0 when all
    are NaN or -inf.  ``logp`` is the stored value at that index.  Float64 tensors on the GPU are searched there."""
    if _is_device_tensor(x) and _is_device_tensor(lp):
        view = _view_of(x, n_ensembles)
        return device_best_sample(view, _view_of(lp.reshape(view.n, -1, 1), n_ensembles))
    rows = _rows(x, n_ensembles)
    E, N, ndim = rows.shape
    lp = np.asarray(lp, dtype=np.float64)
    if lp.shape != np.shape(x)[:-1]:
        raise ValueError(f'log-probability of shape {lp.shape} for a chain of shape {np.shape(x)}')
    lpr = _rows(lp[..., None], n_ensembles)[:, :, 0]
    index = np.argmax(np.where(np.isnan(lpr), -np.inf, lpr), axis=1).astype(np.int64)
    e = np.arange(E)
    return rows[e, index], lpr[e, index], index


# -- the device's order of summation ------------------------------------------------------------------------------------
WORKGROUPS_WANTED, ONE_SEGMENT_ENSEMBLES, SEGMENT_MAX = 2048, 256, 1 << 30   # chain_cov.hip: CV_WGS, CV_ONE_SEGMENT, CV_SEG_MAX
COV_SEGMENT_MIN, BEST_SEGMENT_MIN = 1024, 4096                               # CV_SEG_MIN, BS_SEG_MIN


def _row_plan(N, E, seg_min):
    N, E = int(N), int(E)
    seg_rows = N if E >= ONE_SEGMENT_ENSEMBLES else max(seg_min, -(-N // (WORKGROUPS_WANTED // E)))
    seg_rows = min(seg_rows, SEGMENT_MAX)
    return seg_rows, -(-N // seg_rows)


def plan(n_samples, n_ensembles, walkers_per_ensemble, ndim):
    """``(seg_rows, nseg, slots)``: how bisip_chain_cov_dev cuts the ``n_samples * walkers_per_ensemble`` rows of an
    ensemble into segments, and over how many row slots it spreads the rows of one -- a function of the shape alone."""
    return _row_plan(int(n_samples) * int(walkers_per_ensemble), n_ensembles, COV_SEGMENT_MIN) + (256 if ndim <= 8 else 64,)


def best_plan(n_samples, n_ensembles, walkers_per_ensemble):
    """``(seg_rows, nseg)`` of bisip_chain_best_sample_dev."""
    return _row_plan(int(n_samples) * int(walkers_per_ensemble), n_ensembles, BEST_SEGMENT_MIN)


def ordered_cov(x, n_ensembles=1):
    """``(mean (E, ndim), cov (E, ndim, ndim))`` with the bits bisip_chain_cov_dev produces, in the order
    include/bisip_hip.h states: sums shifted by the ensemble's first row; row ``i`` of a segment to slot ``i mod T``, a
    slot's rows in ascending order; slots pairwise within runs of 64, the runs in ascending order; segments in ascending
    order; products rounded on their own."""
    rows = _rows(x, n_ensembles)
    E, N, ndim = rows.shape
    if N < 2:
        raise ValueError(f'a covariance needs 2 rows, got {N}')
    seg_rows, nseg, T = _row_plan(N, E, COV_SEGMENT_MIN) + (256 if ndim <= 8 else 64,)
    ju, ku = np.triu_indices(ndim)                   # P_jk row by row, k >= j
    NS = ndim + ju.size
    with np.errstate(all='ignore'):
        c = rows[:, 0, :]
        total = None
        for g in range(nseg):
            r0, r1 = g * seg_rows, min(N, (g + 1) * seg_rows)
            acc = np.zeros((E, T, NS))
            for t0 in range(r0, r1, T):
                d = rows[:, t0:min(r1, t0 + T)] - c[:, None, :]
                k = d.shape[1]                       # (a slot beyond the last row adds nothing)
                acc[:, :k, :ndim] = acc[:, :k, :ndim] + d
                acc[:, :k, ndim:] = acc[:, :k, ndim:] + d[:, :, ju] * d[:, :, ku]
            acc = acc.reshape(E, T // 64, 64, NS)
            w = 32
            while w >= 1:
                acc = acc[:, :, :w] + acc[:, :, w:2 * w]
                w //= 2
            s = acc[:, 0, 0]
            for q in range(1, T // 64):
                s = s + acc[:, q, 0]
            total = s if g == 0 else total + s
        S, P = total[:, :ndim], total[:, ndim:]
        mean = c + S / float(N)
        tri = (P - (S[:, ju] * S[:, ku]) / float(N)) / float(N - 1)
        tri = np.where((ju == ku) & (tri < 0.0), 0.0, tri)          # (a NaN stays)
        cov = np.empty((E, ndim, ndim))
        cov[:, ju, ku] = tri
        cov[:, ku, ju] = tri
    return mean, cov


def device_cov(view, mean=False):
    """``np.cov`` of every ensemble's rows of a ChainView, ``(n_ensembles, ndim, ndim)`` (NumPy), taken where the chain
    lies (bisip_chain_cov_dev).  ``mean=True``: ``(mean (n_ensembles, ndim), cov)``."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    if n * Wp < 2:
        raise ValueError(f'a covariance needs 2 rows, got {n * Wp}')
    nbytes = _hip.chain_cov_workspace(n, E, Wp, ndim)
    if nbytes < 0:
        raise ValueError(f'a chain of {E} ensembles of {Wp} walkers is too large for one launch')
    work = view.empty((nbytes,), torch.uint8) if nbytes else None
    cov = view.empty((E, ndim, ndim), torch.float64)
    m = view.empty((E, ndim), torch.float64) if mean else None
    _hip.chain_cov_dev(view.ptr, n, view.stride, E, Wp, ndim, m.data_ptr() if mean else 0, cov.data_ptr(),
                       work.data_ptr() if nbytes else 0, nbytes, view.stream)
    view.synchronize()
    if mean:
        return m.cpu().numpy(), cov.cpu().numpy()
    return cov.cpu().numpy()


def device_best_sample(view, logp_view):
    """``(theta (n_ensembles, ndim), logp (n_ensembles,), index (n_ensembles,))`` (NumPy) of the chain of ``view`` and the
    log-probability of ``logp_view``, a ChainView of ``ndim = 1`` over the same samples, found where they lie
    (bisip_chain_best_sample_dev)."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    if (logp_view.n, logp_view.n_ensembles, logp_view.walkers_per_ensemble, logp_view.ndim) != (n, E, Wp, 1):
        raise ValueError('the log-probability does not belong to the samples of the chain')
    nbytes = _hip.chain_best_sample_workspace(n, E, Wp)
    if nbytes < 0:
        raise ValueError(f'a chain of {E} ensembles of {Wp} walkers is too large for one launch')
    work = view.empty((nbytes,), torch.uint8) if nbytes else None
    theta = view.empty((E, ndim), torch.float64)
    best = view.empty((E,), torch.float64)
    index = view.empty((E,), torch.int64)
    _hip.chain_best_sample_dev(view.ptr, view.stride, logp_view.ptr, logp_view.stride, n, E, Wp, ndim, theta.data_ptr(),
                               best.data_ptr(), index.data_ptr(), work.data_ptr() if nbytes else 0, nbytes, view.stream)
    view.synchronize()
    return theta.cpu().numpy(), best.cpu().numpy(), index.cpu().numpy()


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelCovariance:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are parse_chain's."""

    def get_param_cov(self, chain=None, **kwargs):
        """The posterior covariance of the parameters, ``np.cov(chain.T)`` of the flattened used samples, ``(ndim,
        ndim)``.  ``chain`` / ``discard`` / ``thin`` as parse_chain; a fit with the device sampler is reduced on the GPU
        (``chain='device'``: where the chain lies), an explicit ``chain`` or a host sampler's in NumPy
        (bisip_amd.covariance)."""
        from .utils import discard_thin
        s = self._device_chain_sampler(chain, kwargs, 'param_cov')
        if s is not None:
            return s.param_cov(**discard_thin(kwargs))[0]
        return flat_cov(self.parse_chain(chain, **kwargs))[1][0]

    def get_param_corr(self, chain=None, **kwargs):
        """The posterior correlation matrix, ``np.corrcoef(chain.T)``, ``(ndim, ndim)``: NaN where a parameter does not
        vary.  Arguments as get_param_cov."""
        return corr_from_cov(self.get_param_cov(chain, **kwargs))

    def get_best_sample(self, **kwargs):
        """``(theta (ndim,), log_prob)``: the stored sample of largest log-probability among the used ones -- the
        maximum-a-posteriori point of the run.  ``discard`` / ``thin`` as for ``get_chain``."""
        from .utils import discard_thin, warn_if_nothing_discarded
        kind, src = self._trace_source(None, kwargs)
        warn_if_nothing_discarded(kwargs)      # same advice as parse_chain
        if kind == 'device':
            theta, lp, _ = src.best_sample(**discard_thin(kwargs))
        else:
            theta, lp, _ = best_sample(src, np.asarray(self._sampler.get_log_prob(**discard_thin(kwargs))))
        return theta[0], float(lp[0])


class BatchCovariance:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler)."""

    def get_param_cov(self, discard=0, thin=1):
        """The posterior covariance of every spectrum's parameters, ``(E, ndim, ndim)`` -- per spectrum ``np.cov`` of its
        flattened used samples (bisip_amd.covariance) -- taken on the device for ``chain='device'`` and ``'host'`` alike.
        A multi-GPU survey joins the ranks' blocks with ``gather(get_param_cov(...))``."""
        return self._fitted().param_cov(discard=discard, thin=thin)

    def get_param_corr(self, discard=0, thin=1):
        """The posterior correlation matrix of every spectrum, ``(E, ndim, ndim)``; NaN where a parameter does not vary."""
        return self._fitted().param_corr(discard=discard, thin=thin)

    def get_best_sample(self, discard=0, thin=1):
        """``(theta (E, ndim), logp (E,))``: every spectrum's stored sample of largest log-probability among the used
        ones."""
        theta, lp, _ = self._fitted().best_sample(discard=discard, thin=thin)
        return theta, lp
