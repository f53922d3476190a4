"""Walker traces: per-step statistics over the walkers of an ensemble, the data of ``plot_traces``.

The reference's ``plot_traces`` (src/bisip/plotlib.py:17-54) draws one line per walker from a copy of the chain, to
show where the walkers have settled before ``discard`` is chosen.  Here the trace of a parameter is, for every used
sample, the percentiles and the mean of that step's walkers:

* ``host_trace`` takes them in NumPy: ``np.percentile(chain, p, axis=1)`` and ``np.mean(chain, axis=1)`` of a chain
  ``(n, W, ndim)``;
* ``device_trace`` runs ``bisip_chain_trace_dev`` on a ChainView (bisip_amd.chainview) where the chain lies: the same
  percentiles, double for double; the mean summed in a fixed order.

A stored log-probability ``(n, W)`` is traced as a chain of ``ndim = 1``.  ``used_steps`` gives the x axis: the index
among the stored samples of every sample that ``get_chain(discard, thin)`` keeps.
"""

import numpy as np

from .chainview import used_range

__all__ = ('MAX_PERCENTILES', 'check_percentiles', 'host_trace', 'device_trace', 'used_steps')

MAX_PERCENTILES = 8      # per bisip_chain_trace_dev call; device_trace goes in groups beyond that


def check_percentiles(p):
    """``p`` as a 1-D float64 array of percentiles in [0, 100] (a scalar becomes one entry)."""
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if p.ndim != 1:
        raise ValueError(f'percentiles must be a scalar or one-dimensional, got shape {p.shape}')
    if not np.all((p >= 0.0) & (p <= 100.0)):       # (a NaN fails too)
        raise ValueError('percentiles must be in [0, 100]')
    return p


def host_trace(chain, p):
    """``(pct (len(p), n, ndim), mean (n, ndim))`` over the walkers of a chain ``(n, W, ndim)`` in NumPy."""
    p = check_percentiles(p)
    chain = np.asarray(chain, dtype=np.float64)
    if chain.ndim != 3:
        raise ValueError(f'a trace needs the unflattened chain (n, nwalkers, ndim), got shape {chain.shape}')
    if chain.shape[0] < 1 or chain.shape[1] < 1:
        raise ValueError('no samples')
    pct = np.percentile(chain, p, axis=1) if p.size else np.empty((0, chain.shape[0], chain.shape[2]))
    return pct, np.mean(chain, axis=1)


def used_steps(n_total, discard=0, thin=1):
    """Index among ``n_total`` stored samples of every sample ``get_chain(discard, thin)`` keeps: ``discard + thin - 1
    + k * thin``."""
    first, n = used_range(n_total, discard, thin)
    return first + int(thin) * np.arange(n)


def device_trace(view, p=(), mean=True):
    """``(pct (len(p), n, n_ensembles, ndim), mean (n, n_ensembles, ndim))`` (NumPy) over the walkers of every ensemble
    at every sample of a ChainView, taken where the chain lies.  ``mean=False``: None in its place; ``p`` may be empty."""
    import torch
    from . import _hip
    p = check_percentiles(p)
    if p.size == 0 and not mean:
        raise ValueError('neither percentiles nor the mean asked for')
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    nbytes = _hip.chain_trace_workspace(n, E, Wp, ndim, min(p.size, MAX_PERCENTILES))
    if nbytes < 0:
        raise ValueError(f'a chain of {E} ensembles of {Wp} walkers is too large for one trace launch')
    work = view.empty((nbytes,), torch.uint8) if nbytes else None
    pct = view.empty((p.size, n, E, ndim), torch.float64)
    avg = view.empty((n, E, ndim), torch.float64) if mean else None
    k0 = 0
    while True:
        k1 = min(p.size, k0 + MAX_PERCENTILES)
        _hip.chain_trace_dev(view.ptr, n, view.stride, E, Wp, ndim, p[k0:k1], pct[k0:].data_ptr() if k1 > k0 else 0,
                             avg.data_ptr() if (mean and k0 == 0) else 0, work.data_ptr() if nbytes else 0, nbytes,
                             view.stream)
        k0 = k1
        if k0 >= p.size:
            break
    view.synchronize()
    return pct.cpu().numpy(), (avg.cpu().numpy() if mean else None)
