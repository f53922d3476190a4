"""Histograms of a posterior: the counts behind the reference's ``plot_histograms`` (src/bisip/plotlib.py:56-90,
``np.histogram`` of every parameter, 25 bins) and ``plot_corner`` (src/bisip/plotlib.py:233-259, corner's 1-D and
pairwise 2-D histograms, 20 bins).

Definition (what ``np.histogram`` / ``np.histogram2d`` count for equal-width bins):

* the edges of a range ``(lo, hi)`` are ``np.linspace(lo, hi, bins + 1)``; ``lo == hi`` becomes
  ``(lo - 0.5, hi + 0.5)`` first.  Edges are always made on the host;
* value ``x`` is in bin ``i`` iff ``edges[i] <= x < edges[i + 1]``; ``x == edges[bins]`` is in the last bin;
* everything else -- below or above the range, NaN -- is counted nowhere.  In a pair, a row outside the range in
  either coordinate is left out of that pair only.

``histogram_by_edges`` and ``pair_histograms_by_edges`` count on the host in NumPy.  The ``device_*`` functions run
``bisip_chain_range_dev`` / ``bisip_chain_histograms_dev`` / ``bisip_chain_pair_histograms_dev`` on a ChainView
(bisip_amd.chainview) on the GPU.  Both give the same integers.

A ``range`` argument is ``None`` (min and max of the samples, per ensemble and parameter; a non-finite sample raises
ValueError as NumPy does), ``'bounds'`` (the prior box: the same edges for every spectrum) or an array ``(ndim, 2)``
or ``(E, ndim, 2)``.
"""

import operator

import numpy as np

__all__ = ('check_bins', 'pair_index', 'edges_from_range', 'bin_index', 'histogram_by_edges',
           'pair_histograms_by_edges', 'resolve_range', 'host_histograms', 'host_pair_histograms',
           'device_param_range', 'device_histograms', 'device_pair_histograms')


def check_bins(bins):
    """``bins`` as an int >= 1 (equal-width bins only)."""
    if isinstance(bins, (bool, np.bool_)):
        raise TypeError('bins must be an integer')
    try:
        bins = operator.index(bins)
    except TypeError:
        raise TypeError(f'bins must be an integer, got {type(bins).__name__}') from None
    if bins < 1:
        raise ValueError(f'bins={bins}: at least one bin')
    return bins


def pair_index(ndim):
    """The pairs ``(j, k)``, ``j < k``, in the order of the pair histograms: ``np.triu_indices(ndim, 1)``."""
    return np.triu_indices(int(ndim), 1)


def check_range(rng):
    """A range array ``(..., 2)``: finite, ``lo <= hi``."""
    rng = np.asarray(rng, dtype=np.float64)
    if rng.ndim < 1 or rng.shape[-1] != 2:
        raise ValueError(f'a range must end in (lo, hi), got shape {rng.shape}')
    if not np.all(np.isfinite(rng)):
        raise ValueError('range must be finite')
    if np.any(rng[..., 0] > rng[..., 1]):
        raise ValueError('range: lo must be <= hi')
    return rng


def edges_from_range(rng, bins):
    """Bin edges ``(..., bins + 1)`` of ranges ``(..., 2)``: ``np.linspace(lo, hi, bins + 1)`` of every row,
    ``lo == hi`` widened by 0.5 on either side first (numpy.lib._histograms_impl._get_outer_edges)."""
    bins = check_bins(bins)
    rng = check_range(rng)
    lo, hi = rng[..., 0].copy(), rng[..., 1].copy()
    same = lo == hi
    lo[same] -= 0.5
    hi[same] += 0.5
    with np.errstate(over='ignore'):
        step = (hi - lo) / bins
    if np.all(step != 0) and np.all(np.isfinite(step)):
        return np.ascontiguousarray(np.linspace(lo, hi, bins + 1, axis=-1))
    # np.linspace takes another route (for the whole array) when a step underflows to 0: row by row then
    out = np.empty(lo.shape + (bins + 1,))
    for i in np.ndindex(lo.shape):
        out[i] = np.linspace(lo[i], hi[i], bins + 1)
    return out


def bin_index(x, edges):
    """Bin of every value of ``x`` among ``edges (bins + 1,)``; -1 where it has none."""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.size - 1
    idx = np.searchsorted(edges, x, side='right') - 1
    idx[x == edges[-1]] = bins - 1
    with np.errstate(invalid='ignore'):
        inside = (x >= edges[0]) & (x <= edges[-1])
    idx[~inside] = -1
    return idx


def _columns(x, edges):
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    if x.ndim != 2 or edges.ndim != 2 or edges.shape[0] != x.shape[1] or edges.shape[1] < 2:
        raise ValueError(f'expected samples (n, ndim) and edges (ndim, bins + 1), got {x.shape} and {edges.shape}')
    return x, edges


def histogram_by_edges(x, edges):
    """Counts (int64) of ``x (n,)`` within ``edges (bins + 1,)``: ``(bins,)``; or of every column of ``x (n, ndim)``
    within its row of ``edges (ndim, bins + 1)``: ``(ndim, bins)``."""
    if np.ndim(x) == 1:
        return histogram_by_edges(np.asarray(x)[:, None], np.asarray(edges)[None])[0]
    x, edges = _columns(x, edges)
    bins = edges.shape[1] - 1
    out = np.empty((x.shape[1], bins), dtype=np.int64)
    for q in range(x.shape[1]):
        idx = bin_index(x[:, q], edges[q])
        out[q] = np.bincount(idx[idx >= 0], minlength=bins)
    return out


def pair_histograms_by_edges(x, edges):
    """Counts (int64) of every pair of columns of ``x (n, ndim)`` within ``edges (ndim, bins + 1)``:
    ``(npairs, bins, bins)`` in ``pair_index`` order, first axis of a pair = the bin of its first parameter."""
    x, edges = _columns(x, edges)
    bins = edges.shape[1] - 1
    idx = np.stack([bin_index(x[:, q], edges[q]) for q in range(x.shape[1])], axis=1) if x.shape[1] else x.astype(int)
    jj, kk = pair_index(x.shape[1])
    out = np.empty((jj.size, bins, bins), dtype=np.int64)
    for q, (j, k) in enumerate(zip(jj, kk)):
        both = (idx[:, j] >= 0) & (idx[:, k] >= 0)
        out[q] = np.bincount(idx[both, j] * bins + idx[both, k], minlength=bins * bins).reshape(bins, bins)
    return out


def resolve_range(rng, n_ensembles, ndim, bounds=None, data_range=None):
    """The ``range`` argument of the public functions as an array ``(n_ensembles, ndim, 2)``.  ``bounds``: the prior
    box ``(2, ndim)`` for ``'bounds'``; ``data_range``: a function that returns ``(minmax (E, ndim, 2), n_nonfinite
    (E, ndim))`` of the used samples, called for ``None``."""
    E, ndim = int(n_ensembles), int(ndim)
    if rng is None:
        minmax, bad = data_range()
        if np.any(bad):
            raise ValueError(f'{int(np.sum(bad))} of the samples are not finite: their range cannot be taken, pass one')
        return check_range(np.reshape(minmax, (E, ndim, 2)))
    if isinstance(rng, str):
        if rng != 'bounds':
            raise ValueError(f"range={rng!r}: None, 'bounds' or an array")
        if bounds is None:
            raise ValueError("range='bounds' needs parameter bounds")
        b = np.asarray(bounds, dtype=np.float64)
        if b.shape != (2, ndim):
            raise ValueError(f'bounds must have shape (2, {ndim}), got {b.shape}')
        rng = b.T
    rng = check_range(rng)
    if rng.shape not in ((ndim, 2), (E, ndim, 2)):
        raise ValueError(f'range must have shape ({ndim}, 2) or ({E}, {ndim}, 2), got {rng.shape}')
    return np.ascontiguousarray(np.broadcast_to(rng, (E, ndim, 2)))


def host_data_range(flat):
    """``(minmax (ndim, 2), n_nonfinite (ndim,))`` of a flat chain ``(n, ndim)``."""
    flat = np.asarray(flat, dtype=np.float64)
    bad = np.sum(~np.isfinite(flat), axis=0)
    if flat.shape[0] < 1:
        raise ValueError('no samples')
    return np.stack([flat.min(axis=0), flat.max(axis=0)], axis=-1), bad


def host_histograms(flat, bins=25, rng=None, bounds=None):
    """``(counts (ndim, bins), edges (ndim, bins + 1))`` of a flat chain ``(n, ndim)`` on the host."""
    bins = check_bins(bins)
    flat = np.asarray(flat, dtype=np.float64)
    if flat.ndim != 2:
        raise ValueError('Flatten chain by passing flat=True.')
    r = resolve_range(rng, 1, flat.shape[1], bounds, lambda: host_data_range(flat))
    edges = edges_from_range(r[0], bins)
    return histogram_by_edges(flat, edges), edges


def host_pair_histograms(flat, bins=20, rng=None, bounds=None):
    """``(counts (npairs, bins, bins), edges (ndim, bins + 1), pairs)`` of a flat chain ``(n, ndim)`` on the host."""
    bins = check_bins(bins)
    flat = np.asarray(flat, dtype=np.float64)
    if flat.ndim != 2:
        raise ValueError('Flatten chain by passing flat=True.')
    r = resolve_range(rng, 1, flat.shape[1], bounds, lambda: host_data_range(flat))
    edges = edges_from_range(r[0], bins)
    return pair_histograms_by_edges(flat, edges), edges, pair_index(flat.shape[1])


# -- device drivers ---------------------------------------------------------------------------------------------
def device_param_range(view):
    """``(minmax (n_ensembles, ndim, 2), n_nonfinite (n_ensembles, ndim))`` (NumPy) of the samples of a ChainView
    (bisip_amd.chainview).  Min and max are over the finite values."""
    import torch
    from . import _hip
    E, ndim = view.n_ensembles, view.ndim
    out = view.empty((E, ndim, 2), torch.float64)
    bad = view.empty((E, ndim), torch.int64)
    _hip.chain_range_dev(view.ptr, view.n, view.stride, E, view.walkers_per_ensemble, ndim, out.data_ptr(),
                         bad.data_ptr(), view.stream)
    view.synchronize()
    return out.cpu().numpy(), bad.cpu().numpy()


def _device_counts(entry, shape_of, view, edges):
    import torch
    E, ndim = view.n_ensembles, view.ndim
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 3 or edges.shape[:2] != (E, ndim) or edges.shape[2] < 2:
        raise ValueError(f'edges must have shape ({E}, {ndim}, bins + 1), got {edges.shape}')
    bins = edges.shape[2] - 1
    d_edges = view.upload(edges)
    counts = view.empty(shape_of(E, ndim, bins), torch.int64)
    entry(view.ptr, view.n, view.stride, E, view.walkers_per_ensemble, ndim, d_edges.data_ptr(), bins,
          counts.data_ptr(), view.stream)
    view.synchronize()
    return counts.cpu().numpy()


def device_histograms(view, edges):
    """Counts ``(n_ensembles, ndim, bins)`` int64 (NumPy) of the samples of a ChainView within ``edges (n_ensembles,
    ndim, bins + 1)``, counted where the chain lies."""
    from . import _hip
    return _device_counts(_hip.chain_histograms_dev, lambda E, d, b: (E, d, b), view, edges)


def device_pair_histograms(view, edges):
    """Counts ``(n_ensembles, npairs, bins, bins)`` int64 (NumPy) of every pair of parameters, ``pair_index`` order."""
    from . import _hip
    if view.ndim < 2:
        raise ValueError('pair histograms need at least two parameters')
    return _device_counts(_hip.chain_pair_histograms_dev, lambda E, d, b: (E, d * (d - 1) // 2, b, b), view, edges)
