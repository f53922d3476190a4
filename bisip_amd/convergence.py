"""Convergence along the step axis: per-walker moments and the Gelman-Rubin potential scale reduction R-hat.

``get_autocorr_time`` needs a chain of 50 tau or more; a survey's runs are shorter.  What can be said of a short run is
whether the walkers of an ensemble agree with each other: every walker's series has a mean and a variance
(``walker_moments``), and R-hat (``gelman_rubin``) compares the spread of the means with the mean of the variances.
By default each series is cut into halves first (``split_chains``), so that a drift shows as well; it works from four
used samples up.

Walkers of an ensemble sampler are NOT independent chains: the stretch move makes every walker step along the line to
another one, so R-hat here is a screening number -- which fits of a survey to look at, which walkers are stuck -- used
beside the autocorrelation time, not a replacement for it.

* ``split_chains``, ``walker_moments``, ``gelman_rubin``, ``rhat``: the definitions, plain NumPy in float64;
* ``device_rhat`` runs ``bisip_chain_rhat_dev`` on a ChainView (bisip_amd.chainview) where the chain lies;
* ``ordered_rhat`` restates the order of every sum of that kernel (include/bisip_hip.h) in NumPy: the same bits.

A stored log-probability ``(n, W)`` is a chain of ``ndim = 1``.
"""

import numpy as np

__all__ = ('split_chains', 'walker_moments', 'gelman_rubin', 'rhat', 'segment_plan', 'ordered_rhat', 'device_rhat')


def _chain3(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError(f'R-hat needs the unflattened chain (n, nwalkers, ndim), got shape {x.shape}')
    return x


def split_chains(x, split=True):
    """The chains R-hat compares.  ``split=True``: with ``h = n // 2``, ``(h, 2 W, ndim)`` where chain ``half * W + w`` is
    ``x[:h, w]`` for half 0 and ``x[n - h:, w]`` for half 1 (the middle sample of an odd ``n`` belongs to neither);
    ``split=False``: ``x`` itself.  ValueError unless the chains have 2 samples or more and there are 2 or more."""
    x = _chain3(x)
    if split:
        n = x.shape[0]
        h = n // 2
        x = np.concatenate([x[:h], x[n - h:]], axis=1)
    if x.shape[0] < 2:
        raise ValueError(f'a chain of {x.shape[0]} sample(s) has no variance: R-hat needs 2 per chain, '
                         '4 used samples when split')
    if x.shape[1] < 2:
        raise ValueError('R-hat needs 2 chains or more')
    return x


def walker_moments(x):
    """``(mean, var)`` of every walker's own series, ``(W, ndim)`` each; the variance with ddof = 1."""
    x = _chain3(x)
    with np.errstate(all='ignore'):
        return np.mean(x, axis=0), np.var(x, axis=0, ddof=1)


def gelman_rubin(mean, var, L):
    """R-hat ``(ndim,)`` of M chains of length ``L`` from their means and variances ``(M, ndim)``:
    ``sqrt((L - 1) / L + Bn / Wn)`` with ``Wn`` the mean of the variances and ``Bn`` the variance (ddof = 1) of the means
    (B / L).  The IEEE result stands: NaN when both are 0, inf when only ``Wn`` is."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(all='ignore'):
        Wn = var.mean(axis=0)
        Bn = mean.var(axis=0, ddof=1)
        return np.sqrt((L - 1) / L + Bn / Wn)


def rhat(x, split=True):
    """(Split) R-hat of every parameter of a chain ``(n, W, ndim)``, ``(ndim,)``.  A float64 tensor on the GPU is
    reduced there (device_rhat)."""
    if type(x).__module__.split('.')[0] == 'torch' and getattr(x, 'is_cuda', False):
        from .chainview import ChainView
        if x.dim() != 3:
            raise ValueError(f'R-hat needs the unflattened chain (n, nwalkers, ndim), got shape {tuple(x.shape)}')
        return device_rhat(ChainView.of_tensor(x), split=split)[0]
    c = split_chains(x, split)
    return gelman_rubin(*walker_moments(c), c.shape[0])


# -- the device's order of summation ------------------------------------------------------------------------------------
LANES_WANTED, SEGMENT_MIN, TILE = 262144, 32, 256     # chain_rhat.hip: RH_LANES, RH_SEG_MIN, RH_THREADS


def segment_plan(L, columns, splits):
    """``(seg_len, nseg)``: how bisip_chain_rhat_dev cuts the ``L`` samples of a half into segments for a chain of
    ``columns = n_ensembles * walkers_per_ensemble * ndim`` columns -- a function of the shape alone."""
    tiles = -(-int(columns) // TILE)
    want = max(1, LANES_WANTED // (int(splits) * TILE * tiles))
    seg_len = max(SEGMENT_MIN, -(-int(L) // want))
    return seg_len, -(-int(L) // seg_len)


def _wave_sum(v):
    """The sum over the last axis in the order of a wave: element c goes to partial c mod 64, in turn, each from 0.0;
    the 64 partials are added pairwise 32, 16, ..., 1 apart."""
    M = v.shape[-1]
    rows = -(-M // 64)
    padded = np.zeros(v.shape[:-1] + (rows * 64,))
    padded[..., :M] = v
    padded = padded.reshape(v.shape[:-1] + (rows, 64))
    acc = np.zeros(v.shape[:-1] + (64,))
    for r in range(rows):
        k = min(64, M - 64 * r)          # (a lane beyond the last element adds nothing)
        acc[..., :k] = acc[..., :k] + padded[..., r, :k]
    d = 32
    while d >= 1:
        acc = acc[..., :d] + acc[..., d:2 * d]
        d //= 2
    return acc[..., 0]


def _variance(T1, T2, n):
    v = (T2 - (T1 * T1) / float(n)) / float(n - 1)
    return np.where(v < 0.0, 0.0, v)          # (a NaN stays)


def ordered_rhat(x, split=True, n_ensembles=1):
    """``(mean, var, rhat)`` of a chain ``(n, n_ensembles * Wp, ndim)`` with the bits bisip_chain_rhat_dev produces:
    ``(splits, n_ensembles, Wp, ndim)`` twice and ``(n_ensembles, ndim)``.  The order is the one include/bisip_hip.h
    states: sums shifted by the first sample of the half, sample after sample within a segment, segments in ascending
    order, chains to partial sums c mod 64 that are added pairwise."""
    x = _chain3(x)
    n, W, ndim = x.shape
    E = int(n_ensembles)
    if E < 1 or W % E:
        raise ValueError(f'{W} walkers do not divide into {E} ensembles')
    Wp, splits = W // E, (2 if split else 1)
    L = n // 2 if split else n
    if L < 2:
        raise ValueError(f'a chain of {L} sample(s) has no variance: R-hat needs 2 per chain, 4 used samples when split')
    if splits * Wp < 2:
        raise ValueError('R-hat needs 2 chains or more')
    C = W * ndim
    seg_len, nseg = segment_plan(L, C, splits)
    flat = x.reshape(n, C)
    mean, var = np.empty((splits, C)), np.empty((splits, C))
    with np.errstate(all='ignore'):
        for half in range(splits):
            blk = flat[(n - L if half else 0):][:L]
            c = blk[0]
            S1 = S2 = None
            for g in range(nseg):
                a1, a2 = np.zeros(C), np.zeros(C)
                for k in range(g * seg_len, min(L, (g + 1) * seg_len)):
                    d = blk[k] - c
                    a1 = a1 + d
                    a2 = a2 + d * d
                S1, S2 = (a1, a2) if g == 0 else (S1 + a1, S2 + a2)
            mean[half] = c + S1 / float(L)
            var[half] = _variance(S1, S2, L)
        mean, var = mean.reshape(splits, E, Wp, ndim), var.reshape(splits, E, Wp, ndim)
        # chains c = half * Wp + w of every (ensemble, parameter) along the last axis
        m = np.moveaxis(mean, 0, 1).reshape(E, splits * Wp, ndim).transpose(0, 2, 1)
        v = np.moveaxis(var, 0, 1).reshape(E, splits * Wp, ndim).transpose(0, 2, 1)
        M = splits * Wp
        dm = m - m[..., :1]
        V, T1, T2 = _wave_sum(v), _wave_sum(dm), _wave_sum(dm * dm)
        Wn, Bn = V / float(M), _variance(T1, T2, M)
        r = np.sqrt(float(L - 1) / float(L) + Bn / Wn)
    return mean, var, r


def device_rhat(view, split=True, moments=False):
    """R-hat ``(n_ensembles, ndim)`` (NumPy) of every ensemble of a ChainView, taken where the chain lies
    (bisip_chain_rhat_dev).  ``moments=True``: ``(rhat, mean, var)`` with the mean and variance (ddof = 1) of every chain,
    ``(splits, n_ensembles, Wp, ndim)`` each, ``splits = 2`` when split."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    splits = 2 if split else 1
    if n < 2 * splits:
        raise ValueError(f'a chain of {n // splits} sample(s) has no variance: R-hat needs 2 per chain, '
                         '4 used samples when split')
    if splits * Wp < 2:
        raise ValueError('R-hat needs 2 chains or more')
    nbytes = _hip.chain_rhat_workspace(n, E, Wp, ndim, splits)
    if nbytes < 0:
        raise ValueError(f'a chain of {E} ensembles of {Wp} walkers is too large for one launch')
    work = view.empty((nbytes,), torch.uint8) if nbytes else None
    out = view.empty((E, ndim), torch.float64)
    mean = view.empty((splits, E, Wp, ndim), torch.float64) if moments else None
    var = view.empty((splits, E, Wp, ndim), torch.float64) if moments else None
    _hip.chain_rhat_dev(view.ptr, n, view.stride, E, Wp, ndim, splits, mean.data_ptr() if moments else 0,
                        var.data_ptr() if moments else 0, out.data_ptr(), work.data_ptr() if nbytes else 0, nbytes,
                        view.stream)
    view.synchronize()
    if moments:
        return out.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
    return out.cpu().numpy()
