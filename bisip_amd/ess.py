"""Effective sample size (bulk, tail, of the mean) and the Monte-Carlo standard error of the mean.

R-hat (bisip_amd.convergence) says whether the walkers agree; the effective sample size says how much the other numbers
of a posterior table are worth: ``S`` correlated samples carry the information of ``ESS`` independent ones, and the mean
is known to ``sd / sqrt(ESS)``.  ``get_autocorr_time`` needs a chain of 50 tau or more, normalises every walker by its
own variance (walkers that disagree are never seen) and says nothing about the tails, where the percentiles and the HDI
come from.  The estimator here is that of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), as Stan and ArviZ
compute it: split chains, the autocovariance combined over the chains with the between-chain variance, Geyer's initial
positive and initial monotone sequences, rank-normalisation for the bulk and quantile indicators for the tail.

Walkers of an ensemble sampler are NOT independent chains: the stretch move makes every walker step along the line to
another one, so the between-walker term is a screening device, as R-hat is -- a small ESS is a finding, a large one is
not a proof.

The definition, for the chains ``c (L, M)`` of one parameter (``convergence.split_chains``: with ``h = n // 2`` chain
``half * W + w`` is ``x[:h, w]`` or ``x[n - h:, w]``; the middle sample of an odd ``n`` belongs to neither), ``S = L * M``:

1. a value that is not finite gives NaN;  2. ``c.max() - c.min() < np.finfo(float).resolution`` gives ``S``;
3. the biased autocovariance of every chain, ``a[k, m] = (1 / L) sum_{t < L - k} y[t, m] * y[t + k, m]`` with ``y = c -
   c.mean(axis=0)``, as direct sums (what the device computes); ``abar[k]`` its mean over the chains;
4. ``mean_var = abar[0] * L / (L - 1)``; ``var_plus = abar[0]``, plus ``np.var(chain means, ddof=1)`` when ``M > 1``;
5. ``rho(t) = 1 - (mean_var - abar[t]) / var_plus``;
6. Geyer's initial positive sequence: ``rho = zeros(L)``, ``rho[0] = 1``, ``rho[1] = rho(1)``, ``even = 1``, ``odd = rho(1)``,
   ``t = 1``; while ``t < L - 3 and even + odd > 0``: ``even = rho(t + 1)``, ``odd = rho(t + 2)``, both stored if ``even + odd
   >= 0``, ``t += 2``; then ``max_t = t - 2`` and, if ``even > 0``, ``rho[max_t + 1] = even``;
7. the initial monotone sequence: for ``t = 1, 3, ... <= max_t - 2``, if ``rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]``
   both become ``(rho[t - 1] + rho[t]) / 2``;
8. ``tau = -1 + 2 * sum(rho[:max_t + 1]) + sum(rho[max_t + 1:max_t + 2])``;  9. ``tau = max(tau, 1 / log10(S))``;
10. ``ESS = S / tau``.

* ``ndtri``, ``z_scale``, ``autocov``, ``ess_of_chains``, ``ess``, ``mcse_mean``: the definitions, plain NumPy in float64;
* ``device_rank_normalize`` and ``device_ess`` run ``bisip_chain_rank_normalize_dev`` and ``bisip_chain_ess_dev`` on a
  ChainView (bisip_amd.chainview) where the chain lies;
* ``ModelEss`` and ``BatchEss`` are the ``get_ess`` / ``get_mcse_mean`` / ``get_log_prob_ess`` methods of the models
  (bisip_amd.utils.utils) and of SpectraBatch, as mixins.

A stored log-probability ``(n, W)`` is a chain of ``ndim = 1``.
"""

import numpy as np

from .convergence import split_chains

__all__ = ('KINDS', 'ndtri', 'z_scale', 'autocov', 'ess_of_chains', 'ess', 'mcse_mean', 'round_lags',
           'device_rank_normalize', 'device_ess', 'device_mcse_mean', 'ModelEss', 'BatchEss')

KINDS = ('bulk', 'tail', 'mean')
TAIL_PERCENTILES = (5.0, 95.0)
RANK_PASS_BYTES = 1 << 32          # device_rank_normalize: gathered columns of one pass of ensembles
MAX_THRESHOLDS = 8                 # chain_ess.hip: ESS_MAX_THRESHOLDS

# Wichura (1988), Algorithm AS 241, routine PPND16: the published coefficients, highest power first
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _chain3(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError(f'the ESS needs the unflattened chain (n, nwalkers, ndim), got shape {x.shape}')
    return x


def _horner(coef, r):
    v = coef[0] * r
    for c in coef[1:-1]:
        v = (v + c) * r
    return v + coef[-1]


def ndtri(p):
    """The inverse of the standard normal distribution function by Wichura's PPND16 (relative accuracy about 1e-16),
    vectorised: the rational functions of ``statistics.NormalDist.inv_cdf`` in the same order of operations.  0 and 1 give
    -inf and +inf; NaN, or a value outside [0, 1], gives NaN."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all='ignore'):
        q = p - 0.5
        central = np.abs(q) <= 0.425
        r = 0.180625 - q * q
        x = _horner(_A, r) * q / _horner(_B, r)
        r = np.sqrt(-np.log(np.where(q <= 0.0, p, 1.0 - p)))
        mid = _horner(_C, r - 1.6) / _horner(_D, r - 1.6)
        far = _horner(_E, r - 5.0) / _horner(_F, r - 5.0)
        tail = np.where(r <= 5.0, mid, far)
        tail = np.where(np.isinf(r), np.inf, tail)               # p = 0 or 1
        x = np.where(central, x, np.where(q < 0.0, -tail, tail))
        return np.where((p >= 0.0) & (p <= 1.0), x, np.nan)


def z_scale(x):
    """Rank-normalisation of every parameter of a chain ``(n, W, ndim)``: ``ndtri((r - 3 / 8) / (N + 1 / 4))`` with ``r``
    the average rank, from 1, of each value among all ``N = n * W`` samples of the parameter (ties share the mean of their
    ranks: a walker that rejects repeats its value exactly).  Every sample takes part in the ranking; for an even ``n``
    this is ranking the split chains themselves, for an odd ``n`` the middle sample, which belongs to neither half,
    takes part in the ranking only.  A value that is not finite makes every ``z`` of that parameter NaN."""
    x = _chain3(x)
    n, W, ndim = x.shape
    N = n * W
    flat = x.reshape(N, ndim)
    z = np.empty((N, ndim))
    for d in range(ndim):
        col = flat[:, d]
        if not np.isfinite(col).all():
            z[:, d] = np.nan
            continue
        s = np.sort(col)
        below, upto = np.searchsorted(s, col, 'left'), np.searchsorted(s, col, 'right')
        r = (below + upto + 1) / 2.0                             # the mean of the ranks below + 1 ... upto
        z[:, d] = ndtri((r - 0.375) / (N + 0.25))
    return z.reshape(n, W, ndim)


def _lag(y, k):
    L = y.shape[0]
    return np.einsum('tm,tm->m', y[:L - k], y[k:]) / L


def autocov(c):
    """The biased autocovariance of every chain of ``c (L, M)`` at every lag, ``(L, M)``: ``a[k, m] = (1 / L) sum_{t < L -
    k} y[t, m] * y[t + k, m]`` with ``y = c - c.mean(axis=0)``, as direct sums."""
    c = np.asarray(c, dtype=np.float64)
    y = c - c.mean(axis=0)
    return np.stack([_lag(y, k) for k in range(c.shape[0])])


def ess_of_chains(c, margins=False):
    """The effective sample size of the chains ``c (L, M)`` of one quantity (the module docstring holds the steps), a
    float.  The lags are taken as the sequence asks for them, which changes nothing.  ``margins=True``: ``(ess, smallest
    |even + odd| met where the sequence decides to go on, smallest |even| where it ends, the last lag it took)``, inf and
    0 where no decision was made: how far the inputs are from a decision that rounding could turn."""
    c = np.asarray(c, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] < 2:
        raise ValueError(f'expected chains (L, M) of 2 samples or more, got shape {c.shape}')
    L, M = c.shape
    S = L * M
    gap_sum = gap_even = np.inf
    t = 0

    def result(value):
        return (float(value), gap_sum, gap_even, t) if margins else float(value)

    if not np.isfinite(c).all():
        return result(np.nan)
    if c.max() - c.min() < np.finfo(float).resolution:
        return result(S)
    means = c.mean(axis=0)
    y = c - means
    abar = {}

    def rho_at(t):
        if t not in abar:
            abar[t] = _lag(y, t).mean()
        return 1.0 - (mean_var - abar[t]) / var_plus

    abar[0] = _lag(y, 0).mean()
    mean_var = abar[0] * L / (L - 1.0)
    var_plus = abar[0] + (np.var(means, ddof=1) if M > 1 else 0.0)
    rho = np.zeros(L)
    rho[0] = 1.0
    rho[1] = rho_at(1)
    even, odd, t = 1.0, rho[1], 1
    while t < L - 3:
        gap_sum = min(gap_sum, abs(even + odd))
        if not even + odd > 0.0:
            break
        even, odd = rho_at(t + 1), rho_at(t + 2)
        if even + odd >= 0.0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    gap_even = abs(even)
    if even > 0.0:
        rho[max_t + 1] = even
    for k in range(1, max_t - 1, 2):
        if rho[k + 1] + rho[k + 2] > rho[k - 1] + rho[k]:
            rho[k + 1] = rho[k + 2] = (rho[k - 1] + rho[k]) / 2.0
    tau = -1.0 + 2.0 * np.sum(rho[:max_t + 1]) + np.sum(rho[max_t + 1:max_t + 2])
    tau = max(tau, 1.0 / np.log10(S))
    return result(S / tau)


def _chains(x, split):
    """``split_chains`` for the ESS: a single unsplit walker is a chain too (``M = 1``)."""
    x = _chain3(x)
    n = x.shape[0]
    if n < (4 if split else 2):
        raise ValueError(f'a chain of {n // 2 if split else n} sample(s) has no variance: the ESS needs 2 per chain, '
                         '4 used samples when split')
    if not split and x.shape[1] == 1:
        return x
    return split_chains(x, split)


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError(f'kind={kind!r}: one of {KINDS}')
    return kind


def _is_device_tensor(x):
    return type(x).__module__.split('.')[0] == 'torch' and getattr(x, 'is_cuda', False)


def ess(x, kind='bulk', split=True):
    """The effective sample size of every parameter of a chain ``(n, W, ndim)``, ``(ndim,)``:

    * ``'mean'``: ``ess_of_chains`` of the (split) chains of ``x``;
    * ``'bulk'``: the same of ``z_scale(x)``: how well the centre of the distribution is known, whatever its scale;
    * ``'tail'``: the smaller of the two of the indicators ``x <= q`` for ``q`` the 5th and the 95th percentile of the
      parameter over all samples: how well the tails are known, which is what an interval needs.

    A value that is not finite gives NaN for its parameter.  ValueError unless ``n >= 4`` (2 when not split).  Walkers of
    an ensemble are not independent chains: the between-walker term is a screening device.  A float64 tensor on the GPU is
    reduced there (device_ess)."""
    _check_kind(kind)
    if _is_device_tensor(x):
        from .chainview import ChainView
        if x.dim() != 3:
            raise ValueError(f'the ESS needs the unflattened chain (n, nwalkers, ndim), got shape {tuple(x.shape)}')
        return device_ess(ChainView.of_tensor(x), kind, split)[0]
    x = _chain3(x)
    _chains(x[:, :, :1], split)                                   # (the shape is refused before any work)
    ndim = x.shape[2]
    out = np.empty(ndim)
    if kind == 'tail':
        for d in range(ndim):
            col = x[:, :, d:d + 1]
            if not np.isfinite(col).all():
                out[d] = np.nan
                continue
            out[d] = min(ess_of_chains(_chains((col <= np.percentile(col.ravel(), p)).astype(np.float64), split)[:, :, 0])
                         for p in TAIL_PERCENTILES)
        return out
    c = _chains(z_scale(x) if kind == 'bulk' else x, split)
    for d in range(ndim):
        out[d] = ess_of_chains(c[:, :, d])
    return out


def mcse_mean(x, split=True):
    """The Monte-Carlo standard error of the posterior mean of every parameter of a chain ``(n, W, ndim)``, ``(ndim,)``:
    ``np.std(flat, ddof=1) / sqrt(ess(x, 'mean'))``."""
    x = _chain3(x)
    with np.errstate(all='ignore'):
        return np.std(x.reshape(-1, x.shape[2]), axis=0, ddof=1) / np.sqrt(ess(x, 'mean', split))


# -- on the device -------------------------------------------------------------------------------------------------------
def round_lags(n, n_ensembles, walkers_per_ensemble, ndim, split=True, n_threshold=0):
    """How many lags bisip_chain_ess_dev takes per round -- a function of the shape alone: round_lags of
    bisip_amd/csrc/chain_lags.h (whose tile constants the numbers below restate) on the ``L`` samples of a half and the
    ``ceil(columns / 64) * max(1, n_threshold) * splits`` tiles of every series set."""
    splits = 2 if split else 1
    L = int(n) // splits
    tiles = -(-(int(n_ensembles) * int(walkers_per_ensemble) * int(ndim)) // 64) * max(1, int(n_threshold)) * splits
    return 64 * max(1, min(-(-L // 64), -(-512 // tiles), 65535))


def device_rank_normalize(view, center=None):
    """``z_scale`` of every (ensemble, parameter) of a ChainView, taken where the chain lies
    (bisip_chain_rank_normalize_dev): the derived ChainView of a new tensor ``(n, n_ensembles * Wp, ndim)``.  The ensembles
    go in passes whose gathered columns stay under ``RANK_PASS_BYTES`` (one sort takes fewer than 2^31 values).
    ``center (n_ensembles, ndim)``: ``z_scale(abs(x - center))`` instead, folded where the values are read
    (bisip_chain_rank_normalize_folded_dev; bisip_amd.diagnostics)."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    if center is not None:
        center = np.ascontiguousarray(center, dtype=np.float64)
        if center.shape != (E, ndim):
            raise ValueError(f'center must have shape ({E}, {ndim}), got {center.shape}')
        center = view.upload(center)
    z = view.empty((n, E * Wp, ndim), torch.float64)
    G = int(min(E, max(1, RANK_PASS_BYTES // (n * Wp * ndim * 8))))
    if _hip.chain_rank_normalize_workspace(n, G, Wp, ndim) <= 0:
        raise ValueError('chain too large for one device sort (more than 2^31 values per ensemble); thin it or use '
                         'get_chain()')
    for g0 in range(0, E, G):
        k = min(E, g0 + G) - g0
        nbytes = _hip.chain_rank_normalize_workspace(n, k, Wp, ndim)
        work = view.empty((nbytes,), torch.uint8)
        part = z if k == E else view.empty((n, k * Wp, ndim), torch.float64)
        if center is None:
            _hip.chain_rank_normalize_dev(view.ptr + 8 * g0 * Wp * ndim, n, view.stride, k, Wp, ndim, part.data_ptr(),
                                          work.data_ptr(), nbytes, view.stream)
        else:
            _hip.chain_rank_normalize_folded_dev(view.ptr + 8 * g0 * Wp * ndim, n, view.stride, k, Wp, ndim,
                                                 center.data_ptr() + 8 * g0 * ndim, part.data_ptr(), work.data_ptr(), nbytes,
                                                 view.stream)
        if part is not z:                                        # (same stream: ordered after the kernel)
            z[:, g0 * Wp:(g0 + k) * Wp].copy_(part)
        view.synchronize()
        del work, part
    return view.derived(z)


def _ess_call(view, splits, thresholds=None):
    """One bisip_chain_ess_dev call: ``(E, ndim)``, or ``(len(thresholds), E, ndim)`` for thresholds ``(T, E, ndim)``."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    T = 0 if thresholds is None else int(thresholds.shape[0])
    nbytes = _hip.chain_ess_workspace(n, E, Wp, ndim, splits, T)
    if nbytes <= 0:
        raise ValueError(f'chain shape ({n}, {E} x {Wp}, {ndim}) not supported')
    work = view.empty((nbytes,), torch.uint8)
    thr = view.upload(thresholds) if T else None
    out = view.empty((max(T, 1), E, ndim), torch.float64)
    _hip.chain_ess_dev(view.ptr, n, view.stride, E, Wp, ndim, splits, thr.data_ptr() if T else 0, T, out.data_ptr(),
                       work.data_ptr(), nbytes, view.stream)
    view.synchronize()
    res = out.cpu().numpy()
    return res if T else res[0]


def device_ess(view, kind='bulk', split=True):
    """``ess`` of every ensemble of a ChainView, ``(n_ensembles, ndim)`` (NumPy), taken where the chain lies.  ``'mean'``:
    one bisip_chain_ess_dev call.  ``'bulk'``: device_rank_normalize, then that call on the ranks' z.  ``'tail'``:
    device_percentiles gives np.percentile's own doubles, so the indicators are the definition's; one thresholded call for
    both, then the smaller.  (The 0th and 100th percentile come with them: a value that is not finite shows there.)"""
    _check_kind(kind)
    splits = 2 if split else 1
    if view.n < 2 * splits:
        raise ValueError(f'a chain of {view.n // splits} sample(s) has no variance: the ESS needs 2 per chain, '
                         '4 used samples when split')
    if kind == 'mean':
        return _ess_call(view, splits)
    if kind == 'bulk':
        return _ess_call(device_rank_normalize(view), splits)
    from .chainview import device_percentiles
    q = device_percentiles(view, (0.0,) + TAIL_PERCENTILES + (100.0,))
    thr = np.where(np.isfinite(q[0]) & np.isfinite(q[3]), q[1:3], np.nan)
    with np.errstate(invalid='ignore'):
        return np.min(_ess_call(view, splits, thr), axis=0)       # (np.min: a NaN stays)


def device_mcse_mean(view, split=True):
    """``mcse_mean`` of every ensemble of a ChainView, ``(n_ensembles, ndim)``: the standard deviation of
    bisip_chain_moments_dev times ``sqrt(N / (N - 1))`` over the square root of the ``'mean'`` ESS."""
    from .chainview import device_moments
    N = view.n * view.walkers_per_ensemble
    with np.errstate(all='ignore'):
        return device_moments(view)[1] * np.sqrt(N / (N - 1.0)) / np.sqrt(device_ess(view, 'mean', split))


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelEss:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are those of get_rhat
    (``_trace_source``)."""

    def get_ess(self, kind='bulk', chain=None, split=True, **kwargs):
        """The effective sample size of every parameter, ``(ndim,)`` (bisip_amd.ess): ``kind='bulk'`` of the
        rank-normalised samples, ``'tail'`` the smaller of the 5 % and 95 % quantile indicators', ``'mean'`` of the values
        themselves -- Stan's and ArviZ's ``ess_bulk`` / ``ess_tail``.  The walkers, each cut into halves unless
        ``split=False``, are the chains; walkers of an ensemble sampler are not independent chains, so the between-walker
        term is a screening device.  ``chain``: an unflattened chain ``(n, nwalkers, ndim)``, else ``discard`` / ``thin`` as
        for ``get_chain``.  A fit with the device sampler is reduced on the GPU (``chain='device'``: where the chain lies),
        an explicit ``chain`` or a host sampler's in NumPy."""
        from .utils import discard_thin
        _check_kind(kind)
        where, src = self._trace_source(chain, kwargs)
        if where == 'device':
            return src.param_ess(kind, split=split, **discard_thin(kwargs))[0]
        return ess(src, kind, split)

    def get_mcse_mean(self, chain=None, **kwargs):
        """The Monte-Carlo standard error of the posterior mean of every parameter, ``(ndim,)``: the standard deviation
        (ddof = 1) of the flattened used samples over ``sqrt(get_ess('mean'))``.  Arguments as get_ess."""
        from .utils import discard_thin
        where, src = self._trace_source(chain, kwargs)
        if where == 'device':
            return src.param_mcse_mean(**discard_thin(kwargs))[0]
        return mcse_mean(src)

    def get_log_prob_ess(self, kind='bulk', split=True, **kwargs):
        """The effective sample size of the stored log-probability, a scalar.  ``discard`` / ``thin`` as for
        ``get_chain``."""
        from .utils import discard_thin
        _check_kind(kind)
        where, src = self._trace_source(None, kwargs)
        if where == 'device':
            return float(src.log_prob_ess(kind, split=split, **discard_thin(kwargs))[0])
        lp = np.asarray(self._sampler.get_log_prob(**discard_thin(kwargs)), dtype=np.float64)
        return float(ess(lp[:, :, None], kind, split)[0])


class BatchEss:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler)."""

    def get_ess(self, kind='bulk', discard=0, thin=1, split=True):
        """The effective sample size of every parameter of every spectrum, ``(E, ndim)`` -- per spectrum ``ess.ess`` of its
        walkers' series (bulk, tail or mean) -- taken on the device for ``chain='device'`` and ``'host'`` alike: which
        fits of a survey have too few effective samples for their intervals.  A screening number, as get_rhat: walkers of
        an ensemble are not independent chains.  A multi-GPU survey joins the ranks' blocks with ``gather``."""
        return self._fitted().param_ess(kind, discard=discard, thin=thin, split=split)

    def get_mcse_mean(self, discard=0, thin=1):
        """The Monte-Carlo standard error of every posterior mean, ``(E, ndim)``."""
        return self._fitted().param_mcse_mean(discard=discard, thin=thin)

    def get_log_prob_ess(self, kind='bulk', discard=0, thin=1, split=True):
        """The effective sample size of every spectrum's stored log-probability, ``(E,)``."""
        return self._fitted().log_prob_ess(kind, discard=discard, thin=thin, split=split)
