"""Rank-normalised folded R-hat, the Monte-Carlo error of the standard deviation and the posterior table.

``convergence.rhat`` is the R-hat of Gelman and Rubin (1992) on the raw values.  Vehtari, Gelman, Simpson, Carpenter and
Buerkner (2021), "Rank-normalization, folding, and localization: an improved R-hat" -- the paper bisip_amd.ess takes its
effective sample size from -- replace it, because it has two blind spots: walkers that agree in mean but differ in scale
pass it, and heavy tails (an infinite variance) hide a walker that is shifted.  Both happen here: a stuck walker in a
chargeability that piles up against its bound, a Cauchy-like ``log_tau`` of a mode the data barely constrain.

The definitions, for a chain ``x (n, W, ndim)``, per parameter over its ``N = n * W`` values:

* ``rank_rhat``: with ``med = np.percentile(values, 50)``, ``bulk = convergence.rhat(ess.z_scale(x), split)`` and ``folded
  = convergence.rhat(ess.z_scale(np.abs(x - med)), split)``, the larger of the two, taken so that a NaN stays.  The bulk
  part sees a shifted walker whatever the tails, the folded part a walker of another scale.  ``z_scale`` is this
  project's: every sample is ranked, the middle sample of an odd ``n`` (which belongs to neither half of
  ``convergence.split_chains``) included.  A value that is not finite gives NaN; a constant parameter the IEEE result of
  ``convergence.gelman_rubin``, NaN.
* ``ess_sd``: ``ess.ess_of_chains`` of the (split) chains of the series ``(x - m) * (x - m)``, ``m = np.mean(values)``
  (``center=`` replaces it): one subtraction and one multiplication per value.
* ``mcse_sd``: with ``c2 = (x - m) * (x - m)``, ``Evar = mean(c2)``, ``varvar = (mean(c2 * c2) - Evar**2) / ess_sd``,
  ``sqrt(varvar / Evar / 4)``: Kenney and Keeping's variance of a variance scaled by the effective sample size, first
  order for the standard deviation -- the centred-moment form of the R package ``posterior``.  The IEEE result stands:
  NaN for a constant parameter.
* ``summary``: the table ``az.summary`` / Stan's ``summary`` print -- ``mean``, ``sd`` (ddof = 1, the one ``mcse_mean``
  is taken of; NOT ``get_param_std``'s ddof = 0), ``hdi_lo``, ``hdi_hi`` (bisip_amd.interval), ``mcse_mean``, ``mcse_sd``,
  ``ess_bulk``, ``ess_tail``, ``r_hat`` (``rank_rhat``) -- and ``format_summary`` its fixed-width text.

The ``posterior`` form of ``mcse_sd`` and the ranking of the middle sample are this project's definitions: neither was
compared with ArviZ.  Walkers of an ensemble sampler are not independent chains: all of this screens, none of it proves.

* ``device_rank_rhat``, ``device_ess_sd``, ``device_mcse_sd``, ``device_summary`` take them on a ChainView where the chain
  lies (bisip_chain_rank_normalize_folded_dev, bisip_chain_ess_squares_dev, bisip_chain_central_moments_dev and the kernels
  of bisip_amd.ess, .convergence, .interval and .chainview).  The rank pass is the dear step, and the bulk R-hat needs the
  same ``z`` as the bulk effective sample size: ``device_summary`` makes one plain and one folded rank pass.
* ``ordered_central_moments`` restates the order of bisip_chain_central_moments_dev in NumPy: the same bits.
* ``ModelDiagnostics`` and ``BatchDiagnostics`` are the methods of the models (bisip_amd.utils.utils) and of
  SpectraBatch, as mixins.

A stored log-probability ``(n, W)`` is a chain of ``ndim = 1``.
"""

import numpy as np

from . import convergence as cv
from . import ess as es

__all__ = ('SUMMARY_KEYS', 'rank_rhat', 'ess_sd', 'mcse_sd', 'summary', 'format_summary', 'ordered_central_moments',
           'device_central_moments', 'device_rank_rhat', 'device_ess_sd', 'device_mcse_sd', 'device_summary',
           'ModelDiagnostics', 'BatchDiagnostics')

SUMMARY_KEYS = ('mean', 'sd', 'hdi_lo', 'hdi_hi', 'mcse_mean', 'mcse_sd', 'ess_bulk', 'ess_tail', 'r_hat')


def _chain3(x, what='the diagnostics need'):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError(f'{what} the unflattened chain (n, nwalkers, ndim), got shape {x.shape}')
    return x


def _device_view(x):
    """The ChainView of a float64 tensor ``(n, walkers, ndim)`` on the GPU (one ensemble), else None."""
    if not es._is_device_tensor(x):
        return None
    from .chainview import ChainView
    if x.dim() != 3:
        raise ValueError(f'the diagnostics need the unflattened chain (n, nwalkers, ndim), got shape {tuple(x.shape)}')
    return ChainView.of_tensor(x)


def _pick(parts_wanted, bulk, folded):
    with np.errstate(invalid='ignore'):
        both = np.maximum(bulk, folded)                          # (np.maximum: a NaN stays)
    return (both, bulk, folded) if parts_wanted else both


def rank_rhat(x, split=True, parts=False):
    """The rank-normalised folded (split) R-hat of every parameter of a chain ``(n, W, ndim)``, ``(ndim,)``: the larger of
    R-hat of the rank-normalised values and R-hat of the rank-normalised ``abs(x - median)`` (the module docstring holds
    the definition).  ``parts=True``: ``(rank_rhat, bulk, folded)``.  The shape rules are ``convergence.split_chains``'s.
    A float64 tensor on the GPU is reduced there (device_rank_rhat)."""
    view = _device_view(x)
    if view is not None:
        got = device_rank_rhat(view, split, parts)
        return tuple(g[0] for g in got) if parts else got[0]
    x = _chain3(x)
    cv.split_chains(x[:, :, :1], split)                          # (the shape is refused before any work)
    with np.errstate(all='ignore'):
        med = np.percentile(x.reshape(-1, x.shape[2]), 50, axis=0)
        bulk = cv.rhat(es.z_scale(x), split)
        folded = cv.rhat(es.z_scale(np.abs(x - med)), split)
    return _pick(parts, bulk, folded)


def _squares(x, center):
    """``((x - m) * (x - m), m)`` with ``m (ndim,)`` the mean of all values of every parameter, or ``center``."""
    if center is None:
        with np.errstate(all='ignore'):
            m = np.mean(x.reshape(-1, x.shape[2]), axis=0)
    else:
        m = np.asarray(center, dtype=np.float64)
        if m.shape != (x.shape[2],):
            raise ValueError(f'center must have shape ({x.shape[2]},), got {m.shape}')
    with np.errstate(all='ignore'):
        d = x - m
        return d * d, m


def ess_sd(x, split=True, center=None):
    """The effective sample size that the standard deviation is known with, ``(ndim,)``: ``ess.ess_of_chains`` of the
    (split) chains of ``(x - m) * (x - m)``, ``m`` the mean of all values of the parameter or ``center (ndim,)``.  A value
    that is not finite gives NaN.  A float64 tensor on the GPU is reduced there (device_ess_sd)."""
    view = _device_view(x)
    if view is not None:
        return device_ess_sd(view, split, None if center is None else np.reshape(center, (1, -1)))[0]
    x = _chain3(x)
    es._chains(x[:, :, :1], split)
    c = es._chains(_squares(x, center)[0], split)
    return np.array([es.ess_of_chains(c[:, :, d]) for d in range(x.shape[2])])


def mcse_sd(x, split=True):
    """The Monte-Carlo standard error of the posterior standard deviation of every parameter, ``(ndim,)``: with ``c2 = (x
    - m) * (x - m)`` over all values, ``sqrt((mean(c2 * c2) - mean(c2)**2) / ess_sd / mean(c2) / 4)`` (the module
    docstring).  NaN for a constant parameter.  A float64 tensor on the GPU is reduced there (device_mcse_sd)."""
    view = _device_view(x)
    if view is not None:
        return device_mcse_sd(view, split)[0]
    x = _chain3(x)
    n_eff = ess_sd(x, split)
    c2 = _squares(x, None)[0].reshape(-1, x.shape[2])
    with np.errstate(all='ignore'):
        Evar = np.mean(c2, axis=0)
        varvar = (np.mean(c2 * c2, axis=0) - Evar ** 2) / n_eff
        return np.sqrt(varvar / Evar / 4.0)


def summary(x, mass=0.95, split=True):
    """The posterior table of a chain ``(n, W, ndim)``: a dict of ``(ndim,)`` arrays with the keys ``SUMMARY_KEYS`` --
    ``mean``; ``sd``, the standard deviation with ddof = 1 that ``mcse_mean`` is taken of (not ``get_param_std``'s ddof =
    0); ``hdi_lo`` and ``hdi_hi``, the highest-density interval of ``mass`` (bisip_amd.interval.hdi); ``mcse_mean``
    (ess.mcse_mean) and ``mcse_sd``; ``ess_bulk`` and ``ess_tail`` (ess.ess); ``r_hat`` (rank_rhat).  A float64 tensor on
    the GPU is reduced there (device_summary)."""
    from .interval import hdi
    view = _device_view(x)
    if view is not None:
        return {k: v[0] for k, v in device_summary(view, mass, split).items()}
    x = _chain3(x)
    cv.split_chains(x[:, :, :1], split)
    flat = x.reshape(-1, x.shape[2])
    with np.errstate(all='ignore'):
        lo, hi = hdi(flat, mass)[:, 0, :]
        return dict(mean=np.mean(flat, axis=0), sd=np.std(flat, axis=0, ddof=1), hdi_lo=lo, hdi_hi=hi,
                    mcse_mean=es.mcse_mean(x, split), mcse_sd=mcse_sd(x, split), ess_bulk=es.ess(x, 'bulk', split),
                    ess_tail=es.ess(x, 'tail', split), r_hat=rank_rhat(x, split))


def format_summary(summary, names=None, digits=3, spectrum=None):
    """A summary as a fixed-width text table: one row per parameter, the columns in the order of ``SUMMARY_KEYS``, the
    numbers with ``digits`` significant digits (the effective sample sizes as whole numbers).  ``names``: the parameters'
    (default ``p0, p1, ...``).  A batch's summary ``(E, ndim)`` is printed one spectrum at a time: ``spectrum=``."""
    table = {k: np.asarray(summary[k], dtype=np.float64) for k in SUMMARY_KEYS}
    if table['mean'].ndim == 2:
        if spectrum is None:
            raise ValueError('a summary of several spectra is printed one at a time: pass spectrum=')
        table = {k: v[int(spectrum)] for k, v in table.items()}
    elif spectrum is not None:
        raise ValueError('spectrum= belongs to the summary of a batch')
    if any(v.ndim != 1 or v.shape != table['mean'].shape for v in table.values()):
        raise ValueError('every entry of a summary is one number per parameter')
    ndim = table['mean'].size
    names = [f'p{i}' for i in range(ndim)] if names is None else [str(s) for s in names]
    if len(names) != ndim:
        raise ValueError(f'{len(names)} names for {ndim} parameters')
    digits = int(digits)
    if digits < 1:
        raise ValueError('digits must be 1 or more')

    def cell(key, v):
        if np.isnan(v):
            return 'nan'
        if key.startswith('ess_') and np.isfinite(v):
            return f'{v:.0f}'
        return f'{v:.{digits}g}'

    cols = [['', *names]] + [[k, *(cell(k, v) for v in table[k])] for k in SUMMARY_KEYS]
    widths = [max(len(c) for c in col) for col in cols]
    lines = []
    for r in range(ndim + 1):
        row = [cols[0][r].ljust(widths[0])] + [col[r].rjust(w) for col, w in zip(cols[1:], widths[1:])]
        lines.append('  '.join(row).rstrip())
    return '\n'.join(lines)


# -- the device's order of summation ------------------------------------------------------------------------------------
def ordered_central_moments(x, center, n_ensembles=1):
    """``(m2, m4)``, ``(n_ensembles, ndim)`` each, of a chain ``(n, n_ensembles * Wp, ndim)`` about ``center (n_ensembles,
    ndim)`` with the bits bisip_chain_central_moments_dev produces: the sweep of chainview.ordered_moments' second pass
    (its splits, lanes, four accumulators, ascending combination), once per moment; per value ``d = x - c``, ``q = d * d``,
    ``acc2 = fma(d, d, acc2)``, ``acc4 = fma(q, q, acc4)`` taken exactly (``exact_fma``), so for the small shapes of the
    tests only."""
    from .chainview import _ensemble_rows, exact_fma, ordered_sweep
    v, n, E, Wp, ndim, lanes = _ensemble_rows(x, n_ensembles)
    center = np.asarray(center, dtype=np.float64)
    if center.shape != (E, ndim):
        raise ValueError(f'center must have shape ({E}, {ndim}), got {center.shape}')
    fma = np.frompyfunc(exact_fma, 3, 1)
    c = np.tile(center, (1, lanes // ndim))                      # lane t: parameter t % ndim

    def second(acc, values, k):
        d = values - c[:, :k]
        return fma(d, d, acc).astype(np.float64)

    def fourth(acc, values, k):
        d = values - c[:, :k]
        q = d * d
        return fma(q, q, acc).astype(np.float64)

    with np.errstate(all='ignore'):
        count = float(n) * float(Wp)
        return ordered_sweep(v, ndim, lanes, second) / count, ordered_sweep(v, ndim, lanes, fourth) / count


# -- on the device -------------------------------------------------------------------------------------------------------
def _splits(view, split, chains=True):
    splits = 2 if split else 1
    if view.n < 2 * splits:
        raise ValueError(f'a chain of {view.n // splits} sample(s) has no variance: the diagnostics need 2 per chain, '
                         '4 used samples when split')
    if chains and splits * view.walkers_per_ensemble < 2:
        raise ValueError('R-hat needs 2 chains or more')
    return splits


def _centers(view, center):
    c = np.ascontiguousarray(center, dtype=np.float64)
    if c.shape != (view.n_ensembles, view.ndim):
        raise ValueError(f'center must have shape ({view.n_ensembles}, {view.ndim}), got {c.shape}')
    return view.upload(c)


def device_central_moments(view, center):
    """The means of ``(x - c)**2`` and ``(x - c)**4`` over every ensemble's samples of a view about ``center (n_ensembles,
    ndim)``: ``(m2, m4)``, ``(n_ensembles, ndim)`` each (NumPy; bisip_chain_central_moments_dev)."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    c = _centers(view, center)
    m2, m4 = view.empty((E, ndim), torch.float64), view.empty((E, ndim), torch.float64)
    work = view.empty((max(1, _hip.chain_central_moments_workspace(n, E, ndim)),), torch.float64)
    _hip.chain_central_moments_dev(view.ptr, n, view.stride, E, Wp, ndim, c.data_ptr(), m2.data_ptr(), m4.data_ptr(),
                                   work.data_ptr(), view.stream)
    view.synchronize()
    return m2.cpu().numpy(), m4.cpu().numpy()


def _median(view):
    from .chainview import device_percentiles
    return device_percentiles(view, (50.0,))[0]


def _folded_rhat(view, split):
    """R-hat of the rank-normalised ``abs(x - median)``; the folded ``z`` is freed before the return."""
    z = es.device_rank_normalize(view, center=_median(view))
    return cv.device_rhat(z, split=split)


def device_rank_rhat(view, split=True, parts=False):
    """``rank_rhat`` of every ensemble of a ChainView, ``(n_ensembles, ndim)`` (NumPy), taken where the chain lies: one
    plain rank pass (bisip_chain_rank_normalize_dev) and bisip_chain_rhat_dev of its ``z``, then -- that ``z`` freed -- the
    medians (device_percentiles: NumPy's own doubles), one folded rank pass (bisip_chain_rank_normalize_folded_dev) and
    R-hat of its ``z``.  ``parts=True``: ``(rank_rhat, bulk, folded)``."""
    _splits(view, split)
    bulk = cv.device_rhat(es.device_rank_normalize(view), split=split)
    return _pick(parts, bulk, _folded_rhat(view, split))


def device_ess_sd(view, split=True, center=None):
    """``ess_sd`` of every ensemble of a ChainView, ``(n_ensembles, ndim)``: one bisip_chain_ess_squares_dev call about
    ``center (n_ensembles, ndim)``, by default device_moments' mean."""
    import torch
    from . import _hip
    from .chainview import device_moments
    splits = _splits(view, split, chains=False)
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    c = _centers(view, device_moments(view)[0] if center is None else center)
    nbytes = _hip.chain_ess_workspace(n, E, Wp, ndim, splits, 0)
    if nbytes <= 0:
        raise ValueError(f'chain shape ({n}, {E} x {Wp}, {ndim}) not supported')
    work = view.empty((nbytes,), torch.uint8)
    out = view.empty((E, ndim), torch.float64)
    _hip.chain_ess_squares_dev(view.ptr, n, view.stride, E, Wp, ndim, splits, c.data_ptr(), out.data_ptr(), work.data_ptr(),
                               nbytes, view.stream)
    view.synchronize()
    return out.cpu().numpy()


def _mcse_sd_about(view, split, mean):
    m2, m4 = device_central_moments(view, mean)
    with np.errstate(all='ignore'):
        return np.sqrt((m4 - m2 ** 2) / device_ess_sd(view, split, mean) / m2 / 4.0)


def device_mcse_sd(view, split=True):
    """``mcse_sd`` of every ensemble of a ChainView, ``(n_ensembles, ndim)``: the second and fourth moments
    (bisip_chain_central_moments_dev) and the effective sample size of the squares, all about device_moments' mean."""
    from .chainview import device_moments
    _splits(view, split, chains=False)
    return _mcse_sd_about(view, split, device_moments(view)[0])


def device_summary(view, mass=0.95, split=True):
    """``summary`` of every ensemble of a ChainView: a dict of ``(n_ensembles, ndim)`` arrays (NumPy).  Every entry comes
    from the entry point its own getter uses; the plain ``z`` is made once and gives both ``ess_bulk`` and the bulk part of
    ``r_hat``, and it is freed before the folded one is made: one plain and one folded rank pass per pass of ensembles, at
    most one chain-sized ``z`` alive."""
    from .chainview import device_moments
    from .interval import device_hdi
    splits = _splits(view, split)
    N = view.n * view.walkers_per_ensemble
    mean, std = device_moments(view)
    lo, hi = device_hdi(view, mass)
    with np.errstate(all='ignore'):
        sd = std * np.sqrt(N / (N - 1.0))
        mcse_mean = sd / np.sqrt(es._ess_call(view, splits))
    z = es.device_rank_normalize(view)
    ess_bulk = es._ess_call(z, splits)
    bulk = cv.device_rhat(z, split=split)
    del z
    r_hat = _pick(False, bulk, _folded_rhat(view, split))
    return dict(mean=mean, sd=sd, hdi_lo=lo, hdi_hi=hi, mcse_mean=mcse_mean, mcse_sd=_mcse_sd_about(view, split, mean),
                ess_bulk=ess_bulk, ess_tail=es.device_ess(view, 'tail', split), r_hat=r_hat)


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelDiagnostics:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are those of get_rhat and get_ess
    (``_trace_source``)."""

    def get_rank_rhat(self, chain=None, split=True, parts=False, **kwargs):
        """The rank-normalised folded R-hat of every parameter, ``(ndim,)`` (bisip_amd.diagnostics; Vehtari et al. 2021):
        the larger of R-hat of the rank-normalised samples and R-hat of the rank-normalised distances from the median.
        It sees what get_rhat passes -- walkers that agree in mean and differ in scale, a shifted walker under heavy tails
        -- and is what Stan and ArviZ report as ``r_hat``.  ``parts=True``: ``(rank_rhat, bulk, folded)``.  ``chain``: an
        unflattened chain ``(n, nwalkers, ndim)``, else ``discard`` / ``thin`` as for ``get_chain``.  A fit with the
        device sampler is reduced on the GPU (``chain='device'``: where the chain lies), an explicit ``chain`` or a host
        sampler's in NumPy."""
        from .utils import discard_thin
        where, src = self._trace_source(chain, kwargs)
        if where == 'device':
            got = src.param_rank_rhat(split=split, parts=parts, **discard_thin(kwargs))
            return tuple(g[0] for g in got) if parts else got[0]
        return rank_rhat(src, split, parts)

    def get_log_prob_rank_rhat(self, split=True, **kwargs):
        """The rank-normalised folded R-hat of the stored log-probability, a scalar.  ``discard`` / ``thin`` as for
        ``get_chain``."""
        from .utils import discard_thin
        where, src = self._trace_source(None, kwargs)
        if where == 'device':
            return float(src.log_prob_rank_rhat(split=split, **discard_thin(kwargs))[0])
        lp = np.asarray(self._sampler.get_log_prob(**discard_thin(kwargs)), dtype=np.float64)
        return float(rank_rhat(lp[:, :, None], split)[0])

    def get_ess_sd(self, chain=None, split=True, **kwargs):
        """The effective sample size that the posterior standard deviation is known with, ``(ndim,)``: get_ess('mean')
        of the squared distances from the posterior mean.  Arguments as get_rank_rhat."""
        from .utils import discard_thin
        where, src = self._trace_source(chain, kwargs)
        if where == 'device':
            return src.param_ess_sd(split=split, **discard_thin(kwargs))[0]
        return ess_sd(src, split)

    def get_mcse_sd(self, chain=None, split=True, **kwargs):
        """The Monte-Carlo standard error of the posterior standard deviation of every parameter, ``(ndim,)`` (the
        centred-moment form of the R package ``posterior``; bisip_amd.diagnostics).  Arguments as get_rank_rhat."""
        from .utils import discard_thin
        where, src = self._trace_source(chain, kwargs)
        if where == 'device':
            return src.param_mcse_sd(split=split, **discard_thin(kwargs))[0]
        return mcse_sd(src, split)

    def get_summary(self, mass=0.95, chain=None, split=True, **kwargs):
        """The posterior table in one call: a dict of ``(ndim,)`` arrays ``mean``, ``sd`` (ddof = 1, unlike
        get_param_std), ``hdi_lo``, ``hdi_hi`` (of ``mass``), ``mcse_mean``, ``mcse_sd``, ``ess_bulk``, ``ess_tail`` and
        ``r_hat`` (get_rank_rhat) -- what ``az.summary`` and Stan's ``summary`` print.  On the device the rank pass that
        ``ess_bulk`` and ``r_hat`` both need is made once.  Arguments as get_rank_rhat; the advice about ``discard`` is
        given once."""
        from .utils import discard_thin, warn_if_nothing_discarded
        where, src = self._trace_source(chain, kwargs)
        if chain is None:
            warn_if_nothing_discarded(kwargs)
        if where == 'device':
            return {k: v[0] for k, v in src.param_summary(mass, split=split, **discard_thin(kwargs)).items()}
        return summary(src, mass, split)

    def print_summary(self, mass=0.95, chain=None, split=True, digits=3, **kwargs):
        """Print get_summary as a table, one row per parameter under its name (format_summary)."""
        print(format_summary(self.get_summary(mass, chain, split, **kwargs), self.param_names, digits))


class BatchDiagnostics:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler): per spectrum what the models' methods give, taken on the
    device for ``chain='device'`` and ``'host'`` alike.  A multi-GPU survey joins the ranks' blocks with ``gather``."""

    def get_rank_rhat(self, discard=0, thin=1, split=True, parts=False):
        """The rank-normalised folded R-hat of every parameter of every spectrum, ``(E, ndim)`` (``parts=True``: with
        its bulk and its folded part): which fits of a survey to look at, where get_rhat is blind."""
        return self._fitted().param_rank_rhat(discard=discard, thin=thin, split=split, parts=parts)

    def get_log_prob_rank_rhat(self, discard=0, thin=1, split=True):
        """The rank-normalised folded R-hat of every spectrum's stored log-probability, ``(E,)``."""
        return self._fitted().log_prob_rank_rhat(discard=discard, thin=thin, split=split)

    def get_ess_sd(self, discard=0, thin=1, split=True):
        """The effective sample size of every posterior standard deviation, ``(E, ndim)``."""
        return self._fitted().param_ess_sd(discard=discard, thin=thin, split=split)

    def get_mcse_sd(self, discard=0, thin=1, split=True):
        """The Monte-Carlo standard error of every posterior standard deviation, ``(E, ndim)``."""
        return self._fitted().param_mcse_sd(discard=discard, thin=thin, split=split)

    def get_summary(self, mass=0.95, discard=0, thin=1, split=True):
        """The posterior table of every spectrum: a dict of ``(E, ndim)`` arrays with the keys of
        ``diagnostics.SUMMARY_KEYS``; one plain and one folded rank pass for all of them."""
        return self._fitted().param_summary(mass, discard=discard, thin=thin, split=split)

    def print_summary(self, spectrum=0, mass=0.95, discard=0, thin=1, split=True, digits=3):
        """Print one spectrum's rows of get_summary as a table (format_summary)."""
        print(format_summary(self.get_summary(mass, discard, thin, split), self.param_names, digits, spectrum=spectrum))
