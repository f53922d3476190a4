"""Posterior summaries of a chain that a device sampler has stored.

``DeviceChainSummaries`` is the part of ``DeviceEnsembleSampler`` that has nothing to do with sampling: it finds the
used samples of the stored chain (or log-probability) on the device as a ChainView and hands that to the ``device_*``
function of the family asked for (bisip_amd.chainview, .autocorr, .histogram, .trace, .convergence, .covariance,
.interval, .ess, .diagnostics, .decomposition, .response).
``device_model_percentiles`` also needs the model: forward over the samples, then the order statistics of each response.
"""

import numpy as np

from . import _hip, decomposition
from . import histogram as hg
from .autocorr import check_c, check_tol, device_integrated_time
from .chainview import ChainView, _merge_device_parts, device_moments, device_percentiles, used_range
from .convergence import device_rhat
from .covariance import corr_from_cov, device_best_sample, device_cov
from .diagnostics import device_ess_sd, device_mcse_sd, device_rank_rhat, device_summary
from .ess import device_ess, device_mcse_mean
from .fitquality import device_fit_quality
from .interval import device_hdi
from .predictive import device_predictive_check
from .response import device_model_moments
from .trace import device_trace

__all__ = ('DeviceChainSummaries', 'device_model_percentiles')


def device_model_percentiles(view, ctx, p, kind='ri'):
    """``np.percentile`` of the model response of ``ctx`` (a HipContext of ``view.n_ensembles`` spectra) over every
    ensemble's samples of a ChainView: ``(len(p), n_ensembles, 2 * N)`` (NumPy).  Spectra go in passes whose responses
    stay under ``decomposition.RTD_PASS_BYTES``: one forward launch that writes them column by column, one selection of
    the order statistics from each column.  ``kind='pa'``: the columns hold every sample's amplitude and minus phase
    (bisip_amd.response.response_pa) instead of Re and Im; everything else is the same."""
    import torch
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    rows_per, cols = n * Wp, 2 * ctx.N
    G = int(min(E, max(1, decomposition.RTD_PASS_BYTES // (rows_per * cols * 8))))
    out = np.empty((p.size, E, cols))
    grid = view.samples().reshape(n, E, Wp, ndim)
    for g0 in range(0, E, G):
        k = min(E, g0 + G) - g0
        rows = grid[:, g0:g0 + k].permute(1, 0, 2, 3).reshape(k, rows_per, ndim)    # one copy: spectrum-major
        Zc = view.empty((k, cols, rows_per), torch.float64)                       # one column per (spectrum, part, frequency)
        if kind == 'ri':
            ctx.forward_columns_dev(g0, k, rows.data_ptr(), k * rows_per, Zc.data_ptr(), view.stream)
        else:
            ctx.forward_columns_kind_dev(g0, k, rows.data_ptr(), k * rows_per, Zc.data_ptr(), kind, view.stream)
        res = view.empty((p.size, k * cols), torch.float64)
        _hip.columns_percentiles_dev(Zc.data_ptr(), k * cols, rows_per, p, res.data_ptr(), view.stream)
        view.synchronize()
        out[:, g0:g0 + k] = res.cpu().numpy().reshape(p.size, k, cols)
        del rows, Zc, res
    return out


class DeviceChainSummaries:
    """Mixin: the summaries of the chain its host class has stored, taken on the device.

    The host class (DeviceEnsembleSampler) provides ``_chain_parts`` and ``_log_prob_parts`` (the stored samples, one
    part per run: device slabs or host arrays), ``get_chain`` and ``get_log_prob`` (their host form), ``iteration`` (how
    many are stored), ``n_ensembles``, ``walkers_per_ensemble``, ``nwalkers`` and ``ndim`` (their layout), ``backend``
    (a HipStretchBackend: device, stream, allocator and the model's context) and ``chain_on_device``."""

    def _resident(self, parts):
        """Stored parts that lie on the device as ONE tensor (merged where they lie), else AttributeError."""
        if _merge_device_parts(parts):
            return parts[0].tensor()
        raise AttributeError('the chain is not resident on the device (run with chain_on_device=True)')

    def _stored_view(self, parts, ndim, host_get, discard, thin, upload):
        """The ChainView of the used samples of a stored quantity of ``ndim`` values per walker: the device tensor of
        ``parts`` itself, strided, or with ``upload`` a copy of ``host_get(discard, thin)`` sent up."""
        E, Wp, row = self.n_ensembles, self.walkers_per_ensemble, self.nwalkers * ndim
        if not upload:
            t = self._resident(parts)
            first, n = used_range(t.shape[0], discard, thin)
            return ChainView(t, n, E, Wp, ndim, first * row, int(thin) * row, self.backend)
        import torch
        _, n = used_range(self.iteration, discard, thin)
        used = torch.from_numpy(np.ascontiguousarray(host_get(discard=int(discard), thin=int(thin))))
        return ChainView(used.to(self.backend.device), n, E, Wp, ndim, backend=self.backend)

    def device_chain(self):
        """All stored samples as ONE torch tensor (iteration, W, ndim) on the device
        (``chain_on_device=True`` runs only)."""
        return self._resident(self._chain_parts)

    def used_samples_dev(self, discard=0, thin=1, upload=True):
        """``get_chain(discard, thin)`` on the device as a ChainView (bisip_amd.chainview): the stored chain itself
        with ``chain_on_device``, else an upload of the used samples only -- or, with ``upload=False``,
        device_chain()'s AttributeError."""
        return self._stored_view(self._chain_parts, self.ndim, self.get_chain, discard, thin,
                                 upload and not self.chain_on_device)

    def param_moments(self, discard=0, thin=1):
        """Mean and standard deviation of every parameter over the used samples, flattened over the walkers of each
        ensemble -- ``np.mean`` / ``np.std`` of ``get_chain(discard, thin, flat=True)`` (reference:
        src/bisip/utils.py:55-85) -- computed on the device, only the two
        ``(n_ensembles, ndim)`` results come back.  Returns ``(mean, std)``."""
        return device_moments(self.used_samples_dev(discard, thin, upload=False))

    def param_percentiles(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """``np.percentile(get_chain(discard, thin, flat=True), p, axis=0)`` per ensemble
        (reference: src/bisip/utils.py:37-53), sorted and interpolated on the device; returns
        ``(len(p), n_ensembles, ndim)``."""
        return device_percentiles(self.used_samples_dev(discard, thin, upload=False), p)

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False):
        """emcee's integrated autocorrelation time of ``get_chain(discard, thin)``, times ``thin``, every
        (ensemble, parameter) estimated on the device (bisip_chain_autocorr_time_dev): from the chain where it
        lies (``chain_on_device``), else from an upload of the used samples only.  ``(ndim,)`` for one ensemble,
        ``(n_ensembles, ndim)`` for a batch.  The ``tol`` test is that of integrated_time, per ensemble (every
        ensemble has the same number of samples); the AutocorrError carries every estimate."""
        c = check_c(c)
        view = self.used_samples_dev(discard, thin)
        tau, _ = device_integrated_time(view, c)
        E = self.n_ensembles
        what = 'parameter(s)' if E == 1 else f'(ensemble, parameter) pair(s) of {E} ensembles'
        return int(thin) * check_tol(tau if E > 1 else tau[0], view.n, tol, quiet, what)

    def param_range(self, discard=0, thin=1):
        """Min and max of the finite values of every parameter over ``get_chain(discard, thin)`` per ensemble,
        ``(n_ensembles, ndim, 2)``, and how many of its values are not finite, ``(n_ensembles, ndim)``, taken on the
        device (bisip_chain_range_dev)."""
        return hg.device_param_range(self.used_samples_dev(discard, thin))

    def _histogram_edges(self, bins, range, discard, thin, bounds):
        """The used samples on the device (a ChainView) and the edges ``(n_ensembles, ndim, bins + 1)`` of a
        ``range`` argument (None, 'bounds' or an array: bisip_amd.histogram)."""
        bins = hg.check_bins(bins)
        view = self.used_samples_dev(discard, thin)
        r = hg.resolve_range(range, view.n_ensembles, view.ndim, bounds, lambda: hg.device_param_range(view))
        return view, hg.edges_from_range(r, bins)

    def param_histograms(self, bins=25, range=None, discard=0, thin=1, bounds=None):
        """``np.histogram`` of every parameter of every ensemble over ``get_chain(discard, thin, flat=True)`` -- the
        counts of the reference's plot_histograms (src/bisip/plotlib.py:56-90) -- counted on the device
        (bisip_chain_histograms_dev): from the chain where it lies (``chain_on_device``), else from an upload of the
        used samples only.  ``range``: None (min and max of the samples), 'bounds' (the prior box ``bounds (2, ndim)``)
        or an array ``(ndim, 2)`` / ``(n_ensembles, ndim, 2)``.  Returns ``(counts (n_ensembles, ndim, bins) int64, edges
        (n_ensembles, ndim, bins + 1))``."""
        view, edges = self._histogram_edges(bins, range, discard, thin, bounds)
        return hg.device_histograms(view, edges), edges

    def pair_histograms(self, bins=20, range=None, discard=0, thin=1, bounds=None):
        """``np.histogram2d`` of every pair of parameters of every ensemble -- the panels of the reference's
        plot_corner (src/bisip/plotlib.py:233-259) -- counted on the device (bisip_chain_pair_histograms_dev).
        Returns ``(counts (n_ensembles, npairs, bins, bins) int64, edges (n_ensembles, ndim, bins + 1), pairs)``,
        ``pairs = np.triu_indices(ndim, 1)``; ``counts[e, q, a, b]``: parameter ``pairs[0][q]`` in bin ``a``,
        ``pairs[1][q]`` in bin ``b``."""
        view, edges = self._histogram_edges(bins, range, discard, thin, bounds)
        return hg.device_pair_histograms(view, edges), edges, hg.pair_index(self.ndim)

    def trace_percentiles(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """``np.percentile`` over the WALKERS of every ensemble at every sample of ``get_chain(discard, thin)`` -- the
        trace of the reference's plot_traces (src/bisip/plotlib.py:17-54) as statistics per step -- taken on the device
        (bisip_chain_trace_dev): from the chain where it lies (``chain_on_device``), else from an upload of the used
        samples only.  Returns ``(len(p), n, n_ensembles, ndim)``."""
        return device_trace(self.used_samples_dev(discard, thin), p, mean=False)[0]

    def trace_mean(self, discard=0, thin=1):
        """The mean over the walkers of every ensemble at every sample of ``get_chain(discard, thin)``, ``(n,
        n_ensembles, ndim)``, on the device."""
        return device_trace(self.used_samples_dev(discard, thin), ())[1]

    def log_prob_samples_dev(self, discard=0, thin=1):
        """``get_log_prob(discard, thin)`` on the device as a ChainView of ``ndim = 1``: the stored log-probabilities
        themselves with ``chain_on_device``, else an upload of the used ones."""
        parts = self._log_prob_parts
        return self._stored_view(parts, 1, self.get_log_prob, discard, thin, not _merge_device_parts(parts))

    def log_prob_trace(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """``np.percentile`` over the walkers of every ensemble of ``get_log_prob(discard, thin)``, where burn-in shows
        first: ``(len(p), n, n_ensembles)``, on the device."""
        return device_trace(self.log_prob_samples_dev(discard, thin), p, mean=False)[0][..., 0]

    def split_rhat(self, discard=0, thin=1, split=True):
        """The Gelman-Rubin R-hat of every ensemble over its walkers' series of ``get_chain(discard, thin)``, each cut
        into halves unless ``split=False`` (bisip_amd.convergence): ``(n_ensembles, ndim)``, taken on the device
        (bisip_chain_rhat_dev) from the chain where it lies (``chain_on_device``), else from an upload of the used samples
        only.  A screening number beside the autocorrelation time: walkers of an ensemble are not independent chains."""
        return device_rhat(self.used_samples_dev(discard, thin), split=split)

    def walker_moments(self, discard=0, thin=1):
        """``(mean, var)`` of every walker's own series of ``get_chain(discard, thin)``, ``(n_ensembles,
        walkers_per_ensemble, ndim)`` each, the variance with ddof = 1, on the device: a stuck walker is one whose mean
        lies far from its ensemble's."""
        _, mean, var = device_rhat(self.used_samples_dev(discard, thin), split=False, moments=True)
        return mean[0], var[0]

    def log_prob_rhat(self, discard=0, thin=1, split=True):
        """R-hat of every ensemble's stored log-probability, ``(n_ensembles,)``, on the device."""
        return device_rhat(self.log_prob_samples_dev(discard, thin), split=split)[:, 0]

    def param_ess(self, kind='bulk', discard=0, thin=1, split=True):
        """The effective sample size (``kind``: 'bulk', 'tail' or 'mean'; bisip_amd.ess) of every parameter of every
        ensemble over its walkers' series of ``get_chain(discard, thin)``, each cut into halves unless ``split=False``:
        ``(n_ensembles, ndim)``, taken on the device (bisip_chain_ess_dev, bisip_chain_rank_normalize_dev) from the chain
        where it lies (``chain_on_device``), else from an upload of the used samples only.  Walkers of an ensemble are not
        independent chains: the between-walker term is a screening device."""
        return device_ess(self.used_samples_dev(discard, thin), kind, split)

    def log_prob_ess(self, kind='bulk', discard=0, thin=1, split=True):
        """The effective sample size of every ensemble's stored log-probability, ``(n_ensembles,)``, on the device."""
        return device_ess(self.log_prob_samples_dev(discard, thin), kind, split)[:, 0]

    def param_mcse_mean(self, discard=0, thin=1):
        """The Monte-Carlo standard error of every posterior mean, ``(n_ensembles, ndim)``: param_moments' standard
        deviation times ``sqrt(N / (N - 1))`` over the square root of the 'mean' effective sample size."""
        return device_mcse_mean(self.used_samples_dev(discard, thin))

    def param_rank_rhat(self, discard=0, thin=1, split=True, parts=False):
        """The rank-normalised folded R-hat (bisip_amd.diagnostics.rank_rhat) of every parameter of every ensemble over
        its walkers' series of ``get_chain(discard, thin)``: ``(n_ensembles, ndim)``, with ``parts=True`` ``(rank_rhat,
        bulk, folded)``, taken on the device (bisip_chain_rank_normalize_dev and ..._folded_dev, bisip_chain_rhat_dev)
        from the chain where it lies (``chain_on_device``), else from an upload of the used samples only."""
        return device_rank_rhat(self.used_samples_dev(discard, thin), split, parts)

    def log_prob_rank_rhat(self, discard=0, thin=1, split=True):
        """The rank-normalised folded R-hat of every ensemble's stored log-probability, ``(n_ensembles,)``."""
        return device_rank_rhat(self.log_prob_samples_dev(discard, thin), split)[:, 0]

    def param_ess_sd(self, discard=0, thin=1, split=True):
        """The effective sample size of the squared distances from the posterior mean (diagnostics.ess_sd), ``(n_ensembles,
        ndim)``: bisip_chain_ess_squares_dev about param_moments' mean."""
        return device_ess_sd(self.used_samples_dev(discard, thin), split)

    def param_mcse_sd(self, discard=0, thin=1, split=True):
        """The Monte-Carlo standard error of every posterior standard deviation (diagnostics.mcse_sd), ``(n_ensembles,
        ndim)``: bisip_chain_central_moments_dev and param_ess_sd."""
        return device_mcse_sd(self.used_samples_dev(discard, thin), split)

    def param_summary(self, mass=0.95, discard=0, thin=1, split=True):
        """The posterior table (diagnostics.summary) of every ensemble: a dict of ``(n_ensembles, ndim)`` arrays ``mean``,
        ``sd`` (ddof = 1), ``hdi_lo``, ``hdi_hi``, ``mcse_mean``, ``mcse_sd``, ``ess_bulk``, ``ess_tail``, ``r_hat``, with
        one plain and one folded rank pass for all of them."""
        return device_summary(self.used_samples_dev(discard, thin), mass, split)

    def param_cov(self, discard=0, thin=1):
        """``np.cov`` (ddof = 1) of every ensemble's used samples flattened over its walkers -- of ``get_chain(discard,
        thin, flat=True)`` restricted to the ensemble -- ``(n_ensembles, ndim, ndim)``, taken on the device
        (bisip_chain_cov_dev) from the chain where it lies (``chain_on_device``), else from an upload of the used samples
        only."""
        return device_cov(self.used_samples_dev(discard, thin))

    def evidence(self, discard=0, thin=1, **kwargs):
        """The bridge-sampling estimate of every ensemble's log marginal likelihood (bisip_amd.evidence.device_evidence, whose
        keywords ``kwargs`` are): the first half of ``get_chain(discard, thin)`` fits a normal proposal, the second half with
        its stored log-probability and draws of the proposal enter the estimator, all on the device (bisip_bridge_*_dev,
        bisip_logprob_dev) from the chain where it lies (``chain_on_device``), else from an upload of the used samples only.
        A dict of ``(n_ensembles,)`` arrays ``log_ml``, ``se``, ``iterations``, ..."""
        from .evidence import device_evidence
        return device_evidence(self.used_samples_dev(discard, thin), self.log_prob_samples_dev(discard, thin),
                               self.backend.ctx, **kwargs)

    def param_corr(self, discard=0, thin=1):
        """``np.corrcoef`` of the same samples, ``(n_ensembles, ndim, ndim)``: the device's covariance divided on the host
        (covariance.corr_from_cov); NaN where a parameter does not vary."""
        return corr_from_cov(self.param_cov(discard, thin))

    def best_sample(self, discard=0, thin=1):
        """The stored sample of largest log-probability among the used ones of every ensemble: ``(theta (n_ensembles,
        ndim), logp (n_ensembles,), index (n_ensembles,))``, ``index = k * walkers_per_ensemble + w`` in used-sample
        numbering, found on the device (bisip_chain_best_sample_dev)."""
        return device_best_sample(self.used_samples_dev(discard, thin), self.log_prob_samples_dev(discard, thin))

    def param_hdi(self, mass=0.95, discard=0, thin=1):
        """The highest-density interval of every parameter of every ensemble over ``get_chain(discard, thin,
        flat=True)`` restricted to the ensemble (bisip_amd.interval.hdi): ``(2, n_ensembles, ndim)``, or ``(len(mass), 2,
        n_ensembles, ndim)`` for a sequence of masses, taken on the device (bisip_chain_hdi_dev) from the chain where it
        lies (``chain_on_device``), else from an upload of the used samples only."""
        return device_hdi(self.used_samples_dev(discard, thin), mass)

    def _integrating_view(self, log_tau, norm_factor, discard, thin):
        view = self.used_samples_dev(discard, thin)
        return view.derived(decomposition.device_integrating_chain(view, log_tau, norm_factor))

    def integrating_chain_dev(self, log_tau, norm_factor, discard=0, thin=1):
        """PolynomialDecomposition's ``(m_total, log_tau_mean, m_norm)`` of every sample of ``get_chain(discard,
        thin)`` (bisip_rtd_integrals_dev; bisip_amd.decomposition): a device tensor ``(n, nwalkers, 3)``.
        ``norm_factor``: scalar or one per ensemble."""
        return self._integrating_view(log_tau, norm_factor, discard, thin).tensor

    def integrating_moments(self, log_tau, norm_factor, discard=0, thin=1):
        """Mean and std of the integrating parameters per ensemble, ``(n_ensembles, 3)`` each, on the device."""
        return device_moments(self._integrating_view(log_tau, norm_factor, discard, thin))

    def integrating_percentiles(self, p, log_tau, norm_factor, discard=0, thin=1):
        """np.percentile of the integrating parameters per ensemble, ``(len(p), n_ensembles, 3)``, on the device."""
        return device_percentiles(self._integrating_view(log_tau, norm_factor, discard, thin), p)

    def integrating_hdi(self, mass, log_tau, norm_factor, discard=0, thin=1):
        """The highest-density interval of the integrating parameters per ensemble, ``(2, n_ensembles, 3)`` (``(len(mass),
        2, n_ensembles, 3)`` for a sequence of masses), on the device."""
        return device_hdi(self._integrating_view(log_tau, norm_factor, discard, thin), mass)

    def rtd_percentiles(self, p, log_tau, discard=0, thin=1):
        """np.percentile of the RTD ``m_l`` per ensemble, ``(len(p), n_ensembles, L)``, on the device
        (bisip_rtd_columns_dev, then the selection of bisip_columns_percentiles_dev)."""
        return decomposition.device_rtd_percentiles(self.used_samples_dev(discard, thin), p, log_tau)

    def model_percentiles(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """``np.percentile(forward(get_chain(discard, thin, flat=True)), p, axis=0)`` -- the
        reference's get_model_percentile (src/bisip/utils.py:17-35) -- without the chain leaving
        the device: batched forward over the stored samples, written column by column, then the
        selection of the order statistics from each column.  One ensemble only (NotImplementedError
        otherwise); returns ``(len(p), 2, N)``."""
        if self.n_ensembles != 1:
            raise NotImplementedError('model percentiles of a batch of spectra: one spectrum at a time')
        ctx = self.backend.ctx
        return device_model_percentiles(self.used_samples_dev(discard, thin, upload=False), ctx, p).reshape(-1, 2, ctx.N)

    def model_percentiles_pa(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """``np.percentile(response_pa(forward(get_chain(discard, thin, flat=True))), p, axis=0)``: the percentiles of
        every sample's amplitude and minus phase (bisip_amd.response), as model_percentiles -- the forward kernel writes
        amplitude / phase columns, the same selection reads them.  One ensemble only (NotImplementedError otherwise);
        returns ``(len(p), 2, N)``."""
        if self.n_ensembles != 1:
            raise NotImplementedError('model percentiles of a batch of spectra: one spectrum at a time')
        ctx = self.backend.ctx
        out = device_model_percentiles(self.used_samples_dev(discard, thin, upload=False), ctx, p, 'pa')
        return out.reshape(-1, 2, ctx.N)

    def model_moments(self, kind='ri', discard=0, thin=1):
        """``(mean, std)`` of the model response over every ensemble's used samples, ``(n_ensembles, 2, N)`` each, in the
        representation ``kind`` ('ri': Re and Im; 'pa': amplitude and minus phase): ``np.mean`` / ``np.std`` (ddof = 0)
        of ``forward(get_chain(discard, thin, flat=True))`` per ensemble, evaluated and summed in one pass over the chain
        where it lies (bisip_response_moments_dev; ``chain_on_device``), else over an upload of the used samples only.
        No response is stored."""
        return device_model_moments(self.used_samples_dev(discard, thin), self.backend.ctx, kind)

    def fit_quality(self, discard=0, thin=1):
        """``(mean_q, var_q, lmeh)`` per data point of every ensemble's spectrum, ``(n_ensembles, 2, N)`` each, over the
        used samples: with ``q = (zn - forward(get_chain(discard, thin, flat=True)))**2 / zn_err**2`` the mean of ``q``,
        its variance (ddof = 1) and ``log(mean(exp(-q / 2)))`` (bisip_amd.fitquality.fit_sums), evaluated and summed in
        one pass over the chain where it lies (bisip_fit_quality_dev; ``chain_on_device``), else over an upload of the
        used samples only.  No response is stored."""
        return device_fit_quality(self.used_samples_dev(discard, thin), self.backend.ctx)

    def predictive_check(self, discard=0, thin=1):
        """``(pit, row, sign_changes)`` of every ensemble's spectrum over the used samples: ``pit (n_ensembles, 2, N)`` the
        posterior predictive probability ``P(y_rep <= y | y)`` of every data point, ``row (n_ensembles, 3)`` the means of
        the chi-square ``T``, of ``P(chi2_2N >= T)`` and of the probability of the largest standardised residual, and
        ``sign_changes (n_ensembles, 2N - 1)`` the histogram of the residual's sign changes along the frequency axis
        (bisip_amd.predictive.predictive_sums), evaluated and summed over the chain where it lies
        (bisip_predictive_check_dev; ``chain_on_device``), else over an upload of the used samples only.  No response is
        stored."""
        return device_predictive_check(self.used_samples_dev(discard, thin), self.backend.ctx)
