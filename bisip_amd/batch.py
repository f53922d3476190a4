"""Batch of independent spectra (BASELINE config 5): E spectra x Wp walkers each.

The reference inverts one data file per ``Inversion`` object (src/bisip/models.py:41-57)
and a survey of many spectra is a Python loop over objects; here the E spectra share one
device context (``bisip_batch_create``) so one launch evaluates all E*Wp walkers and one
launch per half-step advances all E ensembles.  Ensembles are independent: across GPUs
they shard as whole replicas (spectra [start, stop) per rank, no collective).
"""

import numpy as np

from . import _hip, decomposition
from .autocorr import AutocorrError
from .covariance import BatchCovariance
from .diagnostics import BatchDiagnostics
from .ess import BatchEss
from .fitquality import BatchFitQuality
from .interval import BatchIntervals
from .dist import shard_range
from .loo import BatchLoo
from .mapfit import BatchMapFit
from .modes import BatchModes
from .predictive import BatchPredictive
from .evidence import BatchEvidence
from .response import BatchResponse
from .sampler import DeviceEnsembleSampler
from .summaries import device_model_percentiles
from .utils import first_if_scalar, load_data_batch

_MODELS = {
    'PolynomialDecomposition': _hip.MODEL_POLYDECOMP,
    'PeltonColeCole': _hip.MODEL_COLECOLE,
    'ColeCole': _hip.MODEL_COLECOLE,
    'Dias2000': _hip.MODEL_DIAS2000,
    'Shin2015': _hip.MODEL_SHIN2015,
}


def default_params(model, n_modes=1, poly_deg=5):
    """Parameter names and prior box of a model class (same as the reference's
    __init__ dictionaries, src/bisip/models.py:211-213, 247-252, 287-291, 325-331)."""
    if model == 'PolynomialDecomposition':
        p = {'r0': [0.9, 1.1]}
        p.update({f'a{x}': [-1, 1] for x in range(poly_deg + 1)})
    elif model in ('PeltonColeCole', 'ColeCole'):
        p = {'r0': [0.9, 1.1]}
        p.update({f'm{i+1}': [0.0, 1.0] for i in range(n_modes)})
        p.update({f'log_tau{i+1}': [-15, 5] for i in range(n_modes)})
        p.update({f'c{i+1}': [0.0, 1.0] for i in range(n_modes)})
    elif model == 'Dias2000':
        p = {'r0': [0.9, 1.1], 'm': [0, 1], 'log_tau': [-20, 0], 'eta': [0, 150], 'delta': [0, 1]}
    elif model == 'Shin2015':
        p = {'R1': [0.0, 1.0], 'R2': [0.0, 1.0], 'log_Q1': [-15, -13], 'log_Q2': [-7, -5],
             'n1': [0, 1], 'n2': [0, 1]}
    else:
        raise ValueError(f'unknown model {model!r}')
    return p


class SpectraBatch(BatchCovariance, BatchIntervals, BatchEss, BatchDiagnostics, BatchResponse, BatchFitQuality, BatchLoo,
                   BatchEvidence, BatchPredictive, decomposition.BatchRelaxation, BatchModes, BatchMapFit):
    """E spectra inverted together with the same model class.

    Args:
        model (str): 'PolynomialDecomposition', 'PeltonColeCole', 'Dias2000' or 'Shin2015'.
        spectra: list of file paths or of raw (N,5) tables [freq, amp, pha, amp_err, pha_err];
            all must have the same number of frequencies.
        nwalkers (int): walkers per spectrum (even). nsteps (int): MCMC steps.
        n_modes / poly_deg / c_exp: model options as in the reference classes.
        rank, world: keep only this rank's block of spectra (whole-replica sharding).
    """

    def __init__(self, model, spectra, nwalkers=256, nsteps=1000, headers=1, ph_units='mrad',
                 n_modes=1, poly_deg=5, c_exp=1.0, device=0, rank=0, world=1):
        if model not in _MODELS:
            raise ValueError(f'unknown model {model!r}')
        self.model = 'PeltonColeCole' if model == 'ColeCole' else model
        lo, hi = shard_range(len(spectra), world, rank)
        self.spectrum_range = (lo, hi)
        self.n_spectra_total = len(spectra)
        if hi <= lo:
            raise ValueError('no spectra for this rank')
        batch = load_data_batch(spectra[lo:hi], headers, ph_units)
        self.n_spectra = hi - lo
        self.N = batch['N']
        self.w, self.zn, self.zn_err = batch['w'], batch['zn'], batch['zn_err']
        self.norm_factor = batch['norm_factor']
        self.nwalkers, self.nsteps = int(nwalkers), int(nsteps)
        self.n_modes, self.poly_deg, self.c_exp = n_modes, poly_deg, c_exp
        self.params = default_params(self.model, n_modes, poly_deg)
        kw = {}
        if self.model == 'PolynomialDecomposition':
            # one tau grid for the whole batch, from the union of the frequency ranges
            # (identical to the reference's per-file grid when the spectra share w)
            period = np.log10(1. / self.w)
            self.log_tau = np.linspace(np.floor(period.min() - 1), np.floor(period.max() + 1), 2 * self.N)
            self.log_taus = np.array([self.log_tau ** i for i in range(poly_deg + 1)])
            self.taus = 10 ** self.log_tau
            kw = dict(poly_deg=poly_deg, c_exp=float(c_exp), taus=self.taus, log_taus=self.log_taus)
        elif self.model == 'PeltonColeCole':
            kw = dict(n_modes=n_modes)
        self.ctx = _hip.HipContext(_MODELS[self.model], self.w, self.zn, self.zn_err,
                                   self.param_bounds, device=device, **kw)
        self.ctx.set_spectrum_offset(lo)     # chains do not depend on how the survey is split over ranks
        self._sampler = None

    @property
    def param_names(self):
        return list(self.params.keys())

    @property
    def param_bounds(self):
        return np.array(list(self.params.values()), dtype=np.float64).T

    @property
    def ndim(self):
        return self.param_bounds.shape[1]

    def log_prob(self, theta):
        """theta (E, n, ndim) -> logp (E, n): n walkers of every spectrum in one launch."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[0] != self.n_spectra or theta.shape[2] != self.ndim:
            raise ValueError(f'theta must have shape ({self.n_spectra}, n, {self.ndim})')
        self.ctx.set_bounds(self.param_bounds)
        return self.ctx.logprob(theta.reshape(-1, self.ndim)).reshape(theta.shape[:2])

    def forward(self, theta):
        """theta (E, n, ndim) -> Z (E, n, 2, N)."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        Z = self.ctx.forward(theta.reshape(-1, self.ndim))
        return Z.reshape(theta.shape[0], theta.shape[1], 2, self.N)

    def fit(self, p0=None, seed=None, thin_by=1, chain='host', persistent=None, moves=None):
        """Run E independent stretch-move ensembles on the device (rng='philox').

        ``moves``: 'stretch', 'de' or 'snooker', a ``bisip_amd.moves`` descriptor, a list of them or of ``(move, weight)``
        (``[('de', 0.8), ('snooker', 0.2)]`` for spectra whose modes share a box): every ensemble runs the move drawn for
        the iteration, one launch per half-step (``persistent`` None or False).

        ``thin_by``: store one sample every ``thin_by`` iterations (``nsteps`` samples are
        stored).  ``chain='device'`` keeps the stored samples in HBM: ``get_param_mean`` /
        ``get_param_std`` then summarise them on the device and ``get_chain`` copies them to
        the host only when called.  ``persistent``: one workgroup per spectrum runs all
        iterations of a chunk in one launch (same chain; default: when the ensembles fit a
        workgroup and the batch fills the chip, see DeviceEnsembleSampler).  ``p0='map'``: ``fit_map()`` finds every
        spectrum's least-squares optimum first (32 starts each, one launch) and the walkers are drawn in a ball of its Laplace
        covariance around it (``mapfit.ball``).  The starts (a RandomState(0)) and one seed per spectrum for its ball (from the
        global NumPy RNG) are drawn for the whole survey and this rank's block kept, so a spectrum's chain does not depend on
        the number of ranks, as with ``p0=None``; ``get_map()`` returns the optima."""
        if chain not in ('host', 'device'):
            raise ValueError("chain must be 'host' or 'device'")
        E, Wp, ndim = self.n_spectra, self.nwalkers, self.ndim
        if isinstance(p0, str):
            # every spectrum's least-squares optimum first (fit_map), the walkers in a ball around it (mapfit.ball)
            if p0 != 'map':
                raise ValueError("p0 must be None, an array (n_spectra, nwalkers, ndim) or 'map'")
            p0 = self._map_walkers(np.random)
        if p0 is None:
            # the whole survey's starts from the global RNG, this rank's block kept: with the same
            # np.random.seed on every rank a spectrum starts (and runs) the same on any number of GPUs
            first, last = self.spectrum_range
            p0 = np.random.uniform(*self.param_bounds, (self.n_spectra_total, Wp, ndim))[first:last]
        self.ctx.set_bounds(self.param_bounds)
        self._sampler = DeviceEnsembleSampler(Wp, ndim, self.ctx, rng='philox', seed=seed,
                                              n_ensembles=E, chain_on_device=(chain == 'device'),
                                              persistent=persistent, moves=moves)
        self._sampler.run_mcmc(np.asarray(p0).reshape(E * Wp, ndim), self.nsteps, thin_by=thin_by)
        # PolynomialDecomposition: the reduced kernels were chosen from an estimate; measure them on
        # the final ensembles against long double (see Inversion._check_reduced_kernel)
        self.reduced_check_ = None
        if self.ctx.variant in ('reduced', 'reduced_comp'):
            self.reduced_check_ = self.ctx.reduced_check(self._sampler._coords, self._sampler._lp)
            if not self.reduced_check_ <= 1e-10:
                import warnings
                warnings.warn(f'the {self.ctx.variant!r} kernel is {self.reduced_check_:.1e} (relative) away from the '
                              'exact log-probability on the final ensembles (tolerance 1e-10)', RuntimeWarning)
        return self

    def _fitted(self):
        """The sampler of the fit."""
        if self._sampler is None:
            raise AssertionError('Model is not fitted!')
        return self._sampler

    def _moments(self, discard, thin):
        s = self._fitted()
        if s.chain_on_device:
            return s.param_moments(discard=discard, thin=thin)
        flat = self.get_chain(discard=discard, thin=thin, flat=True)   # (E, n, ndim)
        return flat.mean(axis=1), flat.std(axis=1)

    def get_param_mean(self, discard=0, thin=1):
        """Posterior mean of every parameter of every spectrum, ``(E, ndim)`` -- per spectrum
        what the reference's ``get_param_mean`` returns (src/bisip/utils.py:55-69)."""
        return self._moments(discard, thin)[0]

    def get_param_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles of every parameter of every spectrum, ``(len(p), E, ndim)`` -- per spectrum
        what the reference's ``get_param_percentile`` returns (src/bisip/utils.py:37-53)."""
        s = self._fitted()
        if s.chain_on_device:
            return s.param_percentiles(p, discard=discard, thin=thin)
        flat = self.get_chain(discard=discard, thin=thin, flat=True)   # (E, n, ndim)
        return np.percentile(flat, p, axis=1)

    def get_model_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles of the MODEL response over every spectrum's chain, ``(len(p), E, 2, N)`` -- per
        spectrum what the reference's ``get_model_percentile`` returns (src/bisip/utils.py:17-35): the
        band a fit is plotted with.  On the device, many spectra per pass: one forward launch that
        writes the responses column by column, one selection of the order statistics; with
        ``chain='device'`` the chain never leaves HBM."""
        out = device_model_percentiles(self._fitted().used_samples_dev(discard, thin), self.ctx, p)
        return out.reshape(-1, self.n_spectra, 2, self.N)

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False):
        """emcee's integrated autocorrelation time of every parameter of every spectrum, ``(E, ndim)``, in
        iterations of the stored chain (``thin`` times the estimate on ``get_chain(discard, thin)``), estimated on
        the device for ``chain='device'`` and ``'host'`` alike.  Raises AutocorrError when the chain is shorter
        than ``tol`` times an estimate (``quiet``: warns).  A multi-GPU survey joins the ranks' blocks with
        ``gather(get_autocorr_time(...))``."""
        try:
            tau = self._fitted().get_autocorr_time(discard=discard, thin=thin, c=c, tol=tol, quiet=quiet)
        except AutocorrError as err:
            raise AutocorrError(np.reshape(err.tau, (self.n_spectra, self.ndim)), *err.args) from None
        return np.reshape(tau, (self.n_spectra, self.ndim))

    def get_param_histogram(self, bins=25, range=None, discard=0, thin=1):
        """``np.histogram`` of every parameter of every spectrum, ``(counts (E, ndim, bins) int64, edges (E, ndim,
        bins + 1))`` -- per spectrum the counts of the reference's plot_histograms (src/bisip/plotlib.py:56-90) --
        counted on the device for ``chain='device'`` and ``'host'`` alike.  ``range``: None (each spectrum's own min
        and max), 'bounds' (the prior box: the same edges for every spectrum) or an array ``(ndim, 2)`` / ``(E, ndim,
        2)``."""
        return self._fitted().param_histograms(bins, range, discard=discard, thin=thin, bounds=self.param_bounds)

    def get_corner_histograms(self, bins=20, range=None, discard=0, thin=1):
        """``np.histogram2d`` of every pair of parameters of every spectrum, ``(counts (E, npairs, bins, bins) int64,
        edges (E, ndim, bins + 1), pairs)`` with ``pairs = np.triu_indices(ndim, 1)`` -- per spectrum the panels of
        the reference's plot_corner (src/bisip/plotlib.py:233-259)."""
        return self._fitted().pair_histograms(bins, range, discard=discard, thin=thin, bounds=self.param_bounds)

    def get_trace_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles over the WALKERS of every spectrum at every step, ``(len(p), n, E, ndim)`` (``(n, E, ndim)`` for a
        scalar ``p``) -- per spectrum the trace of the reference's plot_traces (src/bisip/plotlib.py:17-54) as numbers --
        taken on the device for ``chain='device'`` and ``'host'`` alike."""
        return first_if_scalar(p, self._fitted().trace_percentiles(p, discard=discard, thin=thin))

    def get_trace_mean(self, discard=0, thin=1):
        """The mean over the walkers of every spectrum at every step, ``(n, E, ndim)``."""
        return self._fitted().trace_mean(discard=discard, thin=thin)

    def get_log_prob_trace(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles over the walkers of every spectrum's stored log-probability at every step, ``(len(p), n, E)``
        (``(n, E)`` for a scalar ``p``): where burn-in shows first."""
        return first_if_scalar(p, self._fitted().log_prob_trace(p, discard=discard, thin=thin))

    def get_rhat(self, discard=0, thin=1, split=True):
        """The (split) Gelman-Rubin R-hat of every spectrum over its walkers, ``(E, ndim)`` (bisip_amd.convergence) --
        which fits of a survey to look at, beside the autocorrelation time -- taken on the device for ``chain='device'``
        and ``'host'`` alike."""
        return self._fitted().split_rhat(discard=discard, thin=thin, split=split)

    def get_walker_mean(self, discard=0, thin=1):
        """The mean of every walker's own series, ``(E, Wp, ndim)``: a stuck walker lies far from its ensemble's."""
        return self._fitted().walker_moments(discard=discard, thin=thin)[0]

    def get_walker_std(self, discard=0, thin=1):
        """The standard deviation (ddof = 1) of every walker's own series, ``(E, Wp, ndim)``."""
        return np.sqrt(self._fitted().walker_moments(discard=discard, thin=thin)[1])

    def get_log_prob_rhat(self, discard=0, thin=1, split=True):
        """R-hat of every spectrum's stored log-probability, ``(E,)``."""
        return self._fitted().log_prob_rhat(discard=discard, thin=thin, split=split)

    # -- PolynomialDecomposition: relaxation time distribution and integrating parameters ----------------------
    def _decomposition(self):
        if self.model != 'PolynomialDecomposition':
            raise ValueError(f'the RTD and its integrating parameters belong to PolynomialDecomposition, not {self.model}')

    def _decomposition_sampler(self):
        self._decomposition()
        return self._fitted()

    def rtd(self, theta):
        """The RTD ``m_l = sum_p a_p * log_tau_l**p`` of theta ``(E, n, ndim)`` on ``log_tau`` (host): ``(E, n, L)``."""
        self._decomposition()
        return decomposition.rtd(theta, self.log_tau)

    def integrating_params(self, theta):
        """``(m_total, log_tau_mean, m_norm)`` of theta ``(E, n, ndim)`` (host), each spectrum with its own
        ``norm_factor``: ``(E, n, 3)``."""
        self._decomposition()
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[0] != self.n_spectra:
            raise ValueError(f'theta must have shape ({self.n_spectra}, n, {self.ndim})')
        return decomposition.integrating_params(theta, self.log_tau, np.asarray(self.norm_factor)[:, None])

    def get_integrating_chain(self, discard=0, thin=1, flat=False):
        """``(m_total, log_tau_mean, m_norm)`` of every sample of every spectrum, computed on the GPU:
        ``(n', E, Wp, 3)`` as get_chain, ``(E, n' * Wp, 3)`` with ``flat``."""
        d = self._decomposition_sampler().integrating_chain_dev(self.log_tau, self.norm_factor, discard, thin)
        ch = d.cpu().numpy().reshape(-1, self.n_spectra, self.nwalkers, 3)
        if flat:
            ch = ch.transpose(1, 0, 2, 3).reshape(self.n_spectra, -1, 3)
        return ch

    def get_integrating_mean(self, discard=0, thin=1):
        """Posterior mean of ``(m_total, log_tau_mean, m_norm)`` per spectrum, ``(E, 3)``, on the device."""
        return self._decomposition_sampler().integrating_moments(self.log_tau, self.norm_factor, discard, thin)[0]

    def get_integrating_std(self, discard=0, thin=1):
        """Posterior standard deviation of ``(m_total, log_tau_mean, m_norm)`` per spectrum, ``(E, 3)``."""
        return self._decomposition_sampler().integrating_moments(self.log_tau, self.norm_factor, discard, thin)[1]

    def get_integrating_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles of ``(m_total, log_tau_mean, m_norm)`` per spectrum, ``(len(p), E, 3)`` (``(E, 3)`` for a
        scalar ``p``).  A multi-GPU survey joins the ranks with ``gather(np.moveaxis(pct, 1, 0))``."""
        out = self._decomposition_sampler().integrating_percentiles(p, self.log_tau, self.norm_factor, discard, thin)
        return first_if_scalar(p, out)

    def get_rtd_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles of the RTD ``m_l`` per spectrum, ``(len(p), E, L)`` (``(E, L)`` for a scalar ``p``): the m_l
        go column by column on the device, spectra in passes under ``decomposition.RTD_PASS_BYTES``."""
        return first_if_scalar(p, self._decomposition_sampler().rtd_percentiles(p, self.log_tau, discard, thin))

    def get_param_std(self, discard=0, thin=1):
        """Posterior standard deviation, ``(E, ndim)`` (src/bisip/utils.py:71-85)."""
        return self._moments(discard, thin)[1]

    def get_chain(self, discard=0, thin=1, flat=False):
        """(nsteps', E, Wp, ndim); flat=True -> (E, nsteps'*Wp, ndim)."""
        ch = self._fitted().get_chain(discard=discard, thin=thin)
        ch = ch.reshape(ch.shape[0], self.n_spectra, self.nwalkers, self.ndim)
        if flat:
            ch = ch.transpose(1, 0, 2, 3).reshape(self.n_spectra, -1, self.ndim)
        return ch

    def get_log_prob(self, discard=0, thin=1):
        lp = self._fitted().get_log_prob(discard=discard, thin=thin)
        return lp.reshape(lp.shape[0], self.n_spectra, self.nwalkers)

    @property
    def acceptance_fraction(self):
        return self._fitted().acceptance_fraction.reshape(self.n_spectra, self.nwalkers)

    def gather(self, per_spectrum, group=None):
        """The end of a multi-GPU survey: every rank passes a per-spectrum result of ITS block --
        ``(n_spectra, ...)``, e.g. ``get_param_mean()`` -- and gets the whole survey's
        ``(n_spectra_total, ...)`` in spectrum order.  The only collective of the batch path (the
        ensembles never exchange anything while they run); a single process gets its input back.
        A leading percentile axis is the caller's to move: ``gather(np.moveaxis(pct, 1, 0))``."""
        from .dist import all_gather_rows
        a = np.ascontiguousarray(per_spectrum, dtype=np.float64)
        if a.ndim < 1 or a.shape[0] != self.n_spectra:
            raise ValueError(f'expected {self.n_spectra} rows (one per spectrum of this rank), got {a.shape}')
        flat = all_gather_rows(a.reshape(self.n_spectra, -1), self.n_spectra_total, group)
        return flat.reshape((flat.shape[0],) + a.shape[1:])

    def close(self):
        """Release the device context."""
        self.ctx.close()
