"""The model response over the posterior in the units of the measurement: amplitude and phase.

SIP spectra are measured and plotted as amplitude and phase; ``forward`` and ``get_model_percentile`` give the response
in the likelihood's coordinates, Re Z and Im Z.  A phase band cannot be derived from the Re / Im bands -- the two parts
are strongly correlated over the posterior, and ``arctan2`` of two percentile curves is not a percentile of anything -- so
the amplitude and phase of EVERY sample's response are taken first, where the chain lies, and reduced there.  The posterior
mean response and its standard deviation are reduced the same way, without the responses ever being written to memory.

* ``response_pa``, ``represent``, ``model_percentile_pa``, ``response_moments``: the definitions, plain NumPy in float64;
* ``device_model_moments`` runs ``bisip_response_moments_dev`` on a ChainView (bisip_amd.chainview) where the chain
  lies; the amplitude / phase percentiles are ``summaries.device_model_percentiles(..., kind='pa')``: the forward kernel
  writes amplitude / phase columns, the selection kernel reads them as it reads Re / Im ones;
* ``ordered_response_moments`` restates the order of every sum of the moments kernel (include/bisip_hip.h) in NumPy: the
  same bits from the same responses; ``plan`` is the kernel's shape-only plan;
* ``ModelResponse`` and ``BatchResponse`` are the ``get_model_percentile_pa`` / ``get_model_mean`` / ``get_model_std``
  methods of the models (bisip_amd.utils.utils) and of SpectraBatch, as mixins.

``kind``: ``'ri'`` is Re and Im, what ``forward`` returns; ``'pa'`` is amplitude and minus phase (``response_pa``).
The rows of a spectrum are numbered ``k * Wp + w`` (sample ``k``, walker ``w``): the order of ``get_chain(flat=True)``.
"""

import numpy as np

__all__ = ('KINDS', 'response_pa', 'represent', 'model_percentile_pa', 'response_moments', 'plan',
           'ordered_response_moments', 'device_model_moments', 'ModelResponse', 'BatchResponse')

KINDS = ('ri', 'pa')


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError(f"kind must be 'ri' or 'pa', got {kind!r}")
    return kind


def response_pa(Z):
    """Amplitude and minus phase of responses ``Z (..., 2, N)`` (Re, Im): ``(..., 2, N)`` with

    * ``[..., 0, :] = np.hypot(re, im)``: the amplitude, normalised as ``zn`` is (``amp / norm_factor``);
    * ``[..., 1, :] = -np.arctan2(im, re)``: MINUS the phase in rad -- the sign and unit of the reference's ``plot_data``
      and ``plot_fit_pa``, and ``-data['pha']``.

    Nothing is unwrapped: the value lies in [-pi, pi].  A band or a moment of it is meaningful only while the samples
    stay away from +-pi, which holds for every model inside its prior box, where Re Z > 0."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim < 2 or Z.shape[-2] != 2:
        raise ValueError(f'expected responses (..., 2, N), got shape {Z.shape}')
    out = np.empty(Z.shape)
    with np.errstate(all='ignore'):
        out[..., 0, :] = np.hypot(Z[..., 0, :], Z[..., 1, :])
        out[..., 1, :] = -np.arctan2(Z[..., 1, :], Z[..., 0, :])
    return out


def represent(Z, kind):
    """``Z (..., 2, N)`` in the representation ``kind``: as it is (``'ri'``) or ``response_pa(Z)`` (``'pa'``)."""
    return response_pa(Z) if _check_kind(kind) == 'pa' else np.asarray(Z, dtype=np.float64)


def model_percentile_pa(Z, p):
    """``np.percentile(response_pa(Z), p, axis=0)`` of the responses ``Z (n, 2, N)`` of a chain: the amplitude / phase
    band of the posterior."""
    return np.percentile(response_pa(Z), p, axis=0)


def response_moments(Z, kind='ri'):
    """``(mean, std)`` over axis 0 of the responses ``Z (n, ..., 2, N)`` in the representation ``kind``: ``np.mean`` and
    ``np.std`` with ddof = 0, as get_param_std."""
    x = represent(Z, kind)
    with np.errstate(all='ignore'):
        return np.mean(x, axis=0), np.std(x, axis=0)


# -- the device's order of summation ------------------------------------------------------------------------------------
# row_pass.h: RM_WGS, RM_ONE_SEGMENT, RM_SEG_MAX, RM_SEG_MIN, RM_THREADS
WORKGROUPS_WANTED, ONE_SEGMENT_SPECTRA, SEGMENT_MAX, SEGMENT_MIN, SLOTS = 2048, 256, 1 << 30, 1024, 256


def plan(n_samples, n_spectra, walkers_per_ensemble):
    """``(seg_rows, nseg, slots)``: how bisip_response_moments_dev cuts the ``n_samples * walkers_per_ensemble`` rows of
    a spectrum into segments, and over how many row slots it spreads the rows of one -- a function of the shape alone."""
    R, E = int(n_samples) * int(walkers_per_ensemble), int(n_spectra)
    if R < 1 or E < 1:
        raise ValueError('no rows')
    seg_rows = R if E >= ONE_SEGMENT_SPECTRA else max(SEGMENT_MIN, -(-R // (WORKGROUPS_WANTED // E)))
    seg_rows = min(seg_rows, SEGMENT_MAX)
    return seg_rows, -(-R // seg_rows), SLOTS


def ordered_response_moments(Z, kind='ri', n_spectra=None):
    """``(mean, std)``, ``(E, 2, N)`` each, with the bits bisip_response_moments_dev produces from the responses ``Z (E, R,
    2, N)`` (Re, Im) of the R rows of E spectra -- ``(R, 2, N)``: one spectrum -- in the order include/bisip_hip.h states:
    sums shifted by the response of the spectrum's first row; row ``i`` of a segment to slot ``i mod 256``, a slot's rows
    in ascending order; slots pairwise within runs of 64, the four runs in ascending order; segments in ascending order;
    products rounded on their own.  ``n_spectra``: the spectra of the call when ``Z`` holds only some of them (the plan
    depends on it).  ``kind='pa'`` takes NumPy's hypot / arctan2 where the device takes its own: the same order, not
    necessarily the same bits.  The rows of a sample whose parameters are not finite must be NaN in ``Z``."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 3:
        Z = Z[None]
    if Z.ndim != 4 or Z.shape[2] != 2:
        raise ValueError(f'expected responses (E, R, 2, N) or (R, 2, N), got shape {Z.shape}')
    E, R, _, N = Z.shape
    seg_rows, nseg, T = plan(R, E if n_spectra is None else n_spectra, 1)
    x = represent(Z, kind).reshape(E, R, 2 * N)
    with np.errstate(all='ignore'):
        c = x[:, 0, :]
        total = None
        for g in range(nseg):
            r0, r1 = g * seg_rows, min(R, (g + 1) * seg_rows)
            acc = np.zeros((E, T, 4 * N))
            for t0 in range(r0, r1, T):
                d = x[:, t0:min(r1, t0 + T)] - c[:, None, :]
                k = d.shape[1]                       # (a slot beyond the last row adds nothing)
                acc[:, :k, :2 * N] = acc[:, :k, :2 * N] + d
                acc[:, :k, 2 * N:] = acc[:, :k, 2 * N:] + d * d
            acc = acc.reshape(E, T // 64, 64, 4 * N)
            w = 32
            while w >= 1:
                acc = acc[:, :, :w] + acc[:, :, w:2 * w]
                w //= 2
            s = acc[:, 0, 0]
            for q in range(1, T // 64):
                s = s + acc[:, q, 0]
            total = s if g == 0 else total + s
        S, P = total[:, :2 * N], total[:, 2 * N:]
        mean = c + S / float(R)
        var = (P - (S * S) / float(R)) / float(R)
        var = np.where(var < 0.0, 0.0, var)          # (a NaN stays)
        std = np.sqrt(var)
    return mean.reshape(E, 2, N), std.reshape(E, 2, N)


def row_pass_workspace(view, ctx, workspace):
    """``(n, E, Wp, work, nbytes)`` for one of the fused passes over the rows of a ChainView (bisip_response_moments_dev,
    bisip_fit_quality_dev, bisip_predictive_check_dev): the view's shape, held against the model of ``ctx``, and the
    ``nbytes`` of device scratch that ``workspace(n, E, Wp)`` of the context asks for (``work``: None for 0 bytes)."""
    import torch
    n, E, Wp = view.n, view.n_ensembles, view.walkers_per_ensemble
    if view.ndim != ctx.ndim:
        raise ValueError(f'a chain of {view.ndim} parameters for a model of {ctx.ndim}')
    nbytes = workspace(n, E, Wp)
    if nbytes < 0:
        raise ValueError(f'a chain of {E} ensembles of {Wp} walkers is too large for one launch')
    return n, E, Wp, (view.empty((nbytes,), torch.uint8) if nbytes else None), nbytes


def device_model_moments(view, ctx, kind='ri', first_spectrum=0, mean=True, std=True):
    """``(mean, std)`` of the model response of ``ctx`` (a HipContext) over every ensemble's samples of a ChainView, in
    the representation ``kind``: ``(n_ensembles, 2, N)`` each (NumPy; None for the one not asked for), taken where the
    chain lies (bisip_response_moments_dev).  Ensemble ``e`` of the view is spectrum ``first_spectrum + e`` of the
    context."""
    import torch
    _check_kind(kind)
    if view.ndim == ctx.ndim and not (mean or std):      # (a chain of another model is reported first, below)
        raise ValueError('neither mean nor std asked for')
    n, E, Wp, work, nbytes = row_pass_workspace(view, ctx, ctx.response_moments_workspace)
    m = view.empty((E, 2, ctx.N), torch.float64) if mean else None
    s = view.empty((E, 2, ctx.N), torch.float64) if std else None
    ctx.response_moments_dev(first_spectrum, E, view.ptr, n, view.stride, Wp, kind, m.data_ptr() if mean else 0,
                             s.data_ptr() if std else 0, work.data_ptr() if nbytes else 0, nbytes, view.stream)
    view.synchronize()
    return (m.cpu().numpy() if mean else None), (s.cpu().numpy() if std else None)


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelResponse:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are get_model_percentile's."""

    def get_model_percentile_pa(self, p=[2.5, 50, 97.5], chain=None, **kwargs):
        """Percentiles of the AMPLITUDE and of MINUS THE PHASE of the model response over a chain -- the band the
        reference's plot_fit_pa means to draw -- ``(len(p), 2, N)``, ``(2, N)`` for a scalar ``p``:
        ``np.percentile(response_pa(forward(chain)), p, axis=0)`` (bisip_amd.response), every sample's own amplitude and
        phase, taken on the device.  ``[:, 0]`` is ``amp / norm_factor``, ``[:, 1]`` compares with ``-data['pha']``.
        ``chain`` / ``discard`` / ``thin`` as get_model_percentile."""
        from .utils import discard_thin, first_if_scalar
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None:       # fit(chain='device'): forward and percentiles where the chain lies
            try:
                return first_if_scalar(p, s.model_percentiles_pa(p, **discard_thin(kwargs)))
            except NotImplementedError:
                pass
        chain = np.ascontiguousarray(self.parse_chain(chain, **kwargs), dtype=np.float64)
        return first_if_scalar(p, self._context().forward_percentiles_kind(chain, p, 'pa'))

    def _model_moments(self, chain, kind, kwargs):
        from .utils import discard_thin
        _check_kind(kind)
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None and s.n_ensembles == 1:      # fit(chain='device'): reduced where the chain lies
            mean, std = s.model_moments(kind, **discard_thin(kwargs))
            return mean[0], std[0]
        from .chainview import host_chain_view
        flat, ctx = self.parse_chain(chain, **kwargs), self._context()
        mean, std = device_model_moments(host_chain_view(flat, ctx), ctx, kind)
        return mean[0], std[0]

    def get_model_mean(self, chain=None, kind='ri', **kwargs):
        """The posterior mean of the model response, ``(2, N)``: ``np.mean(forward(chain), axis=0)`` (``kind='ri'``) or
        of its amplitude and minus phase (``kind='pa'``: bisip_amd.response.response_pa), evaluated and summed on the
        device in one pass over the chain, no response stored (bisip_response_moments_dev).  ``chain`` / ``discard`` /
        ``thin`` as get_model_percentile."""
        return self._model_moments(chain, kind, kwargs)[0]

    def get_model_std(self, chain=None, kind='ri', **kwargs):
        """The posterior standard deviation (ddof = 0) of the model response, ``(2, N)``.  Arguments as get_model_mean."""
        return self._model_moments(chain, kind, kwargs)[1]


class BatchResponse:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler, ``ctx`` its context)."""

    def get_model_percentile_pa(self, p=(2.5, 50, 97.5), discard=0, thin=1):
        """Percentiles of the amplitude and of minus the phase of the model response over every spectrum's chain,
        ``(len(p), E, 2, N)`` -- per spectrum ``np.percentile(response_pa(forward(chain)), p, axis=0)``
        (bisip_amd.response) -- on the device as get_model_percentile: the forward launch writes amplitude / phase columns,
        one selection of the order statistics.  Under torch.distributed every rank returns its own spectra."""
        from .summaries import device_model_percentiles
        out = device_model_percentiles(self._fitted().used_samples_dev(discard, thin), self.ctx, p, 'pa')
        return out.reshape(-1, self.n_spectra, 2, self.N)

    def get_model_mean(self, kind='ri', discard=0, thin=1):
        """The posterior mean of every spectrum's model response, ``(E, 2, N)``, in the representation ``kind`` ('ri' or
        'pa'): one fused pass over the chain where it lies (bisip_response_moments_dev), for ``chain='device'`` and
        ``'host'`` alike.  Under torch.distributed every rank returns its own spectra."""
        return self._fitted().model_moments(kind, discard=discard, thin=thin)[0]

    def get_model_std(self, kind='ri', discard=0, thin=1):
        """The posterior standard deviation (ddof = 0) of every spectrum's model response, ``(E, 2, N)``."""
        return self._fitted().model_moments(kind, discard=discard, thin=thin)[1]
