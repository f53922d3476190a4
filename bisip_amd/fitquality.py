"""Which model does the spectrum support, and at which frequencies does the chosen one fail: WAIC, DIC and the per-point
misfit of a chain.

The data points of a spectrum are its 2N values, Re and Im at each frequency.  For a sample ``theta`` of the chain,
``q[part, j] = (y - forward(theta))^2 / sigma^2`` is the squared standardised residual of a point and
``l = -0.5 q - log sigma^2`` its log-likelihood with the reference's own constant (src/bisip/models.py:59-62): the sum of
``l`` over the 2N points is the sample's stored log-probability.  Three sums per point over the rows of the chain carry
everything: the mean of ``q`` (the misfit: near 1, the point is fitted to its error bar), its variance (ddof = 1) and
``lmeh = log(mean(exp(-q / 2)))``.

* ``inverse_variance``, ``pointwise_q``, ``pointwise_log_lik``, ``fit_sums``, ``waic``, ``waic_from_sums``, ``dic``,
  ``compare_waic``: the definitions, plain NumPy in float64 (WAIC: Watanabe 2010; Vehtari, Gelman & Gabry 2017; DIC:
  Spiegelhalter et al. 2002);
* ``device_fit_quality`` runs ``bisip_fit_quality_dev`` on a ChainView (bisip_amd.chainview) where the chain lies: the
  model is evaluated in registers, no response and no ``q`` is stored;
* ``ordered_fit_sums`` restates the order of every sum of that kernel (include/bisip_hip.h) in NumPy: the same bits of
  ``mean_q`` and ``var_q`` from the same responses, ``lmeh`` in the same order with NumPy's ``exp``;
* ``ModelFitQuality`` and ``BatchFitQuality`` are the ``get_pointwise_misfit`` / ``get_waic`` / ``get_dic`` methods of the
  models (bisip_amd.utils.utils) and of SpectraBatch, as mixins.

The rows of a spectrum are numbered ``k * Wp + w`` (sample ``k``, walker ``w``): the order of ``get_chain(flat=True)``.
PSIS-LOO, which needs a sort per data point, is bisip_amd.loo.
"""

import warnings

import numpy as np

from .response import plan, row_pass_workspace

__all__ = ('P_WAIC_HIGH', 'inverse_variance', 'pointwise_q', 'pointwise_log_lik', 'fit_sums', 'waic', 'waic_from_sums',
           'dic', 'compare_waic', 'ordered_fit_sums', 'device_fit_quality', 'ModelFitQuality', 'BatchFitQuality')

P_WAIC_HIGH = 0.4      # a point whose p_waic_i exceeds this makes WAIC unreliable (Vehtari, Gelman & Gabry 2017, section 4)


# -- the definitions -----------------------------------------------------------------------------------------------------
def inverse_variance(err):
    """``1 / err^2`` as the context holds it: squared and inverted in long double, rounded once to double
    (host_precompute.cpp: common_operands)."""
    e = np.asarray(err, dtype=np.float64).astype(np.longdouble)
    with np.errstate(all='ignore'):
        return (np.longdouble(1) / (e * e)).astype(np.float64)


def pointwise_q(Z, y, iv):
    """``q = (y - Z)^2 * iv`` of responses ``Z (..., 2, N)``, the normalised measurement ``y`` and the inverse variance
    ``iv`` (both broadcast against Z): ``d = y - Z``, ``t = d * d``, ``q = t * iv``, each rounded on its own."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim < 2 or Z.shape[-2] != 2:
        raise ValueError(f'expected responses (..., 2, N), got shape {Z.shape}')
    with np.errstate(all='ignore'):
        d = np.asarray(y, dtype=np.float64) - Z
        t = d * d
        return t * np.asarray(iv, dtype=np.float64)


def pointwise_log_lik(Z, y, err):
    """The log-likelihood of every data point, ``l = -0.5 q - log(err^2)`` with ``q = pointwise_q(Z, y,
    inverse_variance(err))``: ``l.sum(axis=(-2, -1))`` is the reference's ``_log_likelihood``."""
    err = np.asarray(err, dtype=np.float64)
    return -0.5 * pointwise_q(Z, y, inverse_variance(err)) - np.log(err ** 2)


def fit_sums(q):
    """``(mean_q, var_q, lmeh)`` over axis 0 of ``q (R, ...)``: ``np.mean``, ``np.var`` with ddof = 1 (NaN for one row) and
    ``lmeh = log(mean(exp(-q / 2)))``, evaluated as ``-m / 2 + log(mean(exp(-(q - m) / 2)))`` with ``m = min q``."""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        m = np.min(q, axis=0)
        lmeh = -m / 2 + np.log(np.mean(np.exp(-(q - m) / 2), axis=0))
        return np.mean(q, axis=0), np.var(q, axis=0, ddof=1), lmeh


def _waic_of_points(lppd, p_i, axis):
    """The WAIC dict of pointwise ``lppd`` and ``p_waic_i``; the points of a spectrum lie along ``axis``."""
    with np.errstate(all='ignore'):
        elpd_i = lppd - p_i
        n_points = int(np.prod([lppd.shape[a] for a in axis]))
        elpd = elpd_i.sum(axis=axis)
        out = dict(elpd_waic=elpd, p_waic=p_i.sum(axis=axis), waic=-2 * elpd,
                   se=np.sqrt(n_points * np.var(elpd_i, axis=axis)), n_high=(p_i > P_WAIC_HIGH).sum(axis=axis),
                   lppd=lppd, p_waic_i=p_i, elpd_i=elpd_i)
    if np.ndim(elpd) == 0:
        out.update({k: float(out[k]) for k in ('elpd_waic', 'p_waic', 'waic', 'se')}, n_high=int(out['n_high']))
    return out


def waic(log_lik):
    """WAIC of the pointwise log-likelihoods ``log_lik (R, ...)`` of R posterior samples, the trailing axes being the data
    points of ONE spectrum: per point ``lppd_i = log(mean(exp(l)))`` and ``p_waic_i = var(l)`` with ddof = 1, ``elpd_i =
    lppd_i - p_waic_i``; ``elpd_waic`` and ``p_waic`` their sums, ``waic = -2 elpd_waic``, ``se = sqrt(n var(elpd_i))`` over
    the n points and ``n_high`` the number of points with ``p_waic_i > 0.4``."""
    ll = np.asarray(log_lik, dtype=np.float64)
    if ll.ndim < 2:
        raise ValueError(f'expected log-likelihoods (R, points...), got shape {ll.shape}')
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        top = np.max(ll, axis=0)
        lppd = top + np.log(np.mean(np.exp(ll - top), axis=0))
        p_i = np.var(ll, axis=0, ddof=1)
    return _waic_of_points(lppd, p_i, tuple(range(lppd.ndim)))


def waic_from_sums(var_q, lmeh, log_sigma2):
    """WAIC of ``fit_sums``' results ``(..., 2, N)`` and ``log sigma^2`` of the points: ``lppd_i = lmeh_i - log sigma_i^2``,
    ``p_waic_i = var_q_i / 4`` -- what ``waic(pointwise_log_lik)`` is, ``l`` being ``-q / 2`` plus a constant.  Leading axes
    (spectra) stay: the scalars of the result are then arrays of that shape."""
    var_q, lmeh = np.asarray(var_q, dtype=np.float64), np.asarray(lmeh, dtype=np.float64)
    if lmeh.ndim < 2 or lmeh.shape[-2] != 2 or var_q.shape != lmeh.shape:
        raise ValueError(f'expected sums (..., 2, N), got shapes {var_q.shape} and {lmeh.shape}')
    with np.errstate(all='ignore'):
        return _waic_of_points(lmeh - np.asarray(log_sigma2, dtype=np.float64), var_q / 4, (-2, -1))


def dic(mean_log_prob, log_prob_at_mean):
    """DIC of the mean of the samples' log-probability and the log-probability of the mean sample (scalars, or one per
    spectrum): ``mean_deviance = -2 mean``, ``deviance_at_mean = -2 log_prob(mean theta)``, ``p_d`` their difference,
    ``dic = mean_deviance + p_d``."""
    with np.errstate(all='ignore'):
        dbar = -2 * np.asarray(mean_log_prob, dtype=np.float64)
        dhat = -2 * np.asarray(log_prob_at_mean, dtype=np.float64)
        p_d = dbar - dhat
        out = dict(dic=dbar + p_d, p_d=p_d, mean_deviance=dbar, deviance_at_mean=dhat)
    return {k: float(v) for k, v in out.items()} if np.ndim(dbar) == 0 else out


def compare_waic(results):
    """Models fitted to the SAME spectrum, ranked: ``results`` maps a name to a ``get_waic`` / ``waic`` result; returns a
    list of dicts ``name, elpd_waic, p_waic, waic, se, n_high, d_elpd, d_se``, the largest ``elpd_waic`` first.  ``d_elpd``
    is the best model's ``elpd_waic`` minus the row's and ``d_se = sqrt(n var(elpd_i - elpd_i_best))`` the standard error
    of that difference over the n data points: a ``d_elpd`` of a few ``d_se`` or less does not separate two models."""
    if not results:
        raise ValueError('nothing to compare')
    points = {name: np.asarray(r['elpd_i'], dtype=np.float64) for name, r in results.items()}
    shapes = {p.shape for p in points.values()}
    if len(shapes) != 1:
        raise ValueError(f'the pointwise arrays differ in shape ({sorted(shapes)}): not the same data')
    for name, r in results.items():
        if np.ndim(r['elpd_waic']) != 0:
            raise ValueError(f'{name!r}: one spectrum at a time')
    order = sorted(results, key=lambda name: -float(results[name]['elpd_waic']))
    best = order[0]
    rows = []
    for name in order:
        r = results[name]
        diff = points[name] - points[best]
        rows.append(dict(name=name, elpd_waic=float(r['elpd_waic']), p_waic=float(r['p_waic']), waic=float(r['waic']),
                         se=float(r['se']), n_high=int(r['n_high']),
                         d_elpd=float(results[best]['elpd_waic']) - float(r['elpd_waic']),
                         d_se=float(np.sqrt(diff.size * np.var(diff)))))
    return rows


# -- the device's order of summation ------------------------------------------------------------------------------------
def _scale(d):
    return np.exp(-0.5 * d)


def _merge(ma, sa, mb, sb):
    """Two (m, s) pairs as one: the side whose m is larger is scaled, the other (both, when equal) is not."""
    a_hi, b_hi = ma > mb, mb > ma
    e = _scale(np.where(a_hi, ma - mb, mb - ma))
    return np.where(a_hi, mb, ma), np.where(a_hi, sa * e, sa) + np.where(b_hi, sb * e, sb)


def ordered_fit_sums(Z, y, iv, n_spectra=None):
    """``(mean_q, var_q, lmeh)``, ``(E, 2, N)`` each, of the responses ``Z (E, R, 2, N)`` (Re, Im) of the R rows of E spectra
    -- ``(R, 2, N)``: one spectrum -- with the measurement ``y`` and the inverse variance ``iv``, ``(E, 2, N)`` or ``(2,
    N)``, in the order include/bisip_hip.h states for bisip_fit_quality_dev: ``q`` in three roundings; sums shifted by the
    ``q`` of the spectrum's first row; row ``i`` of a segment to slot ``i mod 256``, a slot's rows in ascending order; a
    pair (m, s) per slot for ``lmeh``, one ``exp`` per row; slots pairwise within runs of 64, the four runs in ascending
    order; segments in ascending order.  ``mean_q`` and ``var_q`` have the device's bits; ``lmeh`` takes NumPy's exp and
    log where the device takes its own: the same order, not necessarily the same bits.  ``n_spectra``: the spectra of the
    call when ``Z`` holds only some of them (the plan depends on it).  The rows of a sample whose parameters are not
    finite must be NaN in ``Z``."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 3:
        Z = Z[None]
    if Z.ndim != 4 or Z.shape[2] != 2:
        raise ValueError(f'expected responses (E, R, 2, N) or (R, 2, N), got shape {Z.shape}')
    E, R, _, N = Z.shape
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), (E, 2, N))
    iv = np.broadcast_to(np.asarray(iv, dtype=np.float64), (E, 2, N))
    seg_rows, nseg, T = plan(R, E if n_spectra is None else n_spectra, 1)
    q = pointwise_q(Z, y[:, None], iv[:, None]).reshape(E, R, 2 * N)
    with np.errstate(all='ignore'):
        c = q[:, 0, :]
        total = None
        for g in range(nseg):
            r0, r1 = g * seg_rows, min(R, (g + 1) * seg_rows)
            S, P, s = (np.zeros((E, T, 2 * N)) for _ in range(3))
            m = np.full((E, T, 2 * N), np.inf)
            for t0 in range(r0, r1, T):
                rows = q[:, t0:min(r1, t0 + T)]
                k = rows.shape[1]                    # (a slot beyond the last row takes nothing)
                d = rows - c[:, None, :]
                S[:, :k] = S[:, :k] + d
                P[:, :k] = P[:, :k] + d * d
                mk, sk = m[:, :k], s[:, :k]
                lower = rows < mk
                e = _scale(np.where(lower, mk - rows, rows - mk))
                s[:, :k] = np.where(lower, sk * e + 1.0, sk + e)
                m[:, :k] = np.where(lower, rows, mk)
            S, P, m, s = (a.reshape(E, T // 64, 64, 2 * N) for a in (S, P, m, s))
            w = 32
            while w >= 1:
                S = S[:, :, :w] + S[:, :, w:2 * w]
                P = P[:, :, :w] + P[:, :, w:2 * w]
                m, s = _merge(m[:, :, :w], s[:, :, :w], m[:, :, w:2 * w], s[:, :, w:2 * w])
                w //= 2
            seg = [S[:, 0, 0], P[:, 0, 0], m[:, 0, 0], s[:, 0, 0]]
            for v in range(1, T // 64):
                seg[0], seg[1] = seg[0] + S[:, v, 0], seg[1] + P[:, v, 0]
                seg[2], seg[3] = _merge(seg[2], seg[3], m[:, v, 0], s[:, v, 0])
            if g == 0:
                total = seg
            else:
                total[0], total[1] = total[0] + seg[0], total[1] + seg[1]
                total[2], total[3] = _merge(total[2], total[3], seg[2], seg[3])
        S, P, m, s = total
        mean_q = c + S / float(R)
        var_q = (P - (S * S) / float(R)) / (float(R) - 1.0)
        var_q = np.where(var_q < 0.0, 0.0, var_q)    # (a NaN stays)
        lmeh = -0.5 * m + np.log(s / float(R))
    return mean_q.reshape(E, 2, N), var_q.reshape(E, 2, N), lmeh.reshape(E, 2, N)


def device_fit_quality(view, ctx, first_spectrum=0):
    """``(mean_q, var_q, lmeh)`` of the model of ``ctx`` (a HipContext) against its data over every ensemble's samples of
    a ChainView: ``(n_ensembles, 2, N)`` each (NumPy), taken where the chain lies (bisip_fit_quality_dev).  Ensemble ``e``
    of the view is spectrum ``first_spectrum + e`` of the context."""
    import torch
    n, E, Wp, work, nbytes = row_pass_workspace(view, ctx, ctx.fit_quality_workspace)
    out = view.empty((3, E, 2, ctx.N), torch.float64)
    ctx.fit_quality_dev(first_spectrum, E, view.ptr, n, view.stride, Wp, out[0].data_ptr(), out[1].data_ptr(),
                        out[2].data_ptr(), work.data_ptr() if nbytes else 0, nbytes, view.stream)
    view.synchronize()
    host = out.cpu().numpy()
    return host[0], host[1], host[2]


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelFitQuality:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are get_model_mean's."""

    def _fit_sums(self, chain, kwargs):
        from .utils import discard_thin
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None and s.n_ensembles == 1:      # fit(chain='device'): reduced where the chain lies
            return tuple(a[0] for a in s.fit_quality(**discard_thin(kwargs)))
        from .chainview import host_chain_view
        flat, ctx = self.parse_chain(chain, **kwargs), self._context()
        return tuple(a[0] for a in device_fit_quality(host_chain_view(flat, ctx), ctx))

    def get_pointwise_misfit(self, chain=None, **kwargs):
        """The posterior mean of the squared standardised residual of every data point, ``(2, N)`` (Re, Im):
        ``np.mean((zn - forward(chain))**2 / zn_err**2, axis=0)``, evaluated and summed on the device in one pass over
        the chain, no response stored (bisip_fit_quality_dev).  Near 1: the point is fitted to its error bar; far above:
        the model fails there.  ``chain`` / ``discard`` / ``thin`` as get_model_percentile."""
        return self._fit_sums(chain, kwargs)[0]

    def get_waic(self, chain=None, **kwargs):
        """The widely applicable information criterion of the fit (bisip_amd.fitquality.waic): a dict of ``elpd_waic``,
        ``p_waic``, ``waic = -2 elpd_waic``, its standard error ``se``, ``n_high`` (points with ``p_waic_i > 0.4``: WAIC is
        then unreliable; ``get_loo`` is the estimate to turn to, and its ``pareto_k`` shows which points) and the pointwise
        ``lppd``, ``p_waic_i``, ``elpd_i``, ``(2, N)`` each.  The sums over the chain are taken on the device;
        ``compare_waic`` ranks the results of several models of one spectrum.  ``chain`` / ``discard`` / ``thin`` as
        get_model_percentile."""
        _, var_q, lmeh = self._fit_sums(chain, kwargs)
        return waic_from_sums(var_q, lmeh, np.log(self._data['zn_err'] ** 2))

    def get_dic(self, chain=None, **kwargs):
        """The deviance information criterion (bisip_amd.fitquality.dic): a dict of ``dic``, ``p_d``, ``mean_deviance``
        (minus twice the mean of the samples' log-probability) and ``deviance_at_mean`` (minus twice the log-probability
        of the mean sample).  ``chain`` / ``discard`` / ``thin`` as get_model_percentile."""
        from .utils import discard_thin
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None and s.n_ensembles == 1:      # the stored log-probabilities and the chain, where they lie
            from .chainview import device_moments
            dt = discard_thin(kwargs)
            mean_lp = device_moments(s.log_prob_samples_dev(**dt))[0][0, 0]
            theta = s.param_moments(**dt)[0][0]
        else:
            flat = np.ascontiguousarray(self.parse_chain(chain, **kwargs), dtype=np.float64)
            theta = flat.mean(axis=0)
            if chain is None:
                mean_lp = self._sampler.get_log_prob(flat=True, **discard_thin(kwargs)).mean()
            else:
                mean_lp = np.mean(self.log_prob(flat))
        return dic(mean_lp, self.log_prob(theta))


class BatchFitQuality:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler, ``ctx`` its context)."""

    def get_pointwise_misfit(self, discard=0, thin=1):
        """The posterior mean of the squared standardised residual of every data point of every spectrum, ``(E, 2, N)``:
        one fused pass over the chain where it lies (bisip_fit_quality_dev), for ``chain='device'`` and ``'host'`` alike.
        Near 1: the point is fitted to its error bar.  Under torch.distributed every rank returns its own spectra."""
        return self._fitted().fit_quality(discard=discard, thin=thin)[0]

    def get_waic(self, discard=0, thin=1):
        """WAIC of every spectrum's fit (bisip_amd.fitquality.waic): a dict of ``elpd_waic``, ``p_waic``, ``waic``, ``se``,
        ``n_high``, ``(E,)`` each, and the pointwise ``lppd``, ``p_waic_i``, ``elpd_i``, ``(E, 2, N)`` each."""
        _, var_q, lmeh = self._fitted().fit_quality(discard=discard, thin=thin)
        return waic_from_sums(var_q, lmeh, np.log(self.zn_err ** 2))

    def get_dic(self, discard=0, thin=1):
        """DIC of every spectrum's fit (bisip_amd.fitquality.dic): a dict of ``dic``, ``p_d``, ``mean_deviance``,
        ``deviance_at_mean``, ``(E,)`` each."""
        from .chainview import device_moments
        s = self._fitted()
        mean_lp = device_moments(s.log_prob_samples_dev(discard, thin))[0][:, 0]
        theta = self.get_param_mean(discard, thin)
        return dic(mean_lp, self.log_prob(theta[:, None, :])[:, 0])
