"""Pareto-smoothed importance-sampling leave-one-out cross-validation (PSIS-LOO) of a chain, and the Pareto shape k-hat of
every data point: where ``get_waic`` reports ``n_high > 0`` this is the estimate to turn to, and ``pareto_k`` shows which
frequencies make a comparison fragile (Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling";
Vehtari, Gelman & Gabry 2017; the fit of the generalised Pareto distribution: Zhang & Stephens 2009).

The data points of a spectrum are its 2N values (bisip_amd.fitquality).  Per data point, over a column ``q`` of R >= 2
values ``q = fitquality.pointwise_q`` -- the log importance ratio of a row is ``q / 2``:

1. ``M = tail_length(R, reff)``; ``s = sort(q)``, ``qmax = s[R - 1]``, ``u = s[R - M - 1]``; the tail is the values strictly
   greater than ``u``, ``n_tail <= M`` of them (ties at ``u`` stay in the body); ``r(x) = exp((x - qmax) / 2)``, ``eu = r(u)``.
2. ``n_tail <= 4``: ``khat = +inf``, nothing is smoothed (``w = r``).
3. Else ``gpd_fit`` of ``x = r(tail) - eu`` in ascending order gives ``khat`` and ``sigma``; a ``khat`` that is not finite is
   reported as ``+inf`` and the point stays unsmoothed.
4. The smoothed tail: ``w_j = min(eu + sigma * expm1(-khat * log1p(-p_j)) / khat, 1)``, ``p_j = (j + 0.5) / n_tail``.
5. ``elpd_rel = -qmax / 2 + log((R - n_tail) + sum_tail w_j / r_j) - log(sum_body r + sum_tail w_j)``; for an unsmoothed
   point every ``w_j / r_j`` is 1 and the second term is ``log R``.  The point's ``elpd_loo_i = elpd_rel - log sigma_i^2``.
6. A column that holds a NaN gives NaN ``elpd_rel``, ``khat`` and ``sigma``, and ``n_tail = 0``.

Departure from ArviZ: ArviZ raises the threshold to ``log(DBL_MIN)`` below the maximum, which can make the tail longer than
M.  Here ``eu`` may underflow to 0 instead; the fit then meets a division by zero and step 3's rule reports ``+inf``.

* ``tail_length``, ``gpd_fit``, ``psis_loo_columns``, ``loo``, ``loo_from_columns``, ``k_threshold``, ``compare_loo``: the
  definitions, plain NumPy in float64;
* ``ordered_columns`` restates the order of every sum of bisip_loo_columns_dev (include/bisip_hip.h) with NumPy's ``exp``,
  ``log``, ``log1p`` and ``expm1``: the same order, not necessarily the same bits;
* ``device_loo`` runs the spectra of a ChainView in passes: bisip_forward_columns_dev, bisip_q_columns_dev,
  bisip_loo_columns_dev, the columns never leaving the device;
* ``ModelLoo`` and ``BatchLoo`` are the ``get_loo`` methods of the models (bisip_amd.utils.utils) and of SpectraBatch.
"""

import warnings

import numpy as np

__all__ = ('tail_length', 'gpd_fit', 'psis_loo_columns', 'loo', 'loo_from_columns', 'k_threshold', 'compare_loo',
           'ordered_columns', 'device_loo', 'ModelLoo', 'BatchLoo')

MIN_TAIL = 5             # a tail of fewer values is not fitted (n_tail <= 4: khat = +inf)
PRIOR_BS, PRIOR_K = 3, 10
CHUNK, SLOTS, WAVE = 4096, 256, 64     # the device's compaction chunk, the slots of a workgroup, those of a wave


# -- the definitions -----------------------------------------------------------------------------------------------------
def tail_length(R, reff=1.0):
    """``M = ceil(min(R / 5, 3 * sqrt(R / reff)))``: how many of the R >= 2 values of a column the tail may hold.  ``reff``, the
    relative efficiency of the chain (1.0: independent draws), sets nothing else."""
    R = int(R)
    reff = float(reff)
    if R < 2:
        raise ValueError(f'a column of {R} value(s): PSIS-LOO needs two at least')
    if not (0.0 < reff < np.inf):
        raise ValueError(f'reff must be positive and finite, got {reff}')
    return int(np.ceil(min(R / 5, 3 * np.sqrt(R / reff))))


def gpd_fit(x):
    """``(khat, sigma)`` of the generalised Pareto distribution fitted to the exceedances ``x (n,)``, ascending, by Zhang &
    Stephens' profile likelihood with the weakly informative prior: ``m = 30 + floor(sqrt(n))`` points ``b_j = 1 / x[n-1] +
    (1 - sqrt(m / (j - 0.5))) / (3 x[floor(n / 4 + 0.5) - 1])``, ``k_j = mean(log1p(-b_j x))``, ``L_j = n (log(-b_j / k_j) -
    k_j - 1)``, ``w_j = 1 / sum_i exp(L_i - L_j)``, ``b = sum b_j w_j``, ``k = mean(log1p(-b x))``, ``sigma = -k / b``,
    ``khat = k n / (n + 10) + 5 / (n + 10)``.  A ``khat`` that is not finite comes back as ``(+inf, NaN)``."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or x.size < 1:
        raise ValueError(f'expected exceedances (n,), n >= 1, got shape {x.shape}')
    n = x.size
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        m = 30 + int(np.floor(np.sqrt(n)))
        j = np.arange(1, m + 1, dtype=np.float64)
        b = 1 / x[n - 1] + (1 - np.sqrt(m / (j - 0.5))) / (PRIOR_BS * x[int(np.floor(n / 4 + 0.5)) - 1])
        k = np.mean(np.log1p(-b[:, None] * x), axis=1)
        L = n * (np.log(-b / k) - k - 1)
        w = 1 / np.sum(np.exp(L - L[:, None]), axis=1)
        b_post = np.sum(b * w)
        k_post = np.mean(np.log1p(-b_post * x))
        sigma = -k_post / b_post
        khat = k_post * n / (n + PRIOR_K) + PRIOR_K * 0.5 / (n + PRIOR_K)
    if not np.isfinite(khat):
        return np.inf, np.nan
    return float(khat), float(sigma)


def _psis_column(q, M):
    """``(elpd_rel, khat, sigma, n_tail)`` of one column ``q (R,)`` with a tail of at most M values."""
    R = q.size
    if np.isnan(q).any():
        return np.nan, np.nan, np.nan, 0
    with np.errstate(all='ignore'):
        s = np.sort(q)
        qmax, u = s[R - 1], s[R - M - 1]
        tail = s[s > u]
        n_tail = tail.size
        r_tail = np.exp((tail - qmax) / 2)
        eu = np.exp((u - qmax) / 2)
        khat, sigma = np.inf, np.nan
        if n_tail >= MIN_TAIL:
            khat, sigma = gpd_fit(r_tail - eu)
        sum_body = np.sum(np.exp((s[:R - n_tail] - qmax) / 2))
        if np.isfinite(khat):
            p = (np.arange(n_tail) + 0.5) / n_tail
            w = np.minimum(eu + sigma * np.expm1(-khat * np.log1p(-p)) / khat, 1)
            ratio = np.sum(w / r_tail)
        else:
            w, ratio = r_tail, float(n_tail)
        elpd = -qmax / 2 + np.log((R - n_tail) + ratio) - np.log(sum_body + np.sum(w))
    return float(elpd), khat, sigma, n_tail


def _columns(q, reff, one):
    q = np.asarray(q, dtype=np.float64)
    if q.ndim < 1 or q.shape[0] < 2:
        raise ValueError(f'expected columns (R, ...), R >= 2, got shape {q.shape}')
    R, shape = q.shape[0], q.shape[1:]
    M = tail_length(R, reff)
    flat = q.reshape(R, -1)
    out = (np.empty(flat.shape[1]), np.empty(flat.shape[1]), np.empty(flat.shape[1]), np.empty(flat.shape[1], np.int64))
    for c in range(flat.shape[1]):
        for o, v in zip(out, one(flat[:, c], M)):
            o[c] = v
    return tuple(o.reshape(shape) for o in out)


def psis_loo_columns(q, reff=1.0):
    """``(elpd_rel, khat, sigma, n_tail)`` over axis 0 of ``q (R, ...)``, every column on its own (steps 1 to 6 of the module's
    docstring); ``n_tail`` is int64, ``sigma`` NaN wherever ``khat`` is not finite."""
    return _columns(q, reff, _psis_column)


def k_threshold(R):
    """``min(1 - 1 / log10(R), 0.7)``: the Pareto k above which the estimate of a point from R samples is unreliable."""
    R = int(R)
    if R < 2:
        raise ValueError(f'{R} sample(s)')
    return float(min(1 - 1 / np.log10(R), 0.7))


def _loo_of_points(elpd_i, lppd, khat, n_tail, R, axis):
    """The LOO dict of pointwise results; the points of a spectrum lie along ``axis``."""
    with np.errstate(all='ignore'):
        p_i = lppd - elpd_i
        n_points = int(np.prod([elpd_i.shape[a] for a in axis]))
        elpd = elpd_i.sum(axis=axis)
        kt = k_threshold(R)
        out = dict(elpd_loo=elpd, p_loo=p_i.sum(axis=axis), looic=-2 * elpd,
                   se=np.sqrt(n_points * np.var(elpd_i, axis=axis)), n_bad=(khat > kt).sum(axis=axis), k_threshold=kt,
                   elpd_i=elpd_i, p_loo_i=p_i, pareto_k=khat, n_tail=n_tail)
    if np.ndim(elpd) == 0:
        out.update({k: float(out[k]) for k in ('elpd_loo', 'p_loo', 'looic', 'se')}, n_bad=int(out['n_bad']))
    return out


def loo_from_columns(elpd_rel, khat, n_tail, lmeh, log_sigma2, R):
    """PSIS-LOO of ``psis_loo_columns``' results ``(..., 2, N)``, ``fitquality.fit_sums``' ``lmeh`` and ``log sigma^2`` of the
    points, from R samples: ``elpd_i = elpd_rel - log sigma_i^2``, ``p_loo_i = (lmeh_i - log sigma_i^2) - elpd_i``; ``elpd_loo``
    and ``p_loo`` their sums over the points, ``looic = -2 elpd_loo``, ``se = sqrt(n var(elpd_i))``, ``n_bad`` the number of
    points with ``pareto_k > k_threshold(R)``.  Leading axes (spectra) stay: the scalars of the result are then arrays."""
    elpd_rel, khat, lmeh = (np.asarray(a, dtype=np.float64) for a in (elpd_rel, khat, lmeh))
    n_tail = np.asarray(n_tail, dtype=np.int64)
    if lmeh.ndim < 2 or lmeh.shape[-2] != 2 or not (elpd_rel.shape == khat.shape == n_tail.shape == lmeh.shape):
        raise ValueError(f'expected results (..., 2, N), got shapes {elpd_rel.shape}, {khat.shape}, {n_tail.shape} and '
                         f'{lmeh.shape}')
    with np.errstate(all='ignore'):
        ls2 = np.asarray(log_sigma2, dtype=np.float64)
        return _loo_of_points(elpd_rel - ls2, lmeh - ls2, khat, n_tail, R, (-2, -1))


def loo(log_lik, reff=1.0):
    """PSIS-LOO of the pointwise log-likelihoods ``log_lik (R, ...)`` of R posterior samples, the trailing axes being the data
    points of ONE spectrum: the log importance ratios are ``-log_lik``, smoothed per point (``psis_loo_columns`` of ``q = -2
    log_lik``); ``elpd_i = log(sum w exp(l) / sum w)``, ``p_loo_i = lppd_i - elpd_i`` with ``lppd_i = log(mean(exp(l)))``."""
    ll = np.asarray(log_lik, dtype=np.float64)
    if ll.ndim < 2:
        raise ValueError(f'expected log-likelihoods (R, points...), got shape {ll.shape}')
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        elpd_i, khat, _, n_tail = psis_loo_columns(-2 * ll, reff)
        top = np.max(ll, axis=0)
        lppd = top + np.log(np.mean(np.exp(ll - top), axis=0))
    return _loo_of_points(elpd_i, lppd, khat, n_tail, ll.shape[0], tuple(range(lppd.ndim)))


def compare_loo(results):
    """Models fitted to the SAME spectrum, ranked: ``results`` maps a name to a ``get_loo`` / ``loo`` result; returns a list of
    dicts ``name, elpd_loo, p_loo, looic, se, n_bad, d_elpd, d_se``, the largest ``elpd_loo`` first.  ``d_elpd`` is the best
    model's ``elpd_loo`` minus the row's and ``d_se = sqrt(n var(elpd_i - elpd_i_best))`` the standard error of that
    difference over the n data points (``fitquality.compare_waic``'s shape and rules)."""
    if not results:
        raise ValueError('nothing to compare')
    points = {name: np.asarray(r['elpd_i'], dtype=np.float64) for name, r in results.items()}
    shapes = {p.shape for p in points.values()}
    if len(shapes) != 1:
        raise ValueError(f'the pointwise arrays differ in shape ({sorted(shapes)}): not the same data')
    for name, r in results.items():
        if np.ndim(r['elpd_loo']) != 0:
            raise ValueError(f'{name!r}: one spectrum at a time')
    order = sorted(results, key=lambda name: -float(results[name]['elpd_loo']))
    best = order[0]
    rows = []
    for name in order:
        r = results[name]
        diff = points[name] - points[best]
        rows.append(dict(name=name, elpd_loo=float(r['elpd_loo']), p_loo=float(r['p_loo']), looic=float(r['looic']),
                         se=float(r['se']), n_bad=int(r['n_bad']),
                         d_elpd=float(results[best]['elpd_loo']) - float(r['elpd_loo']),
                         d_se=float(np.sqrt(diff.size * np.var(diff)))))
    return rows


# -- the device's order of summation ------------------------------------------------------------------------------------
def _slot_sum(v, slots):
    """The values ``v (..., n)``, value i to slot i mod ``slots``, a slot in ascending order from 0.0: ``(..., slots)``."""
    n = v.shape[-1]
    rows = -(-n // slots)
    pad = np.zeros(v.shape[:-1] + (rows * slots,))
    pad[..., :n] = v
    pad = pad.reshape(v.shape[:-1] + (rows, slots))
    acc = np.zeros(v.shape[:-1] + (slots,))
    for k in range(rows):
        acc = acc + pad[..., k, :]                   # (a slot beyond the last value adds 0.0: no change)
    return acc


def _wave_tree(acc):
    """Runs of 64 slots pairwise, 32, 16, ..., 1 apart: ``(..., runs)``."""
    acc = acc.reshape(acc.shape[:-1] + (-1, WAVE))
    w = WAVE // 2
    while w >= 1:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


def _block_sum(v):
    """Value i to slot i mod 256, the slots pairwise within each run of 64, the four runs in ascending order."""
    w = _wave_tree(_slot_sum(v, SLOTS))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _ordered_column(q, M):
    R = q.size
    if np.isnan(q).any():
        return np.nan, np.nan, np.nan, 0
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        s = np.sort(q)
        qmax, u = s[R - 1], s[R - M - 1]
        eu = np.exp(0.5 * (u - qmax))
        # the body sum: chunks of 4096 values of the column as it is stored, a value of the tail adds 0.0
        chunks = -(-R // CHUNK)
        term = np.zeros(chunks * CHUNK)
        term[:R] = np.where(q <= u, np.exp(0.5 * (q - qmax)), 0.0)
        body = 0.0
        for part in _block_sum(term.reshape(chunks, CHUNK)):
            body = body + part
        tail = s[s > u]
        n = tail.size
        nd = float(n)
        r = np.exp(0.5 * (tail - qmax))
        khat, sigma, smooth = np.inf, np.nan, False
        if n >= MIN_TAIL:
            x = r - eu
            m = 30 + int(np.floor(np.sqrt(nd)))
            j = np.arange(1, m + 1, dtype=np.float64)
            b = 1.0 / x[n - 1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * x[int(np.floor(nd / 4.0 + 0.5)) - 1])
            k = _wave_tree(_slot_sum(np.log1p(-b[:, None] * x), WAVE))[:, 0] / nd
            L = nd * ((np.log(-b / k) - k) - 1.0)
            den = np.zeros(m)
            for i in range(m):
                den = den + np.exp(L[i] - L)
            bw = b * (1.0 / den)
            b_post = 0.0
            for v in bw:
                b_post = b_post + v
            k_post = _block_sum(np.log1p(-b_post * x)) / nd
            sigma = -k_post / b_post
            khat = (k_post * nd) / (nd + 10.0) + 5.0 / (nd + 10.0)
            smooth = bool(np.isfinite(khat))
            if not smooth:
                khat, sigma = np.inf, np.nan
        if smooth:
            p = (np.arange(n) + 0.5) / nd
            w = eu + (sigma * np.expm1(-khat * np.log1p(-p))) / khat
            w = np.where(w > 1.0, 1.0, w)
            sw, swr = _block_sum(w), _block_sum(w / r)
        else:
            sw, swr = _block_sum(r), nd
        elpd = (-0.5 * qmax + np.log((R - nd) + swr)) - np.log(body + sw)
    return float(elpd), float(khat), float(sigma), n


def ordered_columns(q, reff=1.0):
    """``psis_loo_columns`` in the order include/bisip_hip.h states for bisip_loo_columns_dev: the body sum over chunks of 4096
    values of the column as it is stored (value i of a chunk to slot i mod 256, slots pairwise within runs of 64, the four
    runs and then the chunks in ascending order); every profile point over slots i mod 64; the softmax denominators and
    ``b`` in ascending order; ``k`` and the two sums of the tail over slots i mod 256 and the same tree.  NumPy's ``exp``,
    ``log``, ``log1p`` and ``expm1`` stand where the device takes its own."""
    return _columns(q, reff, _ordered_column)


# -- on the device -------------------------------------------------------------------------------------------------------
def device_loo(view, ctx, reff=1.0, first_spectrum=0):
    """``(elpd_rel, khat, n_tail)`` of the model of ``ctx`` (a HipContext) against its data over every ensemble's samples of a
    ChainView: ``(n_ensembles, 2, N)`` each (NumPy; ``n_tail`` int64).  Ensemble ``e`` of the view is spectrum
    ``first_spectrum + e`` of the context.  Spectra go in passes whose columns stay under ``decomposition.RTD_PASS_BYTES``:
    the forward launch writes the responses column by column (bisip_forward_columns_dev), bisip_q_columns_dev turns them
    into ``q`` where they lie and bisip_loo_columns_dev takes every column's tail."""
    import torch
    from . import _hip, decomposition
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    if ndim != ctx.ndim:
        raise ValueError(f'a chain of {ndim} parameters for a model of {ctx.ndim}')
    rows_per, cols = n * Wp, 2 * ctx.N
    M = tail_length(rows_per, reff)
    G = int(min(E, max(1, decomposition.RTD_PASS_BYTES // (rows_per * cols * 8))))
    elpd, khat, n_tail = np.empty((E, cols)), np.empty((E, cols)), np.empty((E, cols), np.int64)
    grid = view.samples().reshape(n, E, Wp, ndim)
    for g0 in range(0, E, G):
        k = min(E, g0 + G) - g0
        nbytes = _hip.loo_columns_workspace(rows_per, k * cols, M)
        if nbytes < 0:
            raise ValueError(f'{k * cols} columns of {rows_per} values with tails of {M} are too large for one pass')
        # one copy, spectrum-major (contiguous(): one walker of one spectrum behind a stride reshapes without a copy)
        rows = grid[:, g0:g0 + k].permute(1, 0, 2, 3).reshape(k, rows_per, ndim).contiguous()
        qc = view.empty((k, cols, rows_per), torch.float64)                       # one column per (spectrum, part, frequency)
        ctx.forward_columns_dev(first_spectrum + g0, k, rows.data_ptr(), k * rows_per, qc.data_ptr(), view.stream)
        ctx.q_columns_dev(first_spectrum + g0, k, qc.data_ptr(), rows_per, view.stream)
        work = view.empty((nbytes,), torch.uint8)
        res = view.empty((2, k * cols), torch.float64)
        cnt = view.empty((k * cols,), torch.int64)
        _hip.loo_columns_dev(qc.data_ptr(), rows_per, k * cols, M, res[0].data_ptr(), res[1].data_ptr(), 0, cnt.data_ptr(),
                             work.data_ptr(), nbytes, view.stream)
        view.synchronize()
        host = res.cpu().numpy()
        elpd[g0:g0 + k], khat[g0:g0 + k] = host[0].reshape(k, cols), host[1].reshape(k, cols)
        n_tail[g0:g0 + k] = cnt.cpu().numpy().reshape(k, cols)
        del rows, qc, work, res, cnt
    shape = (E, 2, ctx.N)
    return elpd.reshape(shape), khat.reshape(shape), n_tail.reshape(shape)


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelLoo:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are those of ModelFitQuality._fit_sums."""

    def _loo_view(self, chain, kwargs):
        """``(view, ctx)``: the used samples on the device -- the fitted chain where it lies (fit(chain='device')), else an
        upload of ``parse_chain``'s rows, one walker per row: the rows of get_chain(flat=True) in the same order."""
        from .utils import discard_thin
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None and s.n_ensembles == 1:
            return s.used_samples_dev(**discard_thin(kwargs)), s.backend.ctx
        import torch
        from .chainview import ChainView
        flat = np.ascontiguousarray(self.parse_chain(chain, **kwargs), dtype=np.float64)
        ctx = self._context()
        if flat.ndim != 2 or flat.shape[1] != ctx.ndim or flat.shape[0] < 2:
            raise ValueError(f'the chain must be (n, {ctx.ndim}), n >= 2, got {flat.shape}')
        t = torch.from_numpy(flat).to(torch.device('cuda', ctx.device))
        return ChainView(t, flat.shape[0], 1, 1, ctx.ndim), ctx

    def get_loo(self, chain=None, reff=1.0, **kwargs):
        """PSIS-LOO of the fit (bisip_amd.loo): a dict of ``elpd_loo``, ``p_loo``, ``looic = -2 elpd_loo``, its standard error
        ``se``, ``n_bad`` (points whose ``pareto_k`` exceeds ``k_threshold``: their estimate is unreliable) and
        ``k_threshold``, and the pointwise ``elpd_i``, ``p_loo_i``, ``pareto_k`` and ``n_tail``, ``(2, N)`` each.  The columns
        of ``q`` are written, sorted and fitted on the device; ``compare_loo`` ranks the results of several models of one
        spectrum.  ``reff``: the relative efficiency of the chain (it sets the tail's length only).  ``chain`` / ``discard``
        / ``thin`` as get_model_percentile."""
        from .fitquality import device_fit_quality
        tail_length(2, reff)                                        # (refuses a bad reff before anything runs)
        view, ctx = self._loo_view(chain, kwargs)
        elpd_rel, khat, n_tail = (a[0] for a in device_loo(view, ctx, reff))
        lmeh = device_fit_quality(view, ctx)[2][0]
        return loo_from_columns(elpd_rel, khat, n_tail, lmeh, np.log(self._data['zn_err'] ** 2),
                                view.n * view.walkers_per_ensemble)


class BatchLoo:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler, ``ctx`` its context)."""

    def get_loo(self, discard=0, thin=1, reff=1.0):
        """PSIS-LOO of every spectrum's fit (bisip_amd.loo): a dict of ``elpd_loo``, ``p_loo``, ``looic``, ``se``, ``n_bad``,
        ``(E,)`` each, ``k_threshold`` and the pointwise ``elpd_i``, ``p_loo_i``, ``pareto_k``, ``n_tail``, ``(E, 2, N)`` each.
        Under torch.distributed every rank returns its own spectra."""
        from .fitquality import device_fit_quality
        tail_length(2, reff)
        s = self._fitted()
        view, ctx = s.used_samples_dev(discard, thin), s.backend.ctx
        elpd_rel, khat, n_tail = device_loo(view, ctx, reff)
        lmeh = device_fit_quality(view, ctx)[2]
        return loo_from_columns(elpd_rel, khat, n_tail, lmeh, np.log(self.zn_err ** 2), view.n * view.walkers_per_ensemble)
