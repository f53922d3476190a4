"""Does the fitted model reproduce the spectrum within its stated errors at all: posterior predictive checks of a chain.

WAIC, DIC, PSIS-LOO and the evidence rank models against each other; none says whether the best one fits.  The noise
model is Gaussian with known ``sigma``, so the replicated standardised residual ``(y_rep - Z(theta)) / sigma`` is standard
normal whatever ``theta`` is, and every check is the mean over the rows of the chain of a closed-form function of the
row's residuals (Gelman, Meng & Stern 1996; ``pit`` is ArviZ's ``u_value``).  No random numbers: the results are
reproducible.  For a spectrum of N frequencies, n = 2N data points (Re and Im at each), per row of the chain:

* ``d = y - Z``, ``t = d * d``, ``q = t * iv`` (``fitquality.pointwise_q``), ``sd = sqrt(iv)``, ``z = d * sd``;
* ``T = sum q``, the row's chi-square; ``qmax = max q``; ``C``, the number of adjacent frequency pairs, within Re and
  within Im, whose residual changes sign (2N - 2 pairs).

Over the rows: ``pit`` the mean of ``Phi(z)`` per point, the predictive probability ``P(y_rep <= y | y)`` -- near 0 or 1
the measurement lies in the tail of what the model predicts there --, ``chi2_mean`` the mean of T, ``p_chi2`` the mean of
``P(chi2_2N >= T)``, ``p_max`` the mean of ``P(max of n |eps| >= sqrt(qmax))`` -- a single outlying point --, and the
histogram ``sign_changes`` of C, whose ``p_runs`` is the mean of the Binomial(2N - 2, 1/2) distribution function at C:
under the model the sign changes are independent fair coins, and few of them (a small ``p_runs``) mean residuals that run
in bands along the frequency axis: the model misses the spectrum's shape.

* ``normal_cdf``, ``chi2_sf_even``, ``max_abs_sf``, ``sign_changes``, ``binomial_half_cdf``, ``predictive_sums``,
  ``predictive_check``: the definitions, plain NumPy in float64;
* ``ordered_predictive_sums`` restates the order of every sum of ``bisip_predictive_check_dev`` (include/bisip_hip.h) in
  NumPy: the same bits of ``chi2_mean`` and the same counts from the same responses, ``pit``, ``p_chi2`` and ``p_max`` in
  the same order with glibc's functions where the device takes its own;
* ``device_predictive_check`` runs that entry point on a ChainView (bisip_amd.chainview) where the chain lies: the model
  is evaluated in registers, no response and no residual is stored;
* ``ModelPredictive`` and ``BatchPredictive`` are the ``get_predictive_check`` / ``get_pit`` methods of the models
  (bisip_amd.utils.utils) and of SpectraBatch, as mixins.

The rows of a spectrum are numbered ``k * Wp + w`` (sample ``k``, walker ``w``): the order of ``get_chain(flat=True)``.
A row with a parameter that is not finite, or whose T is not finite, counts in no histogram bin and makes ``pit``,
``chi2_mean``, ``p_chi2`` and ``p_max`` of its own spectrum NaN: ``sum(sign_changes)`` is the number of good rows.
"""

import math
import warnings

import numpy as np

from .fitquality import inverse_variance, pointwise_q
from .response import plan, row_pass_workspace

__all__ = ('PIT_EXTREME', 'normal_cdf', 'chi2_sf_even', 'max_abs_sf', 'sign_changes', 'binomial_half_cdf',
           'predictive_sums', 'predictive_check', 'ordered_predictive_sums', 'device_predictive_check', 'ModelPredictive',
           'BatchPredictive')

PIT_EXTREME = 0.025      # a point whose pit lies outside [0.025, 0.975] is in the 5 % tails of its predictive distribution
ROW_N_MAX = 700          # above it exp(-x) underflows with x < N: the device refuses the row outputs

_erfc = np.frompyfunc(math.erfc, 1, 1)
_SQRT2 = math.sqrt(2.0)


def _erfc64(x):
    return np.asarray(_erfc(np.asarray(x, dtype=np.float64)), dtype=np.float64)


# -- the definitions -----------------------------------------------------------------------------------------------------
def normal_cdf(z):
    """``Phi(z) = erfc(-z / sqrt 2) / 2`` of the standard normal distribution: no cancellation in either tail."""
    return 0.5 * _erfc64(-np.asarray(z, dtype=np.float64) / _SQRT2)


def log_factorial(n):
    """``log(n!)``, summed in long double and rounded once: what the host passes to the kernel."""
    return float(np.sum(np.log(np.arange(2, int(n) + 1, dtype=np.longdouble)), dtype=np.longdouble))


def _chi2_sf_even_one(N, x, lgf):
    if x != x:
        return x
    if x < N:
        term = total = math.exp(-x)
        for k in range(1, N):
            term = term * x / k
            total = total + term
    else:
        if x == math.inf:
            return 0.0
        term = total = math.exp(((N - 1) * math.log(x) - x) - lgf)
        for k in range(N - 1, 0, -1):
            term = term * k / x
            total = total + term
    return min(total, 1.0)                      # (the sum of N rounded terms can come out an ulp or so above 1)


def chi2_sf_even(N, x):
    """``Q(N, x)``, the regularised upper incomplete gamma function of an integer ``N >= 1``: ``P(chi2_2N >= 2 x)``, the
    finite sum ``exp(-x) sum_{k < N} x^k / k!`` with every term positive and nothing overflowing.  ``x < N``: ascending
    from ``exp(-x)`` with factors ``x / k``; ``x >= N``: descending from the top term ``exp((N - 1) log x - x -
    log((N - 1)!))`` with factors ``k / x``.  A sum that rounds above 1 is 1."""
    N = int(N)
    if N < 1:
        raise ValueError(f'N must be at least 1, got {N}')
    lgf = log_factorial(N - 1)
    x = np.asarray(x, dtype=np.float64)
    if (x < 0).any():
        raise ValueError('x must not be negative')
    out = np.array([_chi2_sf_even_one(N, float(v), lgf) for v in x.reshape(-1)], dtype=np.float64)
    return out.reshape(x.shape)


def max_abs_sf(n, qmax):
    """``P(max of n |eps| >= sqrt(qmax))`` of independent standard normal ``eps``: ``-expm1(n log1p(-erfc(sqrt(qmax /
    2))))``, accurate where it is near 0 and where it is near 1."""
    qmax = np.asarray(qmax, dtype=np.float64)
    with np.errstate(all='ignore'):
        e = _erfc64(np.sqrt(0.5 * qmax))
        return -np.expm1(float(n) * np.log1p(-e))


def sign_changes(d):
    """``C`` of residuals ``d (..., 2, N)``: the adjacent frequency pairs, within Re and within Im, whose ``d < 0``
    differs -- between 0 and 2N - 2."""
    neg = np.asarray(d, dtype=np.float64) < 0
    if neg.ndim < 2 or neg.shape[-2] != 2:
        raise ValueError(f'expected residuals (..., 2, N), got shape {neg.shape}')
    return (neg[..., 1:] != neg[..., :-1]).sum(axis=(-2, -1)).astype(np.int64)


def binomial_half_cdf(m):
    """``F(c) = P(Binomial(m, 1/2) <= c)`` for c = 0 ... m, ``(m + 1,)``: exact integers from ``math.comb``, one division."""
    m = int(m)
    if m < 0:
        raise ValueError(f'm must not be negative, got {m}')
    total, out = 0, []
    for c in range(m + 1):
        total += math.comb(m, c)
        out.append(total / 2 ** m)              # (an integer ratio: correctly rounded)
    return np.array(out, dtype=np.float64)


def _check_responses(Z, y, iv):
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 3 or Z.shape[1] != 2 or Z.shape[0] < 1:
        raise ValueError(f'expected responses (R, 2, N), R >= 1, got shape {Z.shape}')
    shape = Z.shape[1:]
    return Z, np.broadcast_to(np.asarray(y, dtype=np.float64), shape), np.broadcast_to(np.asarray(iv, dtype=np.float64), shape)


def predictive_sums(Z, y, iv):
    """``(pit (2, N), row (3,), sign_changes (2N - 1,) int64)`` of ONE spectrum's responses ``Z (R, 2, N)`` over its R
    rows, the normalised measurement ``y (2, N)`` and ``iv = inverse_variance(err)``; ``row = (chi2_mean, p_chi2,
    p_max)``.  The rows of a sample whose parameters are not finite must be NaN in ``Z``."""
    Z, y, iv = _check_responses(Z, y, iv)
    R, _, N = Z.shape
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        d = y - Z
        q = pointwise_q(Z, y, iv)
        z = d * np.sqrt(iv)
        T = np.zeros(R)
        for j in range(N):                       # frequencies ascending, Re before Im
            T = (T + q[:, 0, j]) + q[:, 1, j]
        good = np.isfinite(T)
        hist = np.bincount(sign_changes(d)[good], minlength=2 * N - 1).astype(np.int64)
        if not good.all():
            return np.full((2, N), np.nan), np.full(3, np.nan), hist
        pit = np.mean(normal_cdf(z), axis=0)
        row = np.array([np.mean(T), np.mean(chi2_sf_even(N, 0.5 * T)), np.mean(max_abs_sf(2 * N, q.max(axis=(1, 2))))])
    return pit, row, hist


def _check_of_sums(pit, row, hist):
    """The dict of ``predictive_check`` from the three results; leading axes (spectra) stay."""
    pit, row, hist = np.asarray(pit), np.asarray(row), np.asarray(hist)
    N = pit.shape[-1]
    with np.errstate(all='ignore'):
        n_rows = hist.sum(axis=-1)
        p_runs = (hist * binomial_half_cdf(2 * N - 2)).sum(axis=-1) / n_rows
        out = dict(pit=pit, n_extreme=((pit < PIT_EXTREME) | (pit > 1 - PIT_EXTREME)).sum(axis=(-2, -1)),
                   chi2_mean=row[..., 0], chi2_reduced=row[..., 0] / (2 * N), p_chi2=row[..., 1], p_max=row[..., 2],
                   sign_changes=hist, p_runs=p_runs, n_rows=n_rows)
    if row.ndim == 1:
        out.update({k: float(out[k]) for k in ('chi2_mean', 'chi2_reduced', 'p_chi2', 'p_max', 'p_runs')},
                   n_extreme=int(out['n_extreme']), n_rows=int(n_rows))
    return out


def predictive_check(Z, y, err):
    """The posterior predictive checks of ONE spectrum from its responses ``Z (R, 2, N)`` over the R rows of a chain, the
    normalised measurement ``y (2, N)`` and its errors ``err (2, N)``: a dict of

    * ``pit (2, N)``: ``P(y_rep <= y | y)`` of every point, and ``n_extreme``, the points outside [0.025, 0.975];
    * ``chi2_mean``, the posterior mean of the chi-square ``T``, and ``chi2_reduced = chi2_mean / 2N`` (near 1: fitted to
      the error bars);
    * ``p_chi2``: ``P(T(y_rep) >= T(y) | y)``, small when the misfit is larger than the errors allow;
    * ``p_max``: the same for the largest standardised residual: small when a single point lies far out;
    * ``sign_changes (2N - 1,)``, the histogram of the sign changes along the frequency axis, and ``p_runs``, the mean
      Binomial(2N - 2, 1/2) probability of no more changes than seen: small when the residuals run in bands;
    * ``n_rows``, the rows that counted."""
    return _check_of_sums(*predictive_sums(Z, y, inverse_variance(err)))


# -- the device's order of summation ------------------------------------------------------------------------------------
def _tree_mean(x, seg_rows, nseg, slots):
    """The mean over axis 1 of ``x (E, R, K)`` in the device's order: row i of a segment to slot i mod ``slots``, a slot's
    rows ascending from 0.0; slots pairwise within runs of 64, 32 ... 1 apart; the runs ascending; segments ascending."""
    E, R, K = x.shape
    total = None
    for g in range(nseg):
        r0, r1 = g * seg_rows, min(R, (g + 1) * seg_rows)
        S = np.zeros((E, slots, K))
        for t0 in range(r0, r1, slots):
            rows = x[:, t0:min(r1, t0 + slots)]
            k = rows.shape[1]
            S[:, :k] = S[:, :k] + rows
        S = S.reshape(E, slots // 64, 64, K)
        w = 32
        while w >= 1:
            S = S[:, :, :w] + S[:, :, w:2 * w]
            w //= 2
        seg = S[:, 0, 0]
        for v in range(1, slots // 64):
            seg = seg + S[:, v, 0]
        total = seg if g == 0 else total + seg
    return total / float(R)


def ordered_predictive_sums(Z, y, iv, n_spectra=None):
    """``(pit (E, 2, N), row (E, 3), sign_changes (E, 2N - 1))`` of the responses ``Z (E, R, 2, N)`` of the R rows of E
    spectra -- ``(R, 2, N)``: one spectrum -- with the measurement ``y`` and the inverse variance ``iv``, ``(E, 2, N)`` or
    ``(2, N)``, in the order include/bisip_hip.h states for bisip_predictive_check_dev: ``q`` in three roundings, ``T``
    over the frequencies ascending, Re before Im; ``h = sqrt(iv / 2)``, ``a = d * h``, ``Phi = erfc(-a) / 2``; plain sums
    from 0.0, row ``i`` of a segment to slot ``i mod 256``, a slot's rows in ascending order, slots pairwise within runs
    of 64, the four runs and then the segments in ascending order, divided by R.  ``row[:, 0]`` (chi2_mean) and the
    counts have the device's bits; ``pit``, ``p_chi2`` and ``p_max`` take glibc's functions where the device takes its
    own: the same order, not necessarily the same bits.  ``n_spectra``: the spectra of the call when ``Z`` holds only some
    of them (the plan depends on it).  The rows of a sample whose parameters are not finite must be NaN in ``Z``."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 3:
        Z = Z[None]
    if Z.ndim != 4 or Z.shape[2] != 2:
        raise ValueError(f'expected responses (E, R, 2, N) or (R, 2, N), got shape {Z.shape}')
    E, R, _, N = Z.shape
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), (E, 2, N))
    iv = np.broadcast_to(np.asarray(iv, dtype=np.float64), (E, 2, N))
    seg_rows, nseg, slots = plan(R, E if n_spectra is None else n_spectra, 1)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        d = y[:, None] - Z
        q = pointwise_q(Z, y[:, None], iv[:, None])
        T = np.zeros((E, R))
        for j in range(N):
            T = (T + q[:, :, 0, j]) + q[:, :, 1, j]
        good = np.isfinite(T)
        qmax = np.fmax.reduce(q.reshape(E, R, 2 * N), axis=2, initial=0.0)
        C = sign_changes(d)
        hist = np.stack([np.bincount(C[e][good[e]], minlength=2 * N - 1) for e in range(E)]).astype(np.int64)
        Q = np.stack([chi2_sf_even(N, np.where(good[e], 0.5 * T[e], 0.0)) for e in range(E)])
        pm = max_abs_sf(2 * N, qmax)
        terms = np.where(good[..., None], np.stack([T, Q, pm], axis=-1), np.nan)
        row = _tree_mean(terms, seg_rows, nseg, slots)
        a = d * np.sqrt(0.5 * iv)[:, None]
        pit = _tree_mean((0.5 * _erfc64(-a)).reshape(E, R, 2 * N), seg_rows, nseg, slots).reshape(E, 2, N)
        bad = ~good.all(axis=1)
        pit[bad] = np.nan
        row[bad] = np.nan
    return pit, row, hist


def device_predictive_check(view, ctx, first_spectrum=0):
    """``(pit (n_ensembles, 2, N), row (n_ensembles, 3), sign_changes (n_ensembles, 2N - 1) int64)`` of the model of
    ``ctx`` (a HipContext) against its data over every ensemble's samples of a ChainView (NumPy), taken where the chain
    lies (bisip_predictive_check_dev); ``row`` holds chi2_mean, p_chi2 and p_max.  Ensemble ``e`` of the view is spectrum
    ``first_spectrum + e`` of the context."""
    import torch
    n, E, Wp, work, nbytes = row_pass_workspace(view, ctx, ctx.predictive_check_workspace)      # (never 0 bytes)
    N = ctx.N
    pit = view.empty((E, 2, N), torch.float64)
    row = view.empty((E, 3), torch.float64)
    hist = view.empty((E, 2 * N - 1), torch.int64)
    ctx.predictive_check_dev(first_spectrum, E, view.ptr, n, view.stride, Wp, pit.data_ptr(), row.data_ptr(),
                             hist.data_ptr(), work.data_ptr(), nbytes, view.stream)
    view.synchronize()
    return pit.cpu().numpy(), row.cpu().numpy(), hist.cpu().numpy()


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelPredictive:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are get_waic's."""

    def _predictive_sums(self, chain, kwargs):
        from .utils import discard_thin
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None and s.n_ensembles == 1:      # fit(chain='device'): reduced where the chain lies
            return tuple(a[0] for a in s.predictive_check(**discard_thin(kwargs)))
        from .chainview import host_chain_view
        flat, ctx = self.parse_chain(chain, **kwargs), self._context()
        return tuple(a[0] for a in device_predictive_check(host_chain_view(flat, ctx), ctx))

    def get_predictive_check(self, chain=None, **kwargs):
        """The posterior predictive checks of the fit (bisip_amd.predictive.predictive_check): a dict of ``pit (2, N)``,
        ``n_extreme``, ``chi2_mean``, ``chi2_reduced``, ``p_chi2``, ``p_max``, ``sign_changes (2N - 1,)``, ``p_runs`` and
        ``n_rows``.  ``chi2_reduced`` near 1 and no probability near 0: the model reproduces the spectrum within its
        errors; a small ``p_runs``: the residuals run in bands along the frequency axis (a mode is missing); a small
        ``p_max``: one point lies far out.  Evaluated and summed on the device in one call over the chain, no response
        stored (bisip_predictive_check_dev).  ``chain`` / ``discard`` / ``thin`` as get_waic."""
        return _check_of_sums(*self._predictive_sums(chain, kwargs))

    def get_pit(self, chain=None, **kwargs):
        """The posterior predictive probability ``P(y_rep <= y | y)`` of every data point, ``(2, N)`` (Re, Im): the
        ``pit`` of get_predictive_check.  ``chain`` / ``discard`` / ``thin`` as get_waic."""
        return self._predictive_sums(chain, kwargs)[0]


class BatchPredictive:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler)."""

    def get_predictive_check(self, discard=0, thin=1):
        """The posterior predictive checks of every spectrum's fit (bisip_amd.predictive.predictive_check): the dict of
        the models' get_predictive_check, every entry with a leading ``E``.  One call over the chain where it lies
        (bisip_predictive_check_dev), for ``chain='device'`` and ``'host'`` alike.  Under torch.distributed every rank
        returns its own spectra."""
        return _check_of_sums(*self._fitted().predictive_check(discard=discard, thin=thin))

    def get_pit(self, discard=0, thin=1):
        """``P(y_rep <= y | y)`` of every data point of every spectrum, ``(E, 2, N)``."""
        return self._fitted().predictive_check(discard=discard, thin=thin)[0]
