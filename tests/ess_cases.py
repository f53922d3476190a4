"""What tests/test_ess.py and tests/test_gpu_ess.py share: the generators of the chains, the covering set of shapes, the
definition's values with their decision margins, and the comparisons.

The device takes its sums in another order than NumPy, so its values differ from the definition's in the last bits.  Two
of the estimator's steps are comparisons: Geyer's sequence goes on while ``even + odd > 0`` and ends with ``even > 0``.  A
chain that meets one of them within rounding of zero has no single right answer, so every case here is held to a margin:
``ess_of_chains(margins=True)`` reports the smallest ``|even + odd|`` and ``|even|`` met at a decision, and both must stay
above ``MARGIN``.  That is a condition on the inputs: test_ess.py checks it without a GPU for every generated case.
"""
import functools

import numpy as np

from bisip_amd import ess as es

ESS_RTOL = 1e-10      # |got - want| <= ESS_RTOL * max(1, |want|) against the NumPy definition
Z_RTOL = 1e-14        # the same form, for z: one rank off by one moves z by more than 2 / N
MARGIN = 1e-9

# (E, Wp, ndim, n, discard, thin): E in {1, 3, 64}, Wp in {1, 2, 31, 256, 300}, ndim in {1, 7, 16}, n in {4, 5, 7, 64, 65, 1000,
# 2001}.  Wp = 300: more than one group of 256 chains, no multiple of the tile; n = 4: halves of 2; n = 5, 7, 65, 2001:
# odd, the middle sample dropped; (64, 31, 7): 217 tiles of 64 series that straddle (ensemble, parameter) pairs; n = 2001
# with 4800 columns: rounds of 256 (split) and 448 (unsplit) lags, which rho = 0.99 outruns while rho = 0 stops at lag 1.
COVER = [(1, 2, 1, 4, 0, 1), (3, 1, 7, 5, 1, 2), (64, 1, 16, 7, 0, 1), (1, 31, 16, 7, 2, 1), (3, 2, 7, 64, 5, 3),
         (64, 31, 7, 64, 0, 1), (3, 300, 7, 65, 1, 2), (1, 256, 7, 1000, 0, 1), (64, 2, 1, 1000, 3, 1),
         (1, 300, 16, 2001, 0, 1)]
THRESHOLD_COVER = [(3, 2, 7, 64, 5, 3), (3, 300, 7, 65, 1, 2), (1, 256, 7, 1000, 0, 1)]
PAD = 3               # doubles between the samples of a stored chain that nothing may read


def cover_id(case):
    return 'x'.join(map(str, case))


def ar1(rng, n, W, rho, ties=True):
    """AR(1) chains ``(n, W, len(rho))`` of unit innovations with per-parameter rho, scale (0.1 ... 10) and offset (-5 ...
    5).  ``ties``: parameter 1 (parameter 0 of a single one when W is even) is rounded to one decimal first, so that equal
    values are everywhere, as in the chain of a sampler that rejects."""
    rho = np.asarray(rho, dtype=np.float64)
    ndim = rho.size
    x = np.empty((n, W, ndim))
    x[0] = rng.standard_normal((W, ndim)) / np.sqrt(1.0 - rho ** 2)
    e = rng.standard_normal((n, W, ndim))
    for t in range(1, n):
        x[t] = rho * x[t - 1] + e[t]
    if ties:
        q = 1 if ndim > 1 else 0
        if ndim > 1 or W % 2 == 0:
            x[:, :, q] = np.round(x[:, :, q], 1)
    return x * rng.uniform(0.1, 10.0, ndim) + rng.uniform(-5.0, 5.0, ndim)


@functools.lru_cache(maxsize=None)
def cover_case(E, Wp, ndim, n, discard, thin):
    """``(stored (discard + n * thin, E * Wp * ndim + PAD), used (n, E * Wp, ndim))``: AR(1) with rho from 0 to 0.99 across
    the parameters; the used samples are read through an offset and a stride, what lies between them is NaN."""
    rng = np.random.default_rng(E * 100003 + Wp * 1009 + ndim * 101 + n)
    used = ar1(rng, n, E * Wp, np.linspace(0.0, 0.99, ndim))
    row = E * Wp * ndim
    stored = np.full((discard + n * thin, row + PAD), np.nan)
    stored[discard + thin - 1::thin, :row] = used.reshape(n, row)
    assert stored[discard + thin - 1::thin].shape[0] == n
    used.setflags(write=False)
    stored.setflags(write=False)
    return stored, used


def chains_of(x, split):
    """The chains ``(L, M, ndim)`` of one ensemble's ``x (n, Wp, ndim)``."""
    return es._chains(x, split)


def definition_of_series(series, E, split):
    """``(ess, smallest |even + odd|, smallest |even|, last lag taken)``, ``(E, ndim)`` each, of the series ``(n, E * Wp,
    ndim)`` by ess_of_chains per (ensemble, parameter)."""
    n, W, ndim = series.shape
    Wp = W // E
    out = np.empty((4, E, ndim))
    for e in range(E):
        c = chains_of(series[:, e * Wp:(e + 1) * Wp], split)
        for d in range(ndim):
            out[:, e, d] = es.ess_of_chains(c[:, :, d], margins=True)
    return out[0], out[1], out[2], out[3]


def definition(x, E, kind, split):
    """The definition's ``kind`` of ESS of every (ensemble, parameter) of ``x (n, E * Wp, ndim)`` with its margins (of
    'tail': the smaller ESS, the smaller margins of the two indicators); NaN where ``ess.ess`` gives NaN."""
    n, W, ndim = x.shape
    Wp = W // E
    if kind == 'mean':
        return definition_of_series(x, E, split)
    if kind == 'bulk':
        z = np.concatenate([es.z_scale(x[:, e * Wp:(e + 1) * Wp]) for e in range(E)], axis=1)
        return definition_of_series(z, E, split)
    grid = x.reshape(n, E, Wp, ndim)
    finite = np.isfinite(grid).all(axis=(0, 2))
    with np.errstate(all='ignore'):
        q = np.percentile(grid.transpose(1, 0, 2, 3).reshape(E, n * Wp, ndim), es.TAIL_PERCENTILES, axis=1)     # (2, E, ndim)
    both = [definition_thresholded(x, E, q[k], split) for k in range(2)]
    with np.errstate(invalid='ignore'):
        val = np.where(finite, np.minimum(both[0][0], both[1][0]), np.nan)
    return val, np.minimum(both[0][1], both[1][1]), np.minimum(both[0][2], both[1][2]), np.maximum(both[0][3], both[1][3])


def definition_thresholded(x, E, thr, split):
    """The same of the indicators ``x <= thr`` for thresholds ``(E, ndim)``; a NaN threshold gives NaN."""
    n, W, ndim = x.shape
    Wp = W // E
    with np.errstate(invalid='ignore'):
        ind = (x.reshape(n, E, Wp, ndim) <= thr[None, :, None, :]).astype(np.float64).reshape(n, W, ndim)
    val, gs, ge, lags = definition_of_series(ind, E, split)
    nan = np.isnan(thr)
    return np.where(nan, np.nan, val), np.where(nan, np.inf, gs), np.where(nan, np.inf, ge), lags


@functools.lru_cache(maxsize=None)
def cover_reference(case, kind, split):
    """``definition`` of a COVER case, computed once per session."""
    return definition(cover_case(*case)[1], case[0], kind, split)


def cover_thresholds(case):
    """``(4, E, ndim)``: the 5th and 95th percentile of every (ensemble, parameter), then a threshold below every sample
    and one above every sample (constant indicators: S), with a NaN planted in the first and the last row."""
    E, Wp, ndim, n = case[:4]
    x = cover_case(*case)[1].reshape(n, E, Wp, ndim)
    flat = x.transpose(1, 0, 2, 3).reshape(E, n * Wp, ndim)
    thr = np.stack([np.percentile(flat, 5, axis=1), np.percentile(flat, 95, axis=1), flat.min(axis=1) - 1.0,
                    flat.max(axis=1) + 1.0])
    thr[0, E - 1, ndim - 1] = np.nan
    thr[3, 0, 0] = np.nan
    return thr


@functools.lru_cache(maxsize=None)
def cover_threshold_reference(case, split):
    thr = cover_thresholds(case)
    x = cover_case(*case)[1]
    parts = [definition_thresholded(x, case[0], thr[k], split) for k in range(thr.shape[0])]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))


def hand_built(n=65, E=3, Wp=6, ndim=4, seed=2):
    """A chain ``(n, E * Wp, ndim)`` (n odd) of moderately correlated walkers with: a constant walker among moving ones
    (ensemble 0, parameter 0); a constant parameter (ensemble E - 1, parameter ndim - 1: S); duplicated values (ensemble 0,
    walker 0, parameter 0: every odd sample repeats the one before); NaN in (0, 1), +inf in (1, 2), -inf in (2, 1), and a
    NaN in the MIDDLE sample of (1, 3), which belongs to neither half: 'mean' does not see it, 'bulk' and 'tail' rank it.
    Returns ``(chain, nan_all (E, ndim) bool, nan_ranked (E, ndim) bool)``."""
    assert n % 2 == 1 and E >= 3 and ndim >= 4 and Wp >= 3
    rng = np.random.default_rng(seed)
    x = ar1(rng, n, E * Wp, np.linspace(0.2, 0.8, ndim), ties=False).reshape(n, E, Wp, ndim)
    x[:, 0, Wp - 1, 0] = 0.25
    x[1::2, 0, 0, 0] = x[0:n - 1:2, 0, 0, 0]
    x[:, E - 1, :, ndim - 1] = 0.25
    x[3, 0, 1, 1] = np.nan
    x[n - 2, 1, 2, 2] = np.inf
    x[7, 2, 0, 1] = -np.inf
    x[n // 2, 1, 1, 3] = np.nan
    nan_all = np.zeros((E, ndim), dtype=bool)
    nan_all[0, 1] = nan_all[1, 2] = nan_all[2, 1] = True
    nan_ranked = nan_all.copy()
    nan_ranked[1, 3] = True
    return x.reshape(n, E * Wp, ndim), nan_all, nan_ranked


def assert_margins(gap_sum, gap_even, what=''):
    """The condition on the inputs: no decision of the sequence within MARGIN of zero (inf: no decision was made)."""
    gs, ge = np.asarray(gap_sum), np.asarray(gap_even)
    assert np.nanmin(gs) > MARGIN and np.nanmin(ge) > MARGIN, (what, float(np.nanmin(gs)), float(np.nanmin(ge)))


def assert_close(got, want, rtol=ESS_RTOL, what=''):
    """NaN exactly where the definition has it; elsewhere ``|got - want| <= rtol * max(1, |want|)``.  Returns the largest
    error in units of the tolerance."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN where the definition has it')
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print(f'{what}: largest error {err.max():.3e} of {rtol:g}')
    assert err.max() <= rtol, (what, float(err.max()))
    return float(err.max() / rtol)
