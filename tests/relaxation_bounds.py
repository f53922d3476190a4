"""The yardstick and the error bound of the relaxation descriptors (bisip_amd.decomposition, "Relaxation descriptors":
the RTD's peak and the cumulative relaxation times log_tau_q), shared by tests/test_relaxation.py and
tests/test_gpu_relaxation.py.

The yardstick is that definition in long double on the long-double m_l of tests/test_decomposition.py's ``yardstick``.
Hatted values are the float64 ones, u = 2**-53, ul = 2**-64; ``bm_l`` is the Horner bound of m_l that
tests/test_decomposition.py's ``bounds`` gives (it covers the Horner of NumPy, two roundings a step, and the fma one).

The bound of log_tau_q, for a row whose crossing index k is the yardstick's:
  * clipping is 1-Lipschitz: |c^_l - c_l| <= bm_l;
  * g^_k is a sequential sum of L or fewer non-negative terms: |g^_k - g_k| <= eg_k = sum_{l<=k} bm_l + L u total
    (+ L ul total for the yardstick's own sum); g_{-1} = 0 is exact;
  * t^ = fl(q total^): |t^ - t| <= et = q eg_{L-1} + u t -- t inherits the error of the whole sum, not only of the sum
    to k;
  * the numerator n = t - g_{k-1}: |n^ - n| <= en = et + eg_{k-1} + u n;
  * f = n / c_k in [0, 1]: f^ - f = (n^ - n) / c^_k - f (c^_k - c_k) / c^_k, so |f^ - f| <= (en + f bm_k) / (c_k - bm_k),
    plus u f^ of the division;
  * the value x_{k-1} + f h, h = x_k - x_{k-1} <= 2 max|x|: the roundings of the division, of h, of the product (NumPy
    has no fma) and of the sum are each at most 2 u max|x|: 8 u max|x| together.
  bound = h (en + f bm_k) / (c_k - bm_k) + 8 u max|x|; infinite where c_k <= bm_k; 0 for k = 0 (the value is x_0 itself).
m_peak is held to bm_l at the peak; log_tau_peak to equality.

A (row, j) is FRAGILE, and left out of the comparison of values, if a margin cannot tell the index -- t - g_{k-1} <=
et + eg_{k-1} or g_k - t <= et + eg_k -- or if the bound exceeds BOUND_CAP = 1e-9; the two peak outputs of a row are
fragile if its two largest m_l are closer than the sum of their bounds.  A fragile entry must still be finite and, a
relaxation time, lie inside [x_0, x_{L-1}].  At most FRAGILE_CAP = 1 % of a family's entries may be fragile.  (With
q = 1 the upper margin is 0 by definition: such fractions are compared bit for bit elsewhere, not against this bound.)
"""

import numpy as np

from test_decomposition import U, bounds, yardstick

UL = 2.0 ** -64
BOUND_CAP = 1e-9
FRAGILE_CAP = 0.01


def descriptors_yardstick(theta, log_tau, q):
    """The definition in long double for rows ``theta`` (n, ndim): a dict of ``values`` (n, 2 + J) (NaN for a row with no
    positive RTD), ``valid`` (n,), ``peak`` (n,), per (row, j) the crossing ``index``, ``share`` = c_k / total and the
    margins ``lo`` = t - g_{k-1}, ``hi`` = g_k - t, and the long-double ``m``, ``c``, ``g``, ``total``."""
    th = np.asarray(theta, dtype=np.float64)
    x = np.asarray(log_tau, dtype=np.float64).astype(np.longdouble)
    ql = np.atleast_1d(np.asarray(q, dtype=np.float64)).astype(np.longdouble)
    n, L, J = th.shape[0], x.size, ql.size
    rows = np.arange(n)
    m = yardstick(th, log_tau, 1.0)[0]
    c = np.where(m > 0, m, np.longdouble(0))
    g = np.cumsum(c, axis=1)
    total = g[:, -1]
    valid = np.isfinite(total) & (total > 0)
    peak = np.argmax(m, axis=1)                          # the first of the largest
    values = np.empty((n, 2 + J), dtype=np.longdouble)
    values[:, 0], values[:, 1] = x[peak], m[rows, peak]
    index = np.empty((n, J), dtype=np.int64)
    share, lo, hi = (np.empty((n, J), dtype=np.longdouble) for _ in range(3))
    with np.errstate(all='ignore'):
        for j in range(J):
            t = ql[j] * total
            k = np.argmax(g >= t[:, None], axis=1)
            k1 = np.minimum(np.maximum(k, 1), L - 1)
            below = np.where(k == 0, np.longdouble(0), g[rows, k1 - 1])
            index[:, j], share[:, j] = k, c[rows, k] / total
            lo[:, j], hi[:, j] = t - below, g[rows, k] - t
            f = lo[:, j] / c[rows, k]
            values[:, 2 + j] = np.where(k == 0, x[0], x[k1 - 1] + f * (x[k1] - x[k1 - 1]))
    values[~valid] = np.nan
    return dict(values=values, valid=valid, peak=peak, index=index, share=share, lo=lo, hi=hi, m=m, c=c, g=g, total=total)


def descriptor_bounds(theta, log_tau, q, ys):
    """``(bound, fragile)``, (n, 2 + J) each, of the yardstick ``ys`` of the same arguments, as the module docstring
    derives them.  Rows that are not valid have no entries: bound 0, not fragile."""
    th = np.asarray(theta, dtype=np.float64)
    x = np.asarray(log_tau, dtype=np.float64).astype(np.longdouble)
    ql = np.atleast_1d(np.asarray(q, dtype=np.float64)).astype(np.longdouble)
    n, L, J = th.shape[0], x.size, ql.size
    rows = np.arange(n)
    bm = bounds(th, log_tau, 1.0)[1]                     # (n, L)
    m, c, g, total = ys['m'], ys['c'], ys['g'], ys['total']
    eg = np.cumsum(bm, axis=1) + (L * (U + UL) * total)[:, None]
    xmax = np.max(np.abs(x))
    bound = np.zeros((n, 2 + J), dtype=np.longdouble)
    fragile = np.zeros((n, 2 + J), dtype=bool)
    # the peak: is the largest m_l the largest beyond the two bounds?
    peak = ys['peak']
    if L > 1:
        rest = m.copy()
        rest[rows, peak] = -np.inf
        second = np.argmax(rest, axis=1)
        ambiguous = m[rows, peak] - m[rows, second] <= bm[rows, peak] + bm[rows, second]
        fragile[:, 0] = fragile[:, 1] = ambiguous
    bound[:, 1] = np.where(fragile[:, 1], bm.max(axis=1), bm[rows, peak])
    with np.errstate(all='ignore'):
        for j in range(J):
            k, lo, hi = ys['index'][:, j], ys['lo'][:, j], ys['hi'][:, j]
            k1 = np.minimum(np.maximum(k, 1), L - 1)
            t = ql[j] * total
            et = ql[j] * eg[:, -1] + U * t
            eg_below = np.where(k == 0, np.longdouble(0), eg[rows, k1 - 1])
            en = et + eg_below + U * lo
            ck, bmk = c[rows, k], bm[rows, k]
            h = x[k1] - x[k1 - 1]
            b = np.where(ck > bmk, h * (en + (lo / ck) * bmk) / (ck - bmk) + 8 * U * xmax, np.inf)
            bound[:, 2 + j] = np.where(k == 0, np.longdouble(0), b)
            fragile[:, 2 + j] = (lo <= et + eg_below) | (hi <= et + eg[rows, k]) | (bound[:, 2 + j] > BOUND_CAP)
    bound[~ys['valid']] = 0
    fragile[~ys['valid']] = False
    return bound, fragile


def assert_descriptors_within(got, ys, bound, fragile, log_tau, what=''):
    """The NaN pattern is the yardstick's; entries that are not fragile are within their bound; fragile ones are finite
    and, relaxation times, inside the grid; at most FRAGILE_CAP of the entries are fragile.  Returns (worst error,
    fragile share)."""
    got = np.asarray(got, dtype=np.float64)
    valid = ys['valid']
    assert got.shape == bound.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.broadcast_to(~valid[:, None], got.shape), err_msg=what)
    entries = np.broadcast_to(valid[:, None], got.shape)
    held = entries & ~fragile
    err = np.abs(got.astype(np.longdouble)[held] - ys['values'][held])
    assert np.all(err <= bound[held]), (what, float(np.max(err - bound[held])))
    assert np.all(np.isfinite(got[fragile])), what
    times = np.ones(got.shape[1], dtype=bool)
    times[1] = False                                     # m_peak is no relaxation time
    inside = got[:, times][entries[:, times]]
    assert np.all((inside >= log_tau[0]) & (inside <= log_tau[-1])), what
    share = fragile.sum() / max(1, entries.sum())
    assert share <= FRAGILE_CAP, (what, share)
    return (float(err.max()) if err.size else 0.0), float(share)
