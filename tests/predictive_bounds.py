"""What tests/test_predictive.py and tests/test_gpu_predictive.py share: the yardstick of the posterior predictive checks of
bisip_amd.predictive (per spectrum over the R rows of a chain: pit, the mean of Phi per data point; chi2_mean, p_chi2 and
p_max, the means of T, Q(N, T / 2) and P(max of 2N |eps| >= sqrt(qmax)) over the rows) and first-order error bounds of
bisip_predictive_check_dev's way of computing them in any summation order.  u = 2^-53.  The responses Z, the measurement y
and the inverse variance iv are doubles and ARE the data; the yardstick evaluates everything from them in long double,
erfc excepted: NumPy has none in long double, so erfc(a) of a long-double a is math.erfc (glibc) at the nearest double a0
plus the first-order term -(a - a0) (2 / sqrt pi) exp(-a0^2) (the next term is of order u^2): no rounding of the
argument, and glibc's own error, which tests/test_predictive.py measures against mpmath at 50 digits on 10,000 arguments
of Phi in [-40, 40] (worst seen 2.7 u relative, where erfc is a normal number) and holds below ERFC_GLIBC = 3.

Ulps of the device library: the HIP math documentation installed with this ROCm states none for double precision, so
OpenCL full profile's (OpenCL C specification, "Relative error as ULPs": exp 3, log 3, log1p 2, expm1 3, erfc 16; sqrt
correctly rounded), counted as tests/fit_quality_bounds.py counts them -- a term K u |x|, K the table's number plus the
yardstick's own.  A result below the smallest normal number has no relative bound: every bound carries TINY = 2^-1073.

q, T.  d = y - Z, t = d d, q = t iv, each rounded on its own: q~ = q (1 + e), |e| <= KQ u, KQ = 4 (fit_quality_bounds).  T is
a sum of 2N terms >= 0 in 2N - 1 additions: T~ = T (1 + e), |e| <= ET = (KQ + 2N - 1) u; qmax~ = qmax (1 + e), |e| <= KQ u.

Sums over the rows.  Every term is >= 0, so a sum of R terms in ANY order (slots, runs, segments) has a relative error of
at most (R - 1) u, and the division by R adds u: R u of the mean, next to the mean of the terms' own absolute errors.

pit, absolute.  A term is Phi = erfc(-a) / 2 (the halving is exact), a = d h the standardised residual over sqrt 2 with
h = sqrt(iv / 2) correctly rounded: three roundings of the argument (d, h, the product), K_ARG = 3.  A relative change e of
a moves Phi by phi(z) |z| e, phi the standard normal density and z = a sqrt 2.  erfc: K_erfc u Phi.
  dpit = u [(R + K_erfc) mean(Phi) + K_ARG mean(phi(z) |z|)] + TINY.
(The NumPy DEFINITION, predictive.normal_cdf(d * sqrt(iv)), rounds d, sqrt(iv), the product and the quotient by a rounded
sqrt 2: K_ARG_DEFINITION = 5.)

p_chi2.  Q(N, x) = exp(-x) sum_{k < N} x^k / k!, x = T / 2 (exact), all terms positive: relative errors of terms bound
that of Q.  dQ / dx = -top, top = exp(-x) x^(N - 1) / (N - 1)! the last term, so the error of T moves Q by top x ET.
  * x < N, ascending: exp(-x): K_exp u; term k carries 2 k roundings (product, quotient), the sum N - 1 more: at most
    (K_exp + 3 (N - 1)) u.
  * x >= N, descending from exp(E), E = ((N - 1) log x - x) - lgf: log x: K_log u |log x|, times N - 1 and rounded:
    (K_log + 1) (N - 1) |log x| u; the two differences, each u of its result, at most u ((N - 1) |log x| + x) and
    u ((N - 1) |log x| + x + lgf); lgf itself, rounded once from long double: u lgf.  An absolute error of E is a relative
    one of every term: ((K_log + 3) (N - 1) |log x| + 2 x + 2 lgf) u; then K_exp u and 3 (N - 1) u as above.
  The yardstick takes the same sums in long double: 2^-11 of the same expression, added.
  dp_chi2 = mean(Q rel + top x ET) + R u mean(Q) + TINY.

p_max = -expm1(n log1p(-erfc(s))), s = sqrt(qmax / 2), n = 2N: the four calls in turn, absolute errors.
  s:  relative KQ u / 2 + u = 3 u
  e = erfc(s):        de = K_erfc u e + (2 / sqrt pi) exp(-s^2) s 3 u
  l = log1p(-e):      dl = K_log1p u |l| + de / (1 - e)
  m = n l:            dm = n dl + u |m|
  p = -expm1(m):      dp = K_expm1 u p + exp(m) dm            (exp(m) = 0, qmax = 0 included: dp = K_expm1 u p)
  dp_max = mean(dp) + R u mean(p) + TINY.
chi2_mean: dchi2_mean = (ET + R u) mean(T).
Every term is first order in u; the quantities on the right come from the long-double evaluation.
"""
import math

import numpy as np

from convergence_bounds import LD, U
from covariance_bounds import assert_within      # noqa: F401  (shared with the tests)
from fit_quality_bounds import KQ, inverse_variance      # noqa: F401

ERFC_GLIBC = 3                                   # u, relative: math.erfc against mpmath (tests/test_predictive.py)
GLIBC_ULP = 1                                    # expl, logl, log1pl, expm1l of the yardstick (fit_quality_bounds)
TINY = LD(2.0) ** -1073
K_ARG, K_ARG_DEFINITION = 3, 5
# K of exp, log, log1p, expm1, erfc
K_DEVICE = dict(exp=3 + GLIBC_ULP, log=3 + GLIBC_ULP, log1p=2 + GLIBC_ULP, expm1=3 + GLIBC_ULP, erfc=16 + ERFC_GLIBC)
# NumPy's and math's (glibc) in ordered_predictive_sums and in the definitions: within 1 ulp <= 2 u |x| each; math.erfc
# as measured
K_NUMPY = dict(exp=2 + GLIBC_ULP, log=2 + GLIBC_ULP, log1p=2 + GLIBC_ULP, expm1=2 + GLIBC_ULP, erfc=2 * ERFC_GLIBC)

_erfc = np.frompyfunc(math.erfc, 1, 1)
_TWO_OVER_SQRT_PI = LD(2) / np.sqrt(LD(math.pi) + LD(1.2246467991473532e-16))     # (pi to long double)
_SQRT2 = np.sqrt(LD(2))


def erfc_ld(a):
    """erfc of a long-double array: glibc's at the nearest double plus the first-order term of the remainder."""
    a = np.asarray(a, dtype=LD)
    a0 = a.astype(np.float64)
    with np.errstate(all='ignore'):
        e = np.asarray(_erfc(a0), dtype=np.float64).astype(LD)
        rest = np.where(np.isfinite(a0), a - a0.astype(LD), LD(0))
        return e - rest * _TWO_OVER_SQRT_PI * np.exp(-(a0.astype(LD) ** 2))


def log_factorial_ld(n):
    return np.sum(np.log(np.arange(2, n + 1, dtype=LD)), dtype=LD) if n >= 2 else LD(0)


def chi2_sf_ld(N, x):
    """(Q(N, x), top term) in long double for an array x >= 0, by the definition's two branches."""
    x = np.asarray(x, dtype=LD)
    lgf = log_factorial_ld(N - 1)
    with np.errstate(all='ignore'):
        up = x < N
        xa = np.where(up, x, LD(0))
        term = np.exp(-xa)
        asc = term.copy()
        for k in range(1, N):
            term = term * xa / k
            asc = asc + term
        top_a = term
        xd = np.where(up, LD(N), x)
        top_d = np.exp(((N - 1) * np.log(xd) - xd) - lgf)
        term = top_d.copy()
        desc = term.copy()
        for k in range(N - 1, 0, -1):
            term = term * k / xd
            desc = desc + term
    return np.where(up, asc, desc), np.where(up, top_a, top_d)


def chi2_sf_rel_bound(N, x, K):
    """The relative bound above of Q(N, x) computed in double from a double x (long-double array), the yardstick's included."""
    with np.errstate(all='ignore'):
        lgf = log_factorial_ld(N - 1)
        lx = np.abs(np.log(np.where(x > 0, x, LD(1))))
        rel = np.where(x < N, LD(K['exp'] + 3 * (N - 1)),
                       K['exp'] + 3 * (N - 1) + (K['log'] + 3) * (N - 1) * lx + 2 * x + 2 * lgf) * U
        return rel * (1 + LD(2.0) ** -11)


def max_abs_sf_ld(n, qm, K, s_u):
    """(p, dp): -expm1(n log1p(-erfc(sqrt(qm / 2)))) in long double and its bound above; s_u: the relative error of the
    square root in u (KQ / 2 + 1 from a device q, 1 from an exact one)."""
    with np.errstate(all='ignore'):
        qm = np.asarray(qm, dtype=LD)
        s = np.sqrt(qm / 2)
        e = erfc_ld(s)
        de = K['erfc'] * U * e + _TWO_OVER_SQRT_PI * np.exp(-s * s) * s * s_u * U
        el = np.log1p(-e)
        dl = K['log1p'] * U * np.abs(el) + de / (1 - e)
        m = n * el
        dm = n * dl + U * np.abs(m)
        p = -np.expm1(m)
        em = np.exp(m)
        return p, K['expm1'] * U * p + np.where(em > 0, em * dm, LD(0))


def reference_and_bounds(Z, y, iv, K=K_DEVICE, k_arg=K_ARG):
    """The long-double yardstick of the responses Z (E, R, 2, N) with y, iv (E, 2, N) or (2, N), and the bounds above:
    dict(pit, dpit (E, 2, N); row, drow (E, 3): chi2_mean, p_chi2, p_max; x_min, x_max (E,): T / 2 over the good rows;
    good (E, R)).  A spectrum with a row that is not finite is NaN throughout.  K: the ulps of whoever computed."""
    Z = np.asarray(Z, dtype=np.float64)
    E, R, _, N = Z.shape
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), (E, 2, N)).astype(LD)
    iv = np.broadcast_to(np.asarray(iv, dtype=np.float64), (E, 2, N)).astype(LD)
    n = 2 * N
    ET = (KQ + n - 1) * U
    with np.errstate(all='ignore'):
        d = y[:, None] - Z.astype(LD)                          # (E, R, 2, N)
        q = d * d * iv[:, None]
        T = q.sum(axis=(2, 3))
        good = np.isfinite(T.astype(np.float64))
        clean = good.all(axis=1)
        # pit
        z = d * np.sqrt(iv)[:, None]
        Phi = erfc_ld(-z / _SQRT2) / 2
        phi_z = np.exp(-z * z / 2) / np.sqrt(2 * LD(math.pi)) * np.abs(z)
        pit = Phi.mean(axis=1)
        dpit = U * ((R + K['erfc']) * pit + k_arg * phi_z.mean(axis=1)) + TINY
        # p_chi2
        x = np.where(good, T / 2, LD(0))
        Q, top = chi2_sf_ld(N, x)
        rel = chi2_sf_rel_bound(N, x, K)
        p_chi2 = Q.mean(axis=1)
        dp_chi2 = (Q * rel + top * x * ET).mean(axis=1) + R * U * p_chi2 + TINY
        # p_max
        qm = np.where(good, q.reshape(E, R, n).max(axis=2), LD(0))
        p, dp = max_abs_sf_ld(n, qm, K, KQ / 2 + 1)
        p_max = p.mean(axis=1)
        dp_max = dp.mean(axis=1) + R * U * p_max + TINY
        chi2_mean = np.where(good, T, LD(0)).mean(axis=1)
        row = np.stack([chi2_mean, p_chi2, p_max], axis=1)
        drow = np.stack([(ET + R * U) * chi2_mean, dp_chi2, dp_max], axis=1)
        pit[~clean], dpit[~clean], row[~clean], drow[~clean] = np.nan, np.nan, np.nan, np.nan
        x_good = np.where(good, x, LD(0)).astype(np.float64)
    return dict(pit=pit, dpit=dpit, row=row, drow=drow, good=good, x_min=np.where(good, x_good, np.inf).min(axis=1),
                x_max=x_good.max(axis=1))


def assert_all_within(pit, row, ref, what):
    """pit and the columns of row against the yardstick; returns the worst error / bound of pit, chi2_mean, p_chi2, p_max."""
    worst = [assert_within(pit, ref, 'pit', what)]
    for c, name in enumerate(('chi2_mean', 'p_chi2', 'p_max')):
        col = {name: ref['row'][:, c], 'd' + name: ref['drow'][:, c]}
        worst.append(assert_within(row[:, c], col, name, what))
    return tuple(worst)


def sum_bounds(a, b):
    """The bounds of two computations of the same quantity, added: each lies within its own of the yardstick."""
    return dict(a, dpit=a['dpit'] + b['dpit'], drow=a['drow'] + b['drow'])
