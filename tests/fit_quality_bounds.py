"""What tests/test_fit_quality.py and tests/test_gpu_fit_quality.py share: the long-double evaluation of the definitions of
bisip_amd.fitquality (per data point over the rows of a chain: mean and variance, ddof = 1, of q = (y - Z)^2 iv, and lmeh =
log mean exp(-q / 2)), first-order error bounds of bisip_fit_quality_dev's way of computing them in any summation order,
and hand-built inputs.  u = 2^-53.  The responses Z, the measurement y and the inverse variance iv are doubles and ARE the
data; the yardstick evaluates everything from them in long double.

q.  The device rounds d = y - Z, t = d d and q = t iv each on its own: q~ = q (1 + e), |e| <= KQ u with KQ = 4 (three
roundings, that of d counted twice by the square).

mean_q, var_q.  The bound of tests/response_bounds.py with ddof = 1, the device's q~ in the place of the PA kind's x~.  For
one point with R rows, c = q~_0, d_i = q~_i - c (one rounding each):
  S = sum d:                    |dS| <= (R - 1) u sum|d|               whatever the order (slots, runs, segments)
  P = sum d^2:                  |dP| <= (R + 1) u sum d^2              (the product rounded on its own)
  mean = c + S / R:             |dmean| <= |dS| / R + u |S / R| + u |mean|
  Q = (S S) / R:                |dQ|    <= 2 |S| |dS| / R + 2 u |Q|
  var = (P - Q) / (R - 1):      |dvar|  <= (|dP| + |dQ| + u |P - Q|) / (R - 1) + u var
and, exactly evaluated, the moments of q~ differ from those of q by
      |mean~ - mean| <= KQ u sum|q| / R
      |var~ - var|   <= (2 / (R - 1)) sum|q_i - mean| * 2 * (KQ u max|q|),
which are added.  R = 1: the variance is NaN on both sides.

lmeh = -m / 2 + log(s / R), m = min q, s = sum exp(-(q_i - m) / 2): an ABSOLUTE bound.
  * Every term of s is positive, so relative errors of terms bound the relative error of s.  A term is created by one exp
    and then travels along a chain of steps to the final s: the later rows of its slot, 6 pairwise levels within its
    wave, 3 merges of the four waves, nseg - 1 merges of segments -- at most L = rows per slot + 8 + nseg steps, its
    creation included.  A step is at most one rescale (an exp: K_exp u; the product: u) and one addition (u): (K_exp + 2) u.
  * The exponents themselves are rounded differences, -(a - b) / 2 with a relative error u of a - b (the halving is
    exact): an absolute error u (a - b) / 2 of the exponent is a relative one of the factor.  Along the chain of a term
    the differences telescope from q_i down to the final minimum: at most u (q_max - q_min) / 2 together.
  * s / R: u.  log: K_log u |log(s / R)|.  The final sum: u |lmeh| <= u |m / 2| + u |log(s / R)|.
  * The device's rows are q~: d lmeh / d q_i = -w_i / 2 with w_i = exp(-(q_i - m) / 2) / s, so the roundings of q move
    lmeh by at most KQ u sum_i w_i q_i / 2.
  dlmeh = u [L (K_exp + 2) + (q_max - q_min) / 2 + 1 + (K_log + 1) |log(s / R)| + |m / 2| + KQ sum w q / 2].
K_exp, K_log: the ulp of whoever computed exp and log, counted as tests/response_bounds.py counts K (a term K u |x|).
Every term is first order in u; the quantities on the right come from the long-double evaluation.
"""
import numpy as np

from bisip_amd.response import plan
from convergence_bounds import LD, U
from covariance_bounds import assert_within      # noqa: F401  (shared with the tests)

KQ = 4
# ulp of the device's double exp / log: the HIP math documentation installed with this ROCm states none, so OpenCL full
# profile's (OpenCL C specification, "Relative error as ULPs", double precision: exp <= 3 ulp, log <= 3 ulp), plus glibc's
# expl / logl of the long-double yardstick, as tests/test_gpu_response.py takes hypot and atan2
EXP_ULP, LOG_ULP, GLIBC_ULP = 3, 3, 1
K_DEVICE = (EXP_ULP + GLIBC_ULP, LOG_ULP + GLIBC_ULP)
# NumPy's exp / log (glibc) in ordered_fit_sums: each within 1 ulp <= 2 u |x|, and the yardstick's own
K_NUMPY = (2 + GLIBC_ULP, 2 + GLIBC_ULP)


def q_ld(Z, y, iv):
    """q (E, R, 2N) in long double of Z (E, R, 2, N), y and iv (E, 2, N)."""
    E, R, _, N = Z.shape
    d = y.astype(LD)[:, None] - Z.astype(LD)
    return (d * d * iv.astype(LD)[:, None]).reshape(E, R, 2 * N)


def reference_and_bounds(Z, y, iv, n_spectra=None, K=K_DEVICE):
    """Long-double (mean_q, var_q, lmeh) of the definitions over the rows of every spectrum of Z (E, R, 2, N) with y, iv
    (E, 2, N) or (2, N), and the bounds above: dict(mean_q, var_q, lmeh, dmean_q, dvar_q, dlmeh, q_min, q_max), each
    (E, 2, N).  n_spectra: the spectra of the call (the plan depends on it).  K = (K_exp, K_log)."""
    Z = np.asarray(Z, dtype=np.float64)
    E, R, _, N = Z.shape
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), (E, 2, N))
    iv = np.broadcast_to(np.asarray(iv, dtype=np.float64), (E, 2, N))
    seg_rows, nseg, slots = plan(R, E if n_spectra is None else n_spectra, 1)
    L = -(-min(seg_rows, R) // slots) + 8 + nseg
    K_exp, K_log = K
    names = ('mean_q', 'var_q', 'lmeh', 'dmean_q', 'dvar_q', 'dlmeh', 'q_min', 'q_max')
    out = {k: [] for k in names}
    with np.errstate(all='ignore'):
        qq = q_ld(Z, y, iv)
        for e in range(E):
            x = qq[e]                                     # (R, 2N)
            d = x - x[0]
            S = d.sum(axis=0)
            md = S / R
            mean = x[0] + md
            z = d - md
            var = (z * z).sum(axis=0) / LD(R - 1)
            a, P = np.abs(d).sum(axis=0), (d * d).sum(axis=0)
            dS = (R - 1) * U * a
            dP = (R + 1) * U * P
            dmean = dS / R + U * np.abs(md) + U * np.abs(mean)
            Q = S * S / R
            dQ = 2 * np.abs(S) * dS / R + 2 * U * np.abs(Q)
            dvar = (dP + dQ + U * np.abs(P - Q)) / LD(R - 1) + U * var
            ax = np.abs(x)
            dmean = dmean + KQ * U * ax.sum(axis=0) / R
            dvar = dvar + (2.0 / LD(R - 1)) * np.abs(z).sum(axis=0) * 2 * (KQ * U * ax.max(axis=0))
            m, top = x.min(axis=0), x.max(axis=0)
            t = np.exp(-(x - m) / 2)
            s = t.sum(axis=0)
            ls = np.log(s / R)
            lmeh = -m / 2 + ls
            wq = (t * x).sum(axis=0) / s
            dlmeh = U * (L * (K_exp + 2) + (top - m) / 2 + 1 + (K_log + 1) * np.abs(ls) + np.abs(m / 2) + KQ * wq / 2)
            for k, v in zip(names, (mean, var, lmeh, dmean, dvar, dlmeh, m, top)):
                out[k].append(v.reshape(2, N))
    return {k: np.stack(v) for k, v in out.items()}


def assert_all_within(got, ref, what):
    """(mean_q, var_q, lmeh) against the yardstick; returns the worst error / bound of each."""
    return tuple(assert_within(g, ref, name, what) for g, name in zip(got, ('mean_q', 'var_q', 'lmeh')))


# -- hand-built inputs ---------------------------------------------------------------------------------------------------
def data_for(Z, seed=0, rel_err=0.02):
    """A measurement and its errors for responses Z (E, R, 2, N): y = the first row's response moved by about one error,
    err = rel_err of its size -- q of order 1 where the rows scatter by about rel_err.  Returns (y, err), (E, 2, N)."""
    rng = np.random.default_rng(seed + Z.shape[1])
    err = rel_err * np.abs(Z[:, 0]) * rng.uniform(0.5, 2.0, Z[:, 0].shape) + 3e-3      # (Im Z is small: a floor)
    return Z[:, 0] + err * rng.normal(size=err.shape), err


def inverse_variance(err):
    """1 / err^2 squared and inverted in long double, rounded once: the context's own (host_precompute.cpp)."""
    e = np.asarray(err, dtype=np.float64).astype(LD)
    return (LD(1) / (e * e)).astype(np.float64)
