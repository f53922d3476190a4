"""What tests/test_evidence.py and tests/test_gpu_evidence.py share: the first-order bounds the bridge-sampling code is held
to.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, "Accuracy and Stability of Numerical Algorithms", 2nd ed., ch. 3 and 8).

log_g(x) = -0.5 sum z_j^2 - c with L z = x - mu.
  * d = x - mu is one rounding, the substitution of row j a sum of j products and a division: the computed z solves (L + dL)
    z = d (1 + delta) with |dL| <= gamma_ndim |L| (Higham Thm 8.5), fma or not, so to first order |dz| <= gamma_{ndim+1} |L^-1|
    (|L| |z|), componentwise.
  * m = sum z_j^2 of the computed z in ndim additions: |dm| <= 2 sum |z_j| |dz_j| + gamma_{ndim+1} m.
  * log_g = -0.5 m - c: one or two roundings of a value no larger than 0.5 m + |c|.
  logg_bound = 0.5 dm + 2 u (0.5 m + |c|).  It holds for evidence.log_g, evidence.ordered_logg and the device alike.

The estimate.  With h(r) = F(r) / r the iteration's fixed point is h = 1; h decreases in r and increases in every l1_j and l2_i
(each numerator term e^l2 / (s1 e^l2 + s2 r) grows with l2, each denominator term 1 / (s1 e^l1 + s2 r) falls with l1), so
raising every l by at most eps raises log r* by at most eps, and shifting all by eps shifts it by eps exactly: |d log r*| <=
max |dl|.  Two evaluations of the same estimate whose l differ entry by entry by at most eps therefore differ by at most eps
in log_ml at the fixed point.
  * an entry of l1: two log_g (2 logg_bound), the stored logp is the same double, l = logp - log_g one rounding a side.
  * an entry of l2: the same draws and the same log_g on both sides; dlogp2, whatever the two log-probabilities differ by.
  * a = exp(l - lstar): the subtraction u |t|, the exp K_exp u, as a perturbation of l (lstar itself cancels in log_ml).
  * the sums of F: positive terms, any order: gamma_{N + 4} each relative; a pass is off by eta = 2 (gamma_{N1+4} + gamma_{N2+4}).
  * stopping: a side stops when its step is within tol r'; with the contraction rate rho of the iteration (measured on the
    NumPy definition's own history of r: the largest ratio of successive steps) it is then within (tol + eta) / (1 - rho) of
    its fixed point.
  * log r: K_log u |log r|; log r + lstar: u |log_ml|.
"""
import numpy as np

from fit_quality_bounds import K_DEVICE, K_NUMPY

U = 2.0 ** -53
FACTOR = 16          # a library function on the device against the float64 definition's own worst error (tests/loo_bounds.py)
LD = np.longdouble


def gamma(k):
    return k * U / (1 - k * U)


def whiten(x, mu, L):
    """z with L z = x - mu, in long double."""
    d = np.asarray(x, dtype=LD) - np.asarray(mu, dtype=LD)
    Ll = np.asarray(L, dtype=LD)
    z = np.empty_like(d)
    for j in range(d.shape[-1]):
        z[..., j] = (d[..., j] - (Ll[j, :j] * z[..., :j]).sum(axis=-1)) / Ll[j, j]
    return z


def logg_ld(x, mu, L, c):
    z = whiten(x, mu, L)
    return -(z * z).sum(axis=-1) / 2 - LD(c)


def logg_bound(L, c, z):
    """The bound of the module's docstring for rows whose whitened coordinates are z (R, ndim): (R,)."""
    ndim = L.shape[0]
    T = np.tril(np.asarray(L, dtype=np.float64))
    az = np.abs(np.asarray(z, dtype=np.float64))
    dz = gamma(ndim + 1) * (az @ np.abs(T).T) @ np.abs(np.linalg.inv(T)).T
    m = (az * az).sum(axis=-1)
    return 0.5 * (2 * (az * dz).sum(axis=-1) + gamma(ndim + 1) * m) + 2 * U * (0.5 * m + abs(float(c)))


def contraction(history):
    """The largest ratio of successive steps of an iteration's history of r (0 with fewer than three)."""
    h = np.asarray(history, dtype=np.float64)
    if h.size < 3:
        return 0.0
    s = np.abs(np.diff(h))
    with np.errstate(all='ignore'):
        q = s[1:] / s[:-1]
    q = q[np.isfinite(q)]
    return float(min(q.max(), 0.99)) if q.size else 0.0


def iterate_bound(N1, N2, history, tol):
    """How far two iterations of the same a1, a2 may end apart in r, relative: each within (tol + eta) / (1 - rho) of the fixed
    point."""
    eta = 2 * (gamma(N1 + 4) + gamma(N2 + 4))
    return 2 * (tol + eta) / (1 - contraction(history))


def log_ml_bound(L, c, z1, logp1, l1, l2, lstar, dlogp2, log_ml, log_r, history, tol):
    """|log_ml of the device - log_ml of the NumPy definition| of one ensemble, as the module's docstring adds it up."""
    k_exp = K_DEVICE[0] + K_NUMPY[0]
    k_log = K_DEVICE[1] + K_NUMPY[1]
    fin2 = np.isfinite(l2)
    e1 = (2 * logg_bound(L, c, z1) + 2 * U * (np.abs(logp1) + np.abs(l1)) + 2 * U * np.abs(l1 - lstar)).max()
    e2 = (dlogp2 + 2 * U * (np.abs(l2[fin2]) + np.abs(l2[fin2] - lstar))).max() if fin2.any() else 0.0
    return float(max(e1, e2) + k_exp * U + iterate_bound(l1.size, l2.size, history, tol) + k_log * U * abs(log_r)
                 + 2 * U * abs(log_ml))
