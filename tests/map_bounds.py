"""What tests/test_mapfit.py and tests/test_gpu_mapfit.py share: the five bundled cases of the MAP fit with their starts, and
the long-double yardstick of the normal equations (bisip_amd.mapfit, "Normal equations") with the tolerance held against it.

The yardstick evaluates the Cole-Cole response in NumPy's long double at the points of the same stencil (theta, theta +- h_j e_j,
formed in long double from the float64 theta and h) and takes d, dZ_j and the three sums in long double.  Its derivative is a
central difference like the definition's, so test_mapfit.py checks it against mpmath.diff of the same response on a few
points: the truncation h^2 Z''' / 6 with h <= 2e-5 (log_tau: 1e-6 of a range of 20) is 7e-11 times Z''' / Z', and the long
double rounding 1e-19 / h <= 1e-13 of |Z|; DIFF_RTOL = 1e-7 of max |dZ_j| leaves room for third derivatives a thousand times
the first.

Errors are measured against the natural scale of every quantity (Cauchy-Schwarz): chi2 against chi2, g_j against
sqrt(A_jj chi2), A_jk against sqrt(A_jj A_kk).  The float64 definition's own error is the cancellation of the central
difference, about u |Z| / h = 1e-10 of dZ for h = 1e-6 of the range and more where the response hardly depends on the parameter.
Following the project's rule (tests/loo_bounds.py, FACTOR) whoever computes the definition in another order -- the ordered
restatement, the device -- is allowed FACTOR = 16 times the definition's own worst error over the same points; that worst
error, measured over ``points(K, 64)`` for K = 1 and 2 on the bundled spectrum SIP-K389174 (1.285e-9 and 1.247e-9 of the
scale), is written down as OWN = 1.5e-9, rounded up, and test_mapfit.py measures it again and holds it below that figure."""
import numpy as np

import bisip_amd
from bisip_amd import mapfit as mf

LD = np.longdouble
PI_LD = LD('3.141592653589793238462643383279502884')
FACTOR = 16
OWN = 1.5e-9                       # the float64 definition against the yardstick, worst scaled error over points(K, 64)
DIFF_RTOL = 1e-7                   # the yardstick's central difference against mpmath.diff, relative to max |dZ_j|
N_STARTS, START_SEED = 32, 7

# (id, class name, keyword arguments, bundled spectrum)
CASES = (('pd5', 'PolynomialDecomposition', dict(poly_deg=5), 'SIP-K389175'),
         ('cc2', 'PeltonColeCole', dict(n_modes=2), 'SIP-K389174'),
         ('cc1', 'PeltonColeCole', dict(n_modes=1), 'SIP-K389174'),
         ('dias', 'Dias2000', {}, 'SIP-K389176'),
         ('shin', 'Shin2015', {}, 'SIP-K389175'))
CASE_IDS = [c[0] for c in CASES]


def model_of(case, **kw):
    _, name, mkw, key = case
    return getattr(bisip_amd, name)(bisip_amd.DataFiles()[key], **dict(dict(nwalkers=32, nsteps=10), **mkw, **kw))


def oracle_problem(m):
    import oracle
    d = m.data
    kw = {}
    if isinstance(m, bisip_amd.PolynomialDecomposition):
        kw = dict(taus=m.taus, log_taus=m.log_taus, c_exp=m.c_exp)
    elif isinstance(m, bisip_amd.PeltonColeCole):
        kw = dict(n_modes=m.n_modes)
    return oracle.OracleProblem(type(m).__name__, d['w'], d['zn'], d['zn_err'], m.param_bounds, **kw)


def starts_of(m, n=N_STARTS, seed=START_SEED):
    b = m.param_bounds
    return np.random.RandomState(seed).uniform(b[0], b[1], (n, b.shape[1]))


def inverse_variance(err):
    from bisip_amd.fitquality import inverse_variance as iv
    return iv(err)


# -- the long-double yardstick (Cole-Cole) -------------------------------------------------------------------------------
def colecole_ld(theta, w, K):
    """Z (..., 2, N) in long double of rows theta (..., 1 + 3K) (long double): r0 (1 - sum m (1 - 1 / (1 + (i w tau)^c)))."""
    theta = np.asarray(theta, dtype=LD)
    w = np.asarray(w, dtype=LD)
    r0 = theta[..., 0, None]
    z = np.zeros(theta.shape[:-1] + w.shape, dtype=np.clongdouble)
    for k in range(K):
        m, lt, c = theta[..., 1 + k, None], theta[..., 1 + K + k, None], theta[..., 1 + 2 * K + k, None]
        x = np.exp(c * (np.log(w) + lt)) * (np.cos(c * PI_LD / 2) + 1j * np.sin(c * PI_LD / 2))     # (i w tau)^c
        z = z + m * (1 - 1 / (1 + x))
    Z = r0 * (1 - z)
    return np.stack([Z.real, Z.imag], axis=-2)


def yardstick(theta, w, K, y, iv, bounds):
    """``(chi2, g, A, J)`` in long double at the float64 rows theta (..., 1 + 3K)."""
    h, _, _ = mf.inner_box(bounds)
    n = theta.shape[-1]
    t = np.asarray(theta, dtype=np.float64).astype(LD)
    pts = np.repeat(t[..., None, :], 2 * n + 1, axis=-2)
    for j in range(n):
        pts[..., 1 + 2 * j, j] = t[..., j] + LD(h[j])
        pts[..., 2 + 2 * j, j] = t[..., j] - LD(h[j])
    Z = colecole_ld(pts, w, K)
    d = np.asarray(y, dtype=LD) - Z[..., 0, :, :]
    J = (Z[..., 1::2, :, :] - Z[..., 2::2, :, :]) / (2 * h.astype(LD))[:, None, None]
    iv = np.asarray(iv, dtype=LD)
    chi2 = np.sum(d * d * iv, axis=(-2, -1))
    g = -np.sum(J * d[..., None, :, :] * iv, axis=(-2, -1))
    A = np.einsum('...jpf,...kpf,pf->...jk', J, J, iv)
    return chi2, g, A, J


def scaled_errors(got, ref):
    """The worst error of got = (chi2, g, A) against ref = the yardstick's (chi2, g, A), each on its natural scale."""
    chi2, g, A = (np.asarray(x).astype(LD) for x in got)
    rc, rg, rA = ref[:3]
    diag = np.sqrt(np.diagonal(rA, axis1=-2, axis2=-1))
    e_c = np.max(np.abs(chi2 - rc) / rc)
    e_g = np.max(np.abs(g - rg) / (diag * np.sqrt(rc)[..., None]))
    e_A = np.max(np.abs(A - rA) / (diag[..., :, None] * diag[..., None, :]))
    return float(max(e_c, e_g, e_A))


def points(K, n, seed=0):
    """n rows uniform in the middle 90 % of the default Cole-Cole box, where every parameter moves the response."""
    lo = np.array([0.9] + [0.0] * K + [-15.0] * K + [0.0] * K)
    hi = np.array([1.1] + [1.0] * K + [5.0] * K + [1.0] * K)
    u = np.random.default_rng([seed, K]).uniform(0.05, 0.95, (n, 1 + 3 * K))
    return lo + u * (hi - lo), np.array([lo, hi])
