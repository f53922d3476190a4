"""What tests/test_modes.py and tests/test_gpu_modes.py share: the rows, the long-double yardstick of the per-mode descriptors
(bisip_amd.modes, "Descriptors") and their first-order error bound.

The ordered row is a permutation and m_total a chain of plain additions in a stated order: both are held bit for bit, not to
a bound.  For the two relaxation times, with u = 2^-53, l = log1p(-m'), q = l / c' and e_l the relative error of the log1p
that an implementation uses:

  the quotient:      |dq|    <= |q| (e_l + u + e_l u)                 (the error of l, one rounding of the division);
  the halving:       2 c' and q / 2 are exact (no rounding; an overflow of l / c' that l / (2 c') avoids does not occur for
                     c' >= 2^-1000), so log_tau_peak has the bound of log_tau_cc with q / 2 for q;
  the sum:           |d(lt + q)| <= |dq| + u (|lt + q| + |dq|)        (one rounding of the sum).

The quantities on the right come from the yardstick (NumPy's long double: every input converts exactly).

e_l is not invented.  It follows the project's rule (tests/loo_bounds.py, FACTOR): whoever computes the definition -- the host
entry point with its C library's log1p, the device with its own -- is allowed FACTOR = 16 times the NumPy definition's own
worst relative error of log1p(-m) against the yardstick over the same families of rows.  That worst error, measured over
the two families below (rows uniform in the default box; rows within 1e-12 of its edges; ``families(K, 200000 // K, seed)`` for
K = 1 and 5, seeds 0 ... 3) is 1.215e-16 in the box and 1.110e-16 at the edges (u = 1.110e-16: glibc's log1p stays within
0.55 ulp) and is written down as LOG1P_OWN = 1.25e-16, rounded up; test_modes.py measures it again and holds it below that
figure.  A log1p of a few ulp fits 16 times that.
"""
import numpy as np

from bisip_amd import modes

U = 2.0 ** -53
LD = np.longdouble
FACTOR = 16
LOG1P_OWN = 1.25e-16               # NumPy's log1p(-m) against long double, relative, worst over both families (docstring)
E_LOG1P = FACTOR * LOG1P_OWN
EDGE = 1e-12                       # how near the box's edges the second family lies (relative to the width of the box)


def default_bounds(K):
    """The default box of PeltonColeCole(n_modes=K): (2, 1 + 3K)."""
    lo = [0.9] + [0.0] * K + [-15.0] * K + [0.0] * K
    hi = [1.1] + [1.0] * K + [5.0] * K + [1.0] * K
    return np.array([lo, hi])


def box_rows(rng, n, K):
    """n rows uniform in the default box."""
    lo, hi = default_bounds(K)
    return rng.uniform(lo, hi, (n, 1 + 3 * K))


def edge_rows(rng, n, K):
    """n rows whose every parameter lies within EDGE (times the width) of the lower or of the upper edge, inside the box."""
    lo, hi = default_bounds(K)
    d = rng.uniform(0.0, EDGE, (n, 1 + 3 * K)) * (hi - lo)
    x = np.where(rng.integers(0, 2, (n, 1 + 3 * K)) == 1, hi - d, lo + d)
    return np.clip(x, np.nextafter(lo, hi), np.nextafter(hi, lo))


def families(K, n, seed=0):
    return {'box': box_rows(np.random.default_rng([seed, K, 1]), n, K), 'edges': edge_rows(np.random.default_rng([seed, K, 2]), n, K)}


def log1p_own_error(rows, K):
    """The worst relative error of NumPy's float64 log1p(-m) against long double over the m of the rows."""
    m = rows[..., 1:1 + K].ravel()
    want = np.log1p(-m.astype(LD))
    ok = want != 0
    return float(np.max(np.abs(np.log1p(-m).astype(LD) - want)[ok] / np.abs(want[ok])))


def yardstick(theta, K, by='log_tau'):
    """``(values, bound)`` (..., 1 + 2K) in long double: the descriptors of the ordered rows and the bound of the docstring
    for the two relaxation times (0 for m_total: held bit for bit elsewhere, here to the rounding of its additions)."""
    o = modes.order_modes(theta, K, by).astype(LD)
    m, lt, c = o[..., 1:1 + K], o[..., 1 + K:1 + 2 * K], o[..., 1 + 2 * K:]
    with np.errstate(all='ignore'):
        q = np.log1p(-m) / c
        values = np.concatenate([m.sum(axis=-1, keepdims=True), lt + q, lt + q / 2], axis=-1)
        bound = np.zeros_like(values)
        for k, qq in ((1, q), (1 + K, q / 2)):
            dq = np.abs(qq) * (E_LOG1P + U + E_LOG1P * U)
            bound[..., k:k + K] = dq + U * (np.abs(lt + qq) + dq)
        bound[..., 0] = (K - 1) * U * np.abs(m).sum(axis=-1)
    return values, bound


def assert_within(got, theta, K, by='log_tau', what=''):
    """The descriptors ``got`` of finite rows within the bound of the yardstick, every entry."""
    values, bound = yardstick(theta, K, by)
    assert np.isfinite(values.astype(np.float64)).all(), what
    err = np.abs(got.astype(LD) - values)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    assert worst <= 1.0, f'{what}: {worst:.3f} times the bound'
    return worst
