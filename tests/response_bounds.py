"""What tests/test_response.py and tests/test_gpu_response.py share: the long-double evaluation of the definitions of
bisip_amd.response (mean and standard deviation of the model response over a chain, in Re / Im or in amplitude / minus
phase) and the first-order error bound of the shifted sums in any summation order.

The bound is that of tests/covariance_bounds.py for a diagonal entry, with ddof = 0.  u = 2^-53.  For one (spectrum, part,
frequency) with R rows, x_i the response of row i in the representation asked for, c = x_0, d_i = x_i - c (one rounding
each; d_0 = 0 exactly):
  S = sum d.  At most R - 2 additions touch an element and its own rounding is one more:
      |dS| <= (R - 1) u sum|d|                                        whatever the order (slots, runs, segments).
  P = sum d^2.  The product carries twice the rounding of d and its own (the kernel rounds the product on its own, no fma),
  then at most R - 2 additions:
      |dP| <= (R + 1) u sum d^2.
  mean = c + S / R:             |dmean| <= |dS| / R + u |S / R| + u |mean|.
  Q = (S S) / R:                |dQ|    <= 2 |S| |dS| / R + 2 u |Q|.
  var = (P - Q) / R:            |dvar|  <= (|dP| + |dQ| + u |P - Q|) / R + u var.
  std = sqrt(var):              |dstd|  <= min(|dvar| / std, sqrt(|dvar|)) + u std
      (|sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(b), and <= sqrt(|a - b|): no first-order step,
      so the bound also holds where the response does not vary and std = 0).
The PA kind.  The definitions take the amplitude and phase of the Re / Im doubles exactly; the device takes them with its
own hypot / atan2: x~_i = x_i (1 + e_i), |e_i| <= K u, the one more term K u |x| per element (K: the constants of
tests/test_gpu_response.py).  The sums above are then those of x~ (their bound is unchanged to first order), and exactly
evaluated the moments of x~ differ from those of x by
      |mean~ - mean| <= K u sum|x| / R
      |var~ - var|   <= (2 / R) sum|x_i - mean| * 2 * (K u max|x|)    (each e_i x_i less their mean: twice the largest),
which are added to dmean and dvar before dstd is taken.  K = 0 for the RI kind: forward's doubles ARE the data.
Every term is first order in u; the quantities on the right are taken from the long-double evaluation, which works on
x - c (exact in long double for RI) so that its own rounding stays far below the bound.
"""
import numpy as np

from convergence_bounds import LD, U
from covariance_bounds import assert_within      # noqa: F401  (shared with the tests)


def represent_ld(Z, kind):
    """Z (..., 2, N) float64 -> the representation ``kind`` in long double, (..., 2 N)."""
    z = np.asarray(Z, dtype=np.float64).astype(LD)
    if kind == 'pa':
        z = np.stack([np.hypot(z[..., 0, :], z[..., 1, :]), -np.arctan2(z[..., 1, :], z[..., 0, :])], axis=-2)
    return z.reshape(z.shape[:-2] + (-1,))


def reference_and_bounds(Z, kind='ri', K=(0, 0)):
    """Long-double (mean, std) of the definitions over the rows of every spectrum of Z (E, R, 2, N), and the bounds above:
    dict(mean, std, dmean, dstd), each (E, 2, N).  K = (K of the amplitude, K of the phase) of whoever computed the PA
    representation; (0, 0) for RI."""
    Z = np.asarray(Z, dtype=np.float64)
    E, R, _, N = Z.shape
    Kv = np.repeat(np.asarray(K, dtype=LD), N) if kind == 'pa' else np.zeros(2 * N, dtype=LD)
    out = {k: [] for k in ('mean', 'std', 'dmean', 'dstd')}
    with np.errstate(all='ignore'):
        for e in range(E):
            x = represent_ld(Z[e], kind)                  # (R, 2N)
            d = x - x[0]
            S = d.sum(axis=0)
            md = S / R
            mean = x[0] + md
            z = d - md
            var = (z * z).sum(axis=0) / R
            std = np.sqrt(var)
            a, P = np.abs(d).sum(axis=0), (d * d).sum(axis=0)
            dS = (R - 1) * U * a
            dP = (R + 1) * U * P
            dmean = dS / R + U * np.abs(md) + U * np.abs(mean)
            Q = S * S / R
            dQ = 2 * np.abs(S) * dS / R + 2 * U * np.abs(Q)
            dvar = (dP + dQ + U * np.abs(P - Q)) / R + U * var
            ax = np.abs(x)
            dmean = dmean + Kv * U * ax.sum(axis=0) / R
            dvar = dvar + (2.0 / R) * np.abs(z).sum(axis=0) * 2 * (Kv * U * ax.max(axis=0))
            dstd = np.minimum(np.where(std > 0, dvar / np.where(std > 0, std, 1), np.inf), np.sqrt(dvar)) + U * std
            for k, v in (('mean', mean), ('std', std), ('dmean', dmean), ('dstd', dstd)):
                out[k].append(v.reshape(2, N))
    return {k: np.stack(v) for k, v in out.items()}


def responses(E, R, N, seed=0):
    """Hand-built responses (E, R, 2, N) with Re Z > 0, as every model gives inside its prior box: a smooth spectrum per
    spectrum plus a posterior scatter of a few per cent, correlated between the parts; frequency 0 of the last spectrum
    does not vary at all (std exactly 0)."""
    rng = np.random.default_rng(1000 * E + 10 * R + N + seed)
    f = np.linspace(0.0, 1.0, N)
    re0 = 1.0 - 0.3 * f + 0.05 * rng.normal(size=(E, 1, N))
    im0 = -0.02 - 0.1 * f * (1 - f) + 0.005 * rng.normal(size=(E, 1, N))
    g = rng.normal(size=(E, R, 1))
    re = re0 * (1 + 0.03 * g + 0.004 * rng.normal(size=(E, R, N)))
    im = im0 * (1 - 0.2 * g + 0.05 * rng.normal(size=(E, R, N)))
    Z = np.stack([re, im], axis=2)
    Z[E - 1, :, :, 0] = Z[E - 1, 0, :, 0]
    assert (Z[:, :, 0] > 0).all()
    return Z
