"""What tests/test_covariance.py and tests/test_gpu_covariance.py share: the long-double evaluation of the definitions of
bisip_amd.covariance and the first-order error bound of the shifted sums in any summation order.

The bound.  u = 2^-53.  For one ensemble of N rows, c its first row, d_i = x_i - c (one rounding each; d_0 = 0 exactly):
  S_j = sum d_j.  At most N - 2 additions touch an element and its own rounding is one more:
      |dS_j| <= (N - 1) u sum|d_j|                                    whatever the order (slots, runs, segments).
  P_jk = sum d_j d_k.  The product carries the roundings of d_j and d_k and its own (the kernel rounds the product on its
  own, no fma), then at most N - 2 additions:
      |dP_jk| <= (N + 1) u sum|d_j d_k|.
  mean_j = c_j + S_j / N:       |dmean| <= |dS_j| / N + u |S_j / N| + u |mean_j|.
  Q = (S_j S_k) / N:            |dQ|    <= (|S_j| |dS_k| + |S_k| |dS_j|) / N + 2 u |Q|.
  cov = (P - Q) / (N - 1):      |dcov|  <= (|dP| + |dQ| + u |P - Q|) / (N - 1) + u |cov|.
  corr_jk = cov_jk / s, s = sqrt(cov_jj cov_kk), computed on the host from the device's covariance by two divisions by the
  rounded square roots and a clip (which only moves a value towards the exact one):
      |dcorr| <= |dcov_jk| / s + |corr| (|dcov_jj| / (2 cov_jj) + |dcov_kk| / (2 cov_kk)) + 4 u |corr|.
Every term is first order in u; the quantities on the right are taken from the long-double evaluation, which works on
x - c (exact in long double) so that its own rounding stays far below the bound.
"""
import numpy as np

from convergence_bounds import LD, U


def rows_of(x, E):
    """(E, N, ndim) rows of a chain (n, E * Wp, ndim) in the order k * Wp + w."""
    n, W, ndim = x.shape
    return x.reshape(n, E, W // E, ndim).transpose(1, 0, 2, 3).reshape(E, -1, ndim)


def reference_and_bounds(x, E):
    """Long-double (mean, cov, corr) of the definitions per ensemble and the bounds above: dict(mean, cov, corr, dmean,
    dcov, dcorr), shaped (E, ndim), (E, ndim, ndim), (E, ndim, ndim)."""
    rows = rows_of(np.asarray(x, dtype=np.float64), E)
    _, N, ndim = rows.shape
    out = {k: [] for k in ('mean', 'cov', 'corr', 'dmean', 'dcov', 'dcorr')}
    with np.errstate(all='ignore'):
        for e in range(E):
            r = rows[e].astype(LD)
            d = r - r[0]
            S = d.sum(axis=0)
            md = S / N
            mean = r[0] + md
            z = d - md
            cov = np.dot(z.T, z) / (N - 1)
            a = np.abs(d)
            P, AP = np.dot(d.T, d), np.dot(a.T, a)
            dS = (N - 1) * U * a.sum(axis=0)
            dP = (N + 1) * U * AP
            dmean = dS / N + U * np.abs(md) + U * np.abs(mean)
            Q = np.outer(S, S) / N
            dQ = (np.outer(np.abs(S), dS) + np.outer(dS, np.abs(S))) / N + 2 * U * np.abs(Q)
            dcov = (dP + dQ + U * np.abs(P - Q)) / (N - 1) + U * np.abs(cov)
            var = np.diagonal(cov)
            s = np.sqrt(np.outer(var, var))
            corr = cov / s
            rel = np.diagonal(dcov) / (2 * var)
            dcorr = dcov / s + np.abs(corr) * (rel[:, None] + rel[None, :]) + 4 * U * np.abs(corr)
            for k, v in (('mean', mean), ('cov', cov), ('corr', corr), ('dmean', dmean), ('dcov', dcov), ('dcorr', dcorr)):
                out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def assert_within(got, ref, name, label=''):
    """Non-finite exactly where the definition is; elsewhere within the bound.  Returns the worst error / bound."""
    want, bound = ref[name], ref['d' + name]
    fin = np.isfinite(want.astype(np.float64))
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=f'{label} {name}: finite where the definition is')
    with np.errstate(invalid='ignore'):
        err = np.abs(got.astype(LD) - want)[fin]
    b = bound[fin]
    assert (err <= b).all(), (label, name, float((err - b).max()), float(np.max(err / np.where(b > 0, b, 1))))
    if not err.size:
        return 0.0
    return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0)))
