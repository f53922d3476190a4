"""What tests/test_convergence.py and tests/test_gpu_convergence.py share: the long-double evaluation of the definitions
of bisip_amd.convergence, the first-order error bound of the shifted sums in any summation order, and hand-built chains.

The bound.  u = 2^-53.  For one chain of L samples, c its first sample, d_k = x_k - c:
  S1 = sum d_k.  d_0 = 0 exactly, so at most L - 2 additions touch an element and its own rounding is one more:
      |dS1| <= (L - 1) u sum|x - c|                                   whatever the order (segments included).
  S2 = sum d_k^2.  The square carries twice the rounding of d_k and its own, then at most L - 2 additions:
      |dS2| <= (L + 1) u sum (x - c)^2.
  mean = c + S1 / L:            |dmean| <= |dS1| / L + u |S1 / L| + u |mean|.
  Q = S1^2 / L:                 |dQ|    <= 2 |S1| |dS1| / L + 2 u Q.
  N = S2 - Q:                   |dN|    <= |dS2| + |dQ| + u |N|.
  var = N / (L - 1):            |dvar|  <= |dN| / (L - 1) + u var.
Over the M chains of an (ensemble, parameter), m0 the mean of chain 0, dm_c = mean_c - m0:
  Wn = sum(var) / M:            |dWn|   <= sum|dvar| / M + (M - 1) u sum(var) / M + u Wn.
  |ddm_c| <= |dmean_c| + |dmean_0| + u |dm_c|;   T1 = sum dm, T2 = sum dm^2:
      |dT1| <= sum|ddm| + (M - 1) u sum|dm|;   |dT2| <= 2 sum|dm| |ddm| + (M + 1) u sum dm^2;
  Bn from (T1, T2, M) as var from (S1, S2, L).
  R = Bn / Wn:                  |dR|    <= |dBn| / Wn + Bn |dWn| / Wn^2 + u R.
  rhat = sqrt(A + R), A = (L - 1) / L:   |drhat| <= (2 u A + u R + |dR|) / (2 rhat) + u rhat.
Every term is first order in u; the quantities on the right are taken from the long-double evaluation, which works on
x - c (exact in long double) so that its own rounding stays far below the bound.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def split_ld(x, E, split):
    """The chains of x (n, E * Wp, ndim) as (L, splits, E, Wp, ndim) in long double."""
    n, W, ndim = x.shape
    L = n // 2 if split else n
    halves = [x[:L], x[n - L:]] if split else [x]
    return np.stack(halves, axis=1).reshape(L, len(halves), E, W // E, ndim).astype(LD)


def reference_and_bounds(x, E, split):
    """Long-double (mean, var, rhat) of the definitions, shaped as the device's outputs, and the bounds above:
    returns dict(mean, var, rhat, dmean, dvar, drhat) in float64 / long double arrays."""
    c4 = split_ld(x, E, split)                      # (L, splits, E, Wp, ndim)
    L, splits, _, Wp, ndim = c4.shape
    M = splits * Wp
    with np.errstate(all='ignore'):
        # x - c of two doubles is exact in long double wherever it matters (64-bit significand), and the variance does not
        # change under a translation: the definitions are evaluated on d.  Taken on x itself, a mean of size 1e3 carries
        # 1e-16 of long-double rounding, which a width of 1e-8 turns into 1e-14 of the variance -- more than the bound.
        d = c4 - c4[0]
        md = d.mean(axis=0)
        mean = c4[0] + md
        var = ((d - md) ** 2).sum(axis=0) / (L - 1)
        S1, a1, S2 = d.sum(axis=0), np.abs(d).sum(axis=0), (d * d).sum(axis=0)
        dS1, dS2 = (L - 1) * U * a1, (L + 1) * U * S2
        dmean = dS1 / L + U * np.abs(S1 / L) + U * np.abs(mean)

        def var_bound(T1, T2, dT1, dT2, n, v):
            Q = T1 * T1 / n
            dQ = 2 * np.abs(T1) * dT1 / n + 2 * U * Q
            dN = dT2 + dQ + U * np.abs(T2 - Q)
            return dN / (n - 1) + U * v

        dvar = var_bound(S1, S2, dS1, dS2, L, var)
        # chains along axis 0: (M, E, ndim)
        mc = np.moveaxis(mean, 2, 1).reshape(M, mean.shape[1], ndim)
        vc = np.moveaxis(var, 2, 1).reshape(M, mean.shape[1], ndim)
        dmc = np.moveaxis(dmean, 2, 1).reshape(M, mean.shape[1], ndim)
        dvc = np.moveaxis(dvar, 2, 1).reshape(M, mean.shape[1], ndim)
        Wn = vc.sum(axis=0) / M
        Bn = ((mc - mc.mean(axis=0)) ** 2).sum(axis=0) / (M - 1)
        dWn = dvc.sum(axis=0) / M + (M - 1) * U * vc.sum(axis=0) / M + U * Wn
        dm = mc - mc[0]
        ddm = dmc + dmc[0] + U * np.abs(dm)
        T1, T2 = dm.sum(axis=0), (dm * dm).sum(axis=0)
        dT1 = ddm.sum(axis=0) + (M - 1) * U * np.abs(dm).sum(axis=0)
        dT2 = 2 * (np.abs(dm) * ddm).sum(axis=0) + (M + 1) * U * T2
        dBn = var_bound(T1, T2, dT1, dT2, M, Bn)
        A = LD(L - 1) / LD(L)
        R = Bn / Wn
        rhat = np.sqrt(A + R)
        dR = dBn / Wn + Bn * dWn / (Wn * Wn) + U * R
        drhat = (2 * U * A + U * R + dR) / (2 * rhat) + U * rhat
    return dict(mean=mean, var=var, rhat=rhat, dmean=dmean, dvar=dvar, drhat=drhat)


def assert_within_bounds(got_mean, got_var, got_rhat, ref, label=''):
    """Non-finite exactly where the definition is; elsewhere within the first-order bound.  Returns the worst ratio
    error / bound seen (0 / 0 counts as 0)."""
    worst = 0.0
    for name, got in (('mean', got_mean), ('var', got_var), ('rhat', got_rhat)):
        if got is None:
            continue
        want, bound = ref[name], ref['d' + name]
        fin = np.isfinite(want.astype(np.float64))
        np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=f'{label} {name}: finite where the definition is')
        with np.errstate(invalid='ignore'):
            err = np.abs(got.astype(LD) - want)[fin]
        b = bound[fin]
        assert (err <= b).all(), (label, name, float((err - b).max()), float(np.max(err / np.where(b > 0, b, 1))))
        if err.size:
            worst = max(worst, float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0))))
    return worst


def hand_built_chain(n, E, Wp, ndim, seed=0):
    """A chain (n, E * Wp, ndim): per (ensemble, parameter) a centre of size 0 ... 1e3 and a width 1e-8 ... 1e2 (parameter 0:
    centre 0), walkers offset from each other by a fraction of the width; a constant walker, a constant parameter,
    duplicated values; NaN, -NaN, +inf, -inf planted in chosen columns.  Returns (chain, centre (E, ndim), width (E,
    ndim))."""
    rng = np.random.default_rng(seed + n * 1000003 + E * 10007 + Wp * 101 + ndim)
    centre = rng.normal(size=(E, ndim)) * 10.0 ** rng.integers(-3, 4, (E, ndim))
    centre[:, 0] = 0.0
    width = 10.0 ** rng.integers(-8, 3, (E, ndim)).astype(np.float64)
    x = centre[None, :, None, :] + width[None, :, None, :] * (rng.normal(size=(n, E, Wp, ndim)) +
                                                              0.3 * rng.normal(size=(1, E, Wp, ndim)))
    if ndim > 1:
        x[:, E - 1, :, ndim - 1] = 0.25                  # a constant parameter: R-hat is NaN
    x[:, 0, Wp - 1, 0] = 0.25                            # a constant walker among moving ones: variance exactly 0
    if n >= 4 and Wp >= 3:                               # (with two walkers, one constant, R-hat would be inf)
        x[1::2, 0, 0, 0] = x[0:2 * (n // 2):2, 0, 0, 0][: len(x[1::2, 0, 0, 0])]      # duplicated values
    cols = [(e, w, q) for e in range(E) for w in range(Wp) for q in range(ndim)]
    if len(cols) >= 24 and ndim > 1:
        plants = [np.nan, -np.nan, np.inf, -np.inf]
        assert np.signbit(np.array([-np.nan]))[0]
        for i, value in enumerate(plants):
            e, w, q = cols[(7 + i * (len(cols) // 5)) % len(cols)]
            if q == 0:
                q = 1                                    # parameter 0 stays finite: the relative bound is asserted there
            x[(i * 3 + 1) % n, e, w, q] = value
    return x.reshape(n, E * Wp, ndim), centre, width
