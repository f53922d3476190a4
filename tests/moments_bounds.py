"""What tests/test_moments.py and tests/test_gpu_moments.py share: the long-double evaluation of np.mean / np.std over the
N = n * Wp values of an (ensemble, parameter), the first-order error bound of bisip_chain_moments_dev's two passes in any
summation order, and the hand-built chains both files run.

The bound.  u = 2^-53, x_1 ... x_N the values, mu and sigma^2 their exact mean and population variance, m the computed mean.
  Pass 0.  A sum of N values takes N - 1 additions that round, in whatever tree (an addition to a 0.0 that nothing was
      added to yet is exact), and a value passes through at most all of them: |ds| <= (N - 1) u sum|x|.  N = n * Wp is
      exact in binary64; the division rounds once:
          |m - mu| <= (N - 1) u sum|x| / N + u |mu| =: delta.
  Pass 1 sums the squares about m, not about mu.  Exactly, sum (x - m)^2 = N (sigma^2 + (m - mu)^2) =: N V.
      d = fl(x - m) = (x - m)(1 + e), |e| <= u, and it enters as d * d:                            2 u
      acc = fma(d, d, acc) rounds once, the product inside is exact.  A lane's first fma (onto 0.0) rounds as every
        later one does, so a chain of k values costs its first value k roundings; combining P partial sums that each
        hold a value costs at most P - 1 more, and k + P - 1 <= N.  All terms are >= 0:             N u
      the division by N:                                                                           1 u
      the square root: std = sqrt(v)(1 + e), so std^2 = v (1 + 2e):                                2 u
      the square that the test takes of std in binary64:                                           1 u
    so std^2 = V (1 + theta), |theta| <= (N + 6) u at first order, and with (m - mu)^2 <= delta^2
          |std^2 - sigma^2| <= delta^2 + (N + 6) u (sigma^2 + delta^2) =: dvar.
    delta^2 is second order in u but stays: for a posterior 1e-8 wide around 1e3 it is what tells the two-pass form,
    which pays delta^2 ~ 1e-26 on sigma^2 = 1e-16, from the one-pass form, which pays u mu^2 ~ 1e-10.
  NumPy's np.std rounds the product on its own (no fma): one u more, c = 7 instead of 6 (``c`` below).
Nothing above depends on the order of the sums.  Where sigma = 0 (a constant column) dvar = delta^2 (1 + (N + 6) u) is
still a bound on std^2, which is why the variance is compared and not the standard deviation relatively.

Range.  The model fl(a op b) = (a op b)(1 + e) needs results in binary64's normal range.  A column is ``checked`` (its
std^2 held to dvar) when all its values are finite, 4 N max|x|^2 < 2^1023 (no (x - m)^2 and no sum of them overflows)
and dvar >= 2^-1022: sums are exact among subnormals, so underflow adds at most 2^-1075 per value to the sum, that is
2^-1075 to the variance, and as much in the division and in the test's square -- below 2^-50 of such a dvar.  Long double
has a wider exponent range than binary64, so it gives sigma^2 = 1e-600 for a column of size 1e-300 where binary64 has 0,
and 1e320 for one of size 1e160 where binary64 has +inf: those columns are held to the stated order's bits and to
NumPy's result instead.  Their mean (and every finite column's) is within delta all the same.

The reference works on x - x_1, which is exact in long double wherever it matters (64-bit significand), so its own
rounding, N 2^-64 relative to sigma^2 and to |mu|, stays 2^-11 below the bound.
"""
import functools

import numpy as np

import chain_harness
from convergence_bounds import LD, U, hand_built_chain

# (n, E, Wp, ndim) of bisip_chain_moments_dev.  splits = max(1, min(ceil(4096 / E), n / 4)); lanes = (256 / ndim) * ndim.
MIRRORED = [
    (1, 1, 1, 1), (2, 1, 3, 1), (3, 2, 2, 2),          # fewer than four samples: the left-over loop only
    (4, 1, 5, 3), (5, 1, 5, 3),                        # one group of four; one group and one sample
    (7, 1, 5, 3), (8, 1, 5, 3), (9, 1, 5, 3),          # the last n with one split; two splits of four; 4 + 5
    (37, 1, 100, 4),                                   # nine splits: eight of four samples, one of five
    (5, 1, 85, 3), (5, 1, 86, 3),                      # exactly lanes = 255 doubles per sample, and one walker more
    (4, 1, 256, 1), (5, 1, 257, 1),                    # ndim 1: 256 lanes
    (8, 5, 19, 13),                                    # lanes = 247
    (12, 2, 33, 16),                                   # ndim = BISIP_MAX_NDIM
    (6, 3, 7, 9),                                      # fewer doubles than lanes
    (8, 4095, 1, 2), (8, 4096, 1, 2), (8, 4097, 1, 2),  # ceil(4096 / E): two splits up to E = 4095, one from 4096 on
]
BOUND_ONLY = [(64, 40, 256, 7), (600, 64, 64, 7)]      # no mirror: value by value in Python it would take minutes
SHAPES = MIRRORED + BOUND_ONLY
EXTREMES = {'tiny': (0, 1, 1e-140), 'huge': (0, 2, 1e160), 'vanishing': (1, 1, 1e-300)}     # name: (ensemble, parameter, size)
BOTH_INFINITIES = (1, 2)                               # (ensemble, parameter)


def has_extremes(E, ndim):
    return ndim >= 3 and E >= 2


def per_ensemble(x, E):
    """(n, E * Wp, ndim) -> (E, n * Wp, ndim): the values np.mean / np.std run over, axis 1."""
    n, W, ndim = x.shape
    return x.reshape(n, E, W // E, ndim).transpose(1, 0, 2, 3).reshape(E, n * (W // E), ndim)


def reference_and_bounds(x, E, c=6):
    """Long-double mean and population variance of every (ensemble, parameter) of x (n, E * Wp, ndim) and the bounds
    above: dict(mean, var, dmean, dvar) in long double, (E, ndim) each, ``finite`` (every value is) and ``checked``
    (std^2 is held to dvar) as boolean arrays, N."""
    v = per_ensemble(x, E)
    N = v.shape[1]
    with np.errstate(all='ignore'):
        ld = v.astype(LD)
        d = ld - ld[:, :1]
        md = d.sum(axis=1) / N
        mean = ld[:, 0] + md
        var = ((d - md[:, None]) ** 2).sum(axis=1) / N
        dmean = (N - 1) * U * np.abs(ld).sum(axis=1) / N + U * np.abs(mean)
        dvar = dmean ** 2 + (N + c) * U * (var + dmean ** 2)
        finite = np.isfinite(v).all(axis=1)
        amax = np.abs(ld).max(axis=1)
        checked = finite & (4 * N * amax * amax < LD(2) ** 1023) & (dvar >= LD(2) ** -1022)
    return dict(mean=mean, var=var, dmean=dmean, dvar=dvar, finite=finite, checked=checked, N=N)


def assert_within_bounds(mean, std, ref, label=''):
    """The mean of every finite column within delta, std^2 of every checked column within dvar; either may be None.
    Returns the worst ratio error / bound seen (0 / 0 counts as 0)."""
    worst = 0.0
    with np.errstate(all='ignore'):
        sq = None if std is None else std * std                       # the square is taken in binary64: it is in the bound
        for name, got, want, bound, where in (('mean', mean, ref['mean'], ref['dmean'], ref['finite']),
                                              ('std^2', sq, ref['var'], ref['dvar'], ref['checked'])):
            if got is None:
                continue
            assert got.shape == want.shape, (label, name, got.shape, want.shape)
            got = got.astype(LD)
            assert np.isfinite(got[where].astype(np.float64)).all(), (label, name, 'not finite where the values are')
            err, b = np.abs(got - want)[where], bound[where]
            assert (err <= b).all(), (label, name, float(np.max(err / np.where(b > 0, b, 1))))
            if err.size:
                worst = max(worst, float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0))))
    return worst


def assert_same_bits(got, want, what=''):
    """chain_harness.assert_same_bits, and NaN only where ``want`` has NaN, every infinity with its sign."""
    chain_harness.assert_same_bits(got, want, what)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(got[np.isinf(want)], want[np.isinf(want)], err_msg=what)


def assert_agrees_with_numpy(mean, std, ref, ref_numpy, np_mean, np_std, label=''):
    """NaN where NumPy has NaN, +inf / -inf / 0 where it has them; on the checked columns both are within their bounds
    of the same reference (NumPy's with c = 7), so they differ by at most the sum of the two."""
    for got, want in ((mean, np_mean), (std, np_std)):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=label)
        inf = np.isinf(want)
        np.testing.assert_array_equal(np.isinf(got), inf, err_msg=label)
        np.testing.assert_array_equal(got[inf], want[inf], err_msg=label)
    fin, chk = ref['finite'], ref['checked']
    with np.errstate(all='ignore'):
        assert (np.abs(mean.astype(LD) - np_mean.astype(LD))[fin] <= 2 * ref['dmean'][fin]).all(), label
        d2 = np.abs((std * std).astype(LD) - (np_std * np_std).astype(LD))
        assert (d2[chk] <= (ref['dvar'] + ref_numpy['dvar'])[chk]).all(), label
    unchecked = fin & ~chk                                            # squares outside binary64: +inf or 0, as NumPy
    np.testing.assert_array_equal(std[unchecked], np_std[unchecked], err_msg=label)


def moments_chain(n, E, Wp, ndim):
    """hand_built_chain -- centres 0 ... 1e3, widths 1e-8 ... 1e2, parameter 0 centred at 0 and finite, a constant walker,
    the constant parameter 0.25 of the last ensemble, duplicates, planted NaN, -NaN, +inf, -inf -- and, where the shape
    has room (has_extremes), whole (ensemble, parameter) columns of size 1e-140, 1e160 and 1e-300 and one that holds
    both infinities.  (n, E * Wp, ndim), read-only."""
    x = hand_built_chain(n, E, Wp, ndim)[0].reshape(n, E, Wp, ndim).copy()
    if ndim > 1:
        x[:, E - 1, :, ndim - 1] = 0.25                  # (a planted value may have landed in the constant parameter)
    if has_extremes(E, ndim):
        assert (E - 1, ndim - 1) not in [BOTH_INFINITIES] + [v[:2] for v in EXTREMES.values()]
        rng = np.random.default_rng(n + 7 * E + 11 * Wp + 13 * ndim)
        for e, q, size in EXTREMES.values():
            x[:, e, :, q] = size * (2.0 + rng.normal(size=(n, Wp)))
        e, q = BOTH_INFINITIES
        x[:, e, :, q] = rng.normal(size=(n, Wp))
        x[0, e, 0, q], x[n - 1, e, Wp - 1, q] = np.inf, -np.inf
    x = x.reshape(n, E * Wp, ndim)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(n, E, Wp, ndim):
    """dict(x, ref, ref_numpy, np_mean, np_std, ordered): the chain, its long-double reference with the kernel's bound
    and with NumPy's, np.mean / np.std of a host copy, and ordered_moments where the shape has a mirror (else None).
    Computed once per session and shared; nothing in it is written to."""
    from bisip_amd.chainview import ordered_moments
    x = moments_chain(n, E, Wp, ndim)
    v = per_ensemble(x, E)
    with np.errstate(all='ignore'):
        np_mean, np_std = v.mean(axis=1), v.std(axis=1)
    ref = reference_and_bounds(x, E)
    ref_numpy = dict(ref, dvar=ref['dmean'] ** 2 + (ref['N'] + 7) * U * (ref['var'] + ref['dmean'] ** 2))
    ordered = ordered_moments(x, E) if (n, E, Wp, ndim) in MIRRORED else None
    return dict(x=x, ref=ref, ref_numpy=ref_numpy, np_mean=np_mean, np_std=np_std, ordered=ordered)
