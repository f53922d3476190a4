"""What tests/test_loo.py and tests/test_gpu_loo.py share: the long-double evaluation of the definitions of bisip_amd.loo (per
column of R values q: the Pareto shape khat and scale sigma of the upper tail of the importance ratios exp(q / 2), and
elpd_rel, the log of the Pareto-smoothed leave-one-out sum), the bounds the device and the ordered restatement are held to,
and the families of columns.  u = 2^-53.  The columns q are doubles and ARE the data; the yardstick evaluates everything
from them in long double (tests/test_loo.py holds it against mpmath at 50 digits on a few columns).

Unsmoothed points (n_tail <= 4, or a khat that is not finite: khat = +inf, sigma = NaN on both sides, compared as such).
  elpd_rel = (-qmax / 2 + log R) - log S,  S = sum_i exp(a_i),  a_i = (q_i - qmax) / 2 <= 0:  an ABSOLUTE first-order bound.
  * a_i is a rounded difference halved (exact): an absolute error u |a_i| of the exponent is a relative one of the term.  The
    exp: K_exp u.  Every term is positive and travels through at most D additions, u each: |dS| <= u [(D + K_exp) S + sum_i
    |a_i| exp(a_i)].  D: the device adds a value of the body within its slot of a chunk (16), over 6 pairwise levels, 3 waves
    and the chunks, a value of the tail within its slot, 6 + 3 levels, and the body to the tail: D = 36 + ceil(R / 4096) +
    ceil(n_tail / 256).  NumPy's pairwise sum passes a term through fewer.
  * log S: |dS| / S + K_log u |log S|.  log R: K_log u log R.  -qmax / 2: exact.  The two additions: u |-qmax / 2 + log R| and
    u |elpd_rel|.
  delpd = u [D + K_exp + sum |a| e^a / S + K_log (|log S| + log R) + |-qmax / 2 + log R| + |elpd_rel|].
  K_exp, K_log as tests/fit_quality_bounds.py counts them (K_DEVICE, K_NUMPY).

Smoothed points.  khat passes through m softmax weights of profile likelihoods L_j = n (...), each a difference of logs
scaled by n: the weighted b resists a first-order bound that is not orders of magnitude above what any implementation
does.  No tolerance is invented.  Instead the float64 NumPy definition (loo.psis_loo_columns: glibc's exp / log1p / expm1,
pairwise sums) is measured against the same yardstick over the same family of columns, and whoever else computes the
definition -- the device, the ordered restatement -- is allowed FACTOR = 16 times the definition's own worst error over
that family, in khat (absolute), sigma (relative) and elpd_rel (absolute).  The factor covers a device exp / log1p / expm1
of a couple of ulp where glibc has one (fit_quality_bounds: 3 + 1 against 1 + 1) and a summation tree of another shape.
The bound so comes from the reference's own error and the number formats, never from what the code under test gives.
"""
import numpy as np

from bisip_amd import loo
from convergence_bounds import LD, U
from fit_quality_bounds import K_DEVICE, K_NUMPY      # noqa: F401  (shared with the tests)

FACTOR = 16


# -- the yardstick ---------------------------------------------------------------------------------------------------------
def gpd_fit_ld(x):
    """loo.gpd_fit in long double: (khat, sigma), (+inf, NaN) when khat is not finite."""
    n = x.size
    with np.errstate(all='ignore'):
        m = 30 + int(np.floor(np.sqrt(n)))
        j = np.arange(1, m + 1).astype(LD)
        b = LD(1) / x[n - 1] + (LD(1) - np.sqrt(LD(m) / (j - LD(0.5)))) / (LD(3) * x[int(np.floor(n / 4 + 0.5)) - 1])
        k = np.log1p(-b[:, None] * x).sum(axis=1) / LD(n)
        L = LD(n) * (np.log(-b / k) - k - LD(1))
        w = LD(1) / np.exp(L - L[:, None]).sum(axis=1)
        b_post = (b * w).sum()
        k_post = np.log1p(-b_post * x).sum() / LD(n)
        sigma = -k_post / b_post
        khat = k_post * LD(n) / LD(n + 10) + LD(5) / LD(n + 10)
    if not np.isfinite(khat):
        return LD(np.inf), LD(np.nan)
    return khat, sigma


def column_ld(q, M, K=K_DEVICE, fit=True):
    """One column in long double: dict(elpd, khat, sigma, n_tail, delpd); delpd is the first-order bound of the module's
    docstring, meaningful where khat is +inf.  fit=False: nothing is fitted -- the yardstick of a column whose eu underflows
    in double (and the fit with it: khat = +inf by the definition's rule) but not in long double."""
    R = q.size
    nan = LD(np.nan)
    if np.isnan(q).any():
        return dict(elpd=nan, khat=nan, sigma=nan, n_tail=0, delpd=nan)
    K_exp, K_log = K
    with np.errstate(all='ignore'):
        s = np.sort(q).astype(LD)
        qmax, u = s[R - 1], s[R - M - 1]
        tail = s[s > u]
        n = tail.size
        a = (s - qmax) / 2
        r = np.exp(a)
        r_tail, eu = r[R - n:], np.exp((u - qmax) / 2)
        khat, sigma = LD(np.inf), nan
        if fit and n >= loo.MIN_TAIL:
            khat, sigma = gpd_fit_ld(r_tail - eu)
        body = r[:R - n].sum()
        if np.isfinite(khat):
            p = (np.arange(n).astype(LD) + LD(0.5)) / LD(n)
            w = np.minimum(eu + sigma * np.expm1(-khat * np.log1p(-p)) / khat, LD(1))
            ratio = (w / r_tail).sum()
        else:
            w, ratio = r_tail, LD(n)
        S = body + w.sum()
        first = -qmax / 2 + np.log(LD(R - n) + ratio)
        elpd = first - np.log(S)
        D = 36 + -(-R // loo.CHUNK) + -(-n // loo.SLOTS)
        delpd = U * (D + K_exp + (np.abs(a) * r).sum() / r.sum() + K_log * (np.abs(np.log(S)) + np.log(LD(R))) + np.abs(first)
                     + np.abs(elpd))
    return dict(elpd=elpd, khat=khat, sigma=sigma, n_tail=n, delpd=delpd)


def yardstick(q, reff=1.0, K=K_DEVICE):
    """The columns q (R, C) in long double: dict of elpd, khat, sigma, delpd (long double) and n_tail (int64), (C,) each."""
    q = np.asarray(q, dtype=np.float64)
    M = loo.tail_length(q.shape[0], reff)
    cols = [column_ld(q[:, c], M, K) for c in range(q.shape[1])]
    out = {k: np.array([c[k] for c in cols], dtype=LD) for k in ('elpd', 'khat', 'sigma', 'delpd')}
    out['n_tail'] = np.array([c['n_tail'] for c in cols], dtype=np.int64)
    return out


# -- errors and bounds ------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """(elpd, khat, sigma) errors of got = (elpd_rel, khat, sigma, n_tail) against a yardstick over the SMOOTHED columns
    (khat finite in the yardstick): absolute, absolute, relative; the worst of each, 0.0 where there is none."""
    sm = np.isfinite(ref['khat'].astype(np.float64))
    if not sm.any():
        return 0.0, 0.0, 0.0
    e = np.abs(got[0][sm].astype(LD) - ref['elpd'][sm]).max()
    k = np.abs(got[1][sm].astype(LD) - ref['khat'][sm]).max()
    s = (np.abs(got[2][sm].astype(LD) - ref['sigma'][sm]) / np.abs(ref['sigma'][sm])).max()
    return float(e), float(k), float(s)


class Family:
    """Columns of one kind, in blocks (R, C) of several lengths, their yardsticks, and the definition's own worst errors
    against them: what FACTOR multiplies."""

    def __init__(self, name, blocks, reff=1.0):
        self.name, self.blocks, self.reff = name, [np.ascontiguousarray(b, dtype=np.float64) for b in blocks], reff
        self.refs = [yardstick(b, reff) for b in self.blocks]
        self.defs = [loo.psis_loo_columns(b, reff) for b in self.blocks]   # the float64 definition itself
        own = [errors(d, ref) for d, ref in zip(self.defs, self.refs)]
        self.own = tuple(max(o[i] for o in own) for i in range(3))          # (elpd, khat, sigma)

    @property
    def allowed(self):
        return tuple(FACTOR * v for v in self.own)

    def check(self, i, got, what=''):
        """got = (elpd_rel, khat, sigma, n_tail) of block i: n_tail the definition's; unsmoothed columns: khat = +inf, sigma NaN and
        elpd_rel within the first-order bound; smoothed columns within FACTOR times the definition's own worst error.
        Returns the errors / the definition's own worst, (elpd, khat, sigma)."""
        ref = self.refs[i]
        what = f'{self.name} block {i} {what}'
        np.testing.assert_array_equal(got[3], self.defs[i][3], err_msg=what)           # the definition's, and the yardstick's
        np.testing.assert_array_equal(got[3], ref['n_tail'], err_msg=what)
        kref = ref['khat'].astype(np.float64)
        nanc = np.isnan(kref)
        for a in got[:3]:
            assert np.isnan(a[nanc]).all(), what
        un = np.isposinf(kref)
        assert np.isposinf(got[1][un]).all() and np.isnan(got[2][un]).all(), what
        assert (np.abs(got[0].astype(LD) - ref['elpd'])[un] <= ref['delpd'][un]).all(), what
        assert np.isfinite(got[1][~un & ~nanc]).all(), what
        err = errors(got, ref)
        for e, allowed, name in zip(err, self.allowed, ('elpd_rel', 'khat', 'sigma')):
            assert e <= allowed, f'{what}: {name} off by {e:.3e}, {FACTOR} x the definition\'s own {allowed / FACTOR:.3e}'
        return tuple(e / o if o else 0.0 for e, o in zip(err, self.own))


# -- the families -----------------------------------------------------------------------------------------------------------
# the smallest lengths at which each branch turns: n_tail <= 4 (2, 5, 20), the first fitted tails (21, 24, 25, 64), R / 5
# against 3 sqrt(R) (224, 225, 226), the slots of a workgroup (256, 257), the compaction chunk (4095, 4096, 4097), and 10,000
LENGTHS = (2, 5, 20, 21, 24, 25, 64, 224, 225, 226, 256, 257, 4095, 4096, 4097, 10000)
COLUMNS = 3


def chi_square(R, C, seed):
    """q of a well-specified point: chi-square with one degree of freedom, times a scale of the column's own."""
    rng = np.random.default_rng([seed, R])
    return rng.chisquare(1, size=(R, C)) * rng.uniform(0.5, 3.0, size=C)


def exponential(R, C, seed, k=0.8):
    """Importance ratios exp(q / 2) that ARE Pareto with shape k: q = 2 k E, E standard exponential."""
    return 2 * k * np.random.default_rng([seed, R, 1]).exponential(size=(R, C))


def quantised(R, C, seed):
    """Chi-square rounded to a grid of 1 / 4 and capped at 6: ties at the threshold, so n_tail < M (a cap so low that the
    cap itself is the threshold makes n_tail = 0)."""
    return np.minimum(np.round(chi_square(R, C, seed) * 4) / 4, 6.0)


def build(kind, seed, lengths=LENGTHS, C=COLUMNS, reff=1.0):
    return Family(kind.__name__, [kind(R, C, seed) for R in lengths], reff)
