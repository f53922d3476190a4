"""bisip_reduced_emulate -- the host emulation of logprob_row_reduced<P, COMP> (host_emulate.inc: chi2_kernel, the
arithmetic every estimate behind BISIP_VARIANT_AUTO is measured on) -- against an independent statement of the same
sequence in exact rational arithmetic: every operation is computed exactly with fractions.Fraction and rounded to
double ONCE (float(Fraction) rounds to nearest, ties to even), an fma is one rounding of the exact a*b + c, and
infinities, NaN and the sign of zero follow IEEE 754.  The statement is written from the comment at
logprob_row_reduced (kernels.h), not from the emulation.  No GPU, no tolerance: equality of bits.
tests/test_gpu_reduced_bits.py then holds the kernels to the emulation."""

import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import golden_cases

INF = float('inf')


# ---------------------------------------------------------------------------------------------------------
# IEEE binary64, one operation at a time, from exact rationals
# ---------------------------------------------------------------------------------------------------------
def _neg(x):
    return math.copysign(1.0, x) < 0


def _rnd(x):
    """The double nearest to the nonzero rational x: overflow goes to an infinity, underflow keeps the sign."""
    try:
        r = float(x)
    except OverflowError:
        return -INF if x < 0 else INF
    return math.copysign(0.0, -1.0 if x < 0 else 1.0) if r == 0.0 else r


def add(a, b):
    if not (math.isfinite(a) and math.isfinite(b)):
        return a + b                      # inf + x = inf, inf - inf = NaN, NaN stays
    x = Fraction(a) + Fraction(b)
    if x == 0:                            # -0 only from (-0) + (-0); x + (-x) = +0
        return -0.0 if (a == 0.0 and b == 0.0 and _neg(a) and _neg(b)) else 0.0
    return _rnd(x)


def sub(a, b):
    return add(a, -b)


def mul(a, b):
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b                      # inf * 0 = NaN
    x = Fraction(a) * Fraction(b)
    if x == 0:
        return -0.0 if _neg(a) != _neg(b) else 0.0
    return _rnd(x)


def fma(a, b, c):
    """One rounding of the exact a*b + c."""
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b + c                  # the product is inf or NaN: (+-inf) + c as IEEE has it
    if not math.isfinite(c):
        return c                          # the exact product is finite
    p = Fraction(a) * Fraction(b)
    x = p + Fraction(c)
    if x == 0:
        if p == 0 and c == 0.0:           # a sum of two zeros: -0 only when both are
            return -0.0 if (_neg(a) != _neg(b)) and _neg(c) else 0.0
        return 0.0
    return _rnd(x)


def two_diff(a, b):
    """a - b = s + err (Knuth's TwoSum on a and -b), six operations."""
    s = sub(a, b)
    bb = sub(s, a)
    return s, add(sub(a, sub(s, bb)), sub(-b, bb))


# ---------------------------------------------------------------------------------------------------------
# the sequence documented at logprob_row_reduced
# ---------------------------------------------------------------------------------------------------------
def statement(ops, lo, hi, th):
    """One row.  ops: comp, R (packed upper triangle, row-major), Rlo, bhat, e, elo, rest, lconst."""
    n = len(ops['bhat'])
    th = [float(t) for t in th]
    R, bhat, e = [float(x) for x in ops['R']], [float(x) for x in ops['bhat']], [float(x) for x in ops['e']]
    chi2 = float(ops['rest'])
    if not ops['comp']:
        d = [sub(bhat[0], th[0])] + [sub(bhat[q], mul(th[0], th[q])) for q in range(1, n)]
        k = 0
        for i in range(n):
            u = e[i]
            for j in range(i, n):
                u = fma(R[k], d[j], u)
                k += 1
            chi2 = fma(u, u, chi2)
    else:
        Rlo, elo = [float(x) for x in ops['Rlo']], [float(x) for x in ops['elo']]
        d, dl = [0.0] * n, [0.0] * n
        d[0], dl[0] = two_diff(bhat[0], th[0])                # d + dl = bhat - b exactly
        for q in range(1, n):
            p = mul(th[0], th[q])
            pe = fma(th[0], th[q], -p)                        # TwoProduct
            d[q], err = two_diff(bhat[q], p)                  # TwoSum
            dl[q] = sub(err, pe)
        k = 0
        for i in range(n):
            s, c = e[i], elo[i]
            for j in range(i, n):                             # Dot2 row, then the first-order terms
                h = mul(R[k], d[j])
                low = fma(R[k], d[j], -h)
                t = add(s, h)
                bb = sub(t, s)
                er = add(sub(s, sub(t, bb)), sub(h, bb))
                s = t
                c = add(c, add(er, low))
                c = fma(R[k], dl[j], c)
                c = fma(Rlo[k], d[j], c)
                k += 1
            u = add(s, c)
            chi2 = fma(u, u, chi2)                            # the square by fma
    lp = fma(-0.5, chi2, float(ops['lconst']))
    inside = all(float(lo[q]) < th[q] < float(hi[q]) for q in range(n))     # open box; NaN compares false
    return lp if inside else -INF


def assert_same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), 'NaN rows differ'
    bad = np.flatnonzero(got[~nan].view(np.int64) != want[~nan].view(np.int64))
    assert bad.size == 0, (f'{bad.size} rows differ, first at {bad[0]}: '
                           f'{got[~nan][bad[0]].hex()} != {want[~nan][bad[0]].hex()}')


# ---------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------
PD_CASE = [p for p in golden_cases() if 'PolynomialDecomposition' in p][0]
_OPS = {}


def operands(n, comp):
    """Plain tier: polydecomp_operands of a golden case's spectrum at degree n - 2.  Compensated tier: the same plus a
    synthetic low word of the triangle (floats of at most 11 significant bits below ulp(R)/2) and of e (below ulp(e)/2)."""
    from bisip_amd import _hip
    if n not in _OPS:
        g = np.load(PD_CASE)
        lt = np.log10(g['taus'])
        log_taus = np.array([lt ** i for i in range(n - 1)])
        o = _hip.polydecomp_operands(g['w'], g['zn'], g['zn_err'], g['taus'], log_taus, float(g['c_exp']))
        assert np.all(np.tril(o['R'], -1) == 0)
        R = o['R'][np.triu_indices(n)]                         # row-major upper triangle
        rng = np.random.RandomState(1000 + n)
        m = rng.randint(-2047, 2048, R.size)                   # 11 bits and a sign
        Rlo = (m / 2048.0 * (np.spacing(np.abs(R)) / 2)).astype(np.float32)
        assert np.all(Rlo.astype(np.float64) == m / 2048.0 * (np.spacing(np.abs(R)) / 2))     # floats hold them exactly
        assert np.any(Rlo != 0)
        elo = rng.uniform(-0.5, 0.5, n) * np.spacing(np.abs(o['e']))
        _OPS[n] = dict(R=R, Rlo=Rlo, bhat=o['bhat'], e=o['e'], elo=elo, rest=o['rest'], lconst=o['lconst'])
    ops = dict(_OPS[n], comp=comp)
    if not comp:
        ops['Rlo'] = ops['elo'] = None
    return ops


def default_box(n):
    return np.array([[0.9] + [-1.0] * (n - 1), [1.1] + [1.0] * (n - 1)])


def edge_rows(lo, hi, rng):
    """On a bound, outside, NaN, +-inf, -0.0 coefficients."""
    n = lo.size
    rows = []

    def base():
        return rng.uniform(lo, hi)
    for q in (0, 1, n - 1):
        for bound in (lo, hi):
            r = base(); r[q] = bound[q]; rows.append(r)                              # on a bound
            r = base(); r[q] = bound[q] + (hi[q] - lo[q]) * (1 if bound is hi else -1); rows.append(r)   # outside
            r = base(); r[q] = np.nextafter(bound[q], 0.5 * (lo[q] + hi[q])); rows.append(r)  # the last value inside
        for bad in (np.nan, np.inf, -np.inf):
            r = base(); r[q] = bad; rows.append(r)
    r = base(); r[1:] = -0.0; rows.append(r)
    r = base(); r[1:] = 0.0; rows.append(r)
    r = base(); r[1::2] = -0.0; rows.append(r)
    rows.append(np.full(n, np.nan))
    return np.array(rows)


@pytest.mark.parametrize('comp', [False, True], ids=['plain', 'comp'])
@pytest.mark.parametrize('n', [2, 3, 7, 12])
def test_emulation_is_the_documented_sequence_bit_for_bit(n, comp):
    from bisip_amd import _hip
    ops = operands(n, comp)
    box = default_box(n)
    rng = np.random.RandomState(7 * n + comp)
    theta = rng.uniform(box[0], box[1], (100, n))
    theta[:30, 1:] *= 1e-2                     # small coefficients: where a decent fit lies
    theta[30:40] = np.r_[ops['bhat'][0], ops['bhat'][1:] / ops['bhat'][0]] * (1 + 1e-9 * rng.randn(10, n))   # at the expansion point: the sums cancel
    edges = edge_rows(box[0], box[1], rng)
    theta = np.vstack([theta, edges])
    got = _hip.reduced_emulate(ops, box, theta)
    want = np.array([statement(ops, box[0], box[1], th) for th in theta])
    assert np.isfinite(want[:30]).all() and np.isneginf(want[100:]).sum() >= 20      # both sides of the prior
    assert_same_bits(got, want)


@pytest.mark.parametrize('comp', [False, True], ids=['plain', 'comp'])
def test_emulation_overflows_as_ieee_does(comp):
    """A box so wide that the sums of in-prior rows overflow: chi^2 = inf, and inf - inf = NaN inside a row.  The width
    is B = 10 sqrt(DBL_MAX): a product theta_0 theta_q near the edge is itself infinite, d = bhat - b with it, and the
    terms R d of a row are infinities of either sign (with finite d the plain tier's fused terms never meet inf - inf:
    the product inside an fma is exact).  From the plain operands: a square (max|R| theta^2)^2 stays below DBL_MAX
    `fin` decades below B.  A third of the rows lie within half a decade of the edge, a third between there and
    `fin` (sums or squares overflow: inf), a third 2 to 40 decades below `fin` (finite)."""
    from bisip_amd import _hip
    n = 7
    ops = operands(n, comp)
    big = float(np.finfo(np.float64).max)
    B = 10.0 * math.sqrt(big)
    fin = math.log10(B) - 0.5 * math.log10(math.sqrt(big) / np.abs(ops['R']).max())
    assert 40 < fin < 150
    box = np.array([[-B] * n, [B] * n])
    rng = np.random.RandomState(11 + comp)
    decades = np.r_[rng.uniform(0.0, 0.5, 40), rng.uniform(0.5, fin, 40), rng.uniform(fin + 2, fin + 40, 40)][:, None]
    theta = rng.choice([-1.0, 1.0], (120, n)) * B * 10.0 ** -decades * rng.uniform(0.1, 1.0, (120, n))
    inside = np.all((box[0] < theta) & (theta < box[1]), axis=1)
    assert inside.all()
    want = np.array([statement(ops, box[0], box[1], th) for th in theta])
    assert np.isfinite(want).sum() >= 5 and np.isinf(want).sum() >= 5 and np.isnan(want).sum() >= 5, \
        (np.isfinite(want).sum(), np.isinf(want).sum(), np.isnan(want).sum())
    assert_same_bits(_hip.reduced_emulate(ops, box, theta), want)


def test_emulate_entry_point_refuses_bad_arguments(hip_lib):
    from bisip_amd import _hip
    n = 3
    ops = operands(n, True)
    box = default_box(n)
    theta, out = np.full((2, n), 0.5), np.empty(2)
    fp, dp = ctypes.POINTER(ctypes.c_float), _hip._dp

    def call(n=n, comp=1, R=ops['R'], Rlo=ops['Rlo'], bhat=ops['bhat'], e=ops['e'], elo=ops['elo'], lo=box[0].copy(),
             hi=box[1].copy(), theta=theta, W=2, out=out):
        def p(a, t=dp):
            return None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)
        return hip_lib.bisip_reduced_emulate(n, comp, p(R), p(Rlo, fp), p(bhat), p(e), p(elo), ops['rest'], ops['lconst'],
                                             p(lo), p(hi), p(theta), W, p(out))
    assert call() == 0 and call(comp=0, Rlo=None, elo=None) == 0 and call(W=0, theta=None, out=None) == 0
    for bad in (dict(R=None), dict(bhat=None), dict(e=None), dict(lo=None), dict(hi=None), dict(theta=None), dict(out=None),
                dict(n=1), dict(n=13), dict(n=-3), dict(Rlo=None), dict(elo=None), dict(comp=2), dict(comp=-1), dict(W=-1)):
        assert call(**bad) == -1, bad                          # BISIP_EINVAL
        assert hip_lib.bisip_last_error()
    with pytest.raises(ValueError):
        _hip.reduced_emulate(dict(ops, R=ops['R'][:-1]), box, theta)
    with pytest.raises(ValueError):
        _hip.reduced_emulate(ops, default_box(n + 1), theta)
    with pytest.raises(ValueError):
        _hip.reduced_emulate(dict(ops, Rlo=None), box, theta)
