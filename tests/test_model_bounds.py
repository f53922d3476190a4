"""Host checks of tests/model_bounds.py: the probe spectrum, the exact values and the rounding bound that
tests/test_gpu_model_exact.py holds the Cole-Cole / Dias / Shin kernels to.  No GPU: the CPU oracle (glibc doubles, the
reference's own arithmetic) stands where the kernels will."""

import numpy as np
import pytest

import model_bounds as mb
from model_bounds import LD, U, ULP

ROWSETS = [(model, D, loop, N) for model, D in mb.CASES for loop, N in mb.shapes(model, D)]


def _id(v):
    return '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


_cache = {}


def rowset(model, D, loop, N):
    """w, rows, exact values and the oracle's forward of one (model, loop) row set, computed once."""
    key = (model, D, loop, N)
    if key not in _cache:
        import oracle
        w = mb.frequencies(N, loop)
        th = mb.rows(model, D, w)
        ex = mb.exact(model, th, w)
        box = mb.default_box(model, D)
        prob = oracle.OracleProblem(model, w, np.zeros((2, N)), np.ones((2, N)), box, n_modes=D)
        _cache[key] = dict(w=w, th=th, ex=ex, box=box, Zo=oracle.forward(prob, th))
    return _cache[key]


def _oracle_probe(model, D, w, box, th, part, j, **kw):
    import oracle
    zn, zn_err = mb.probes(w, part, j)
    prob = oracle.OracleProblem(model, w, zn, zn_err, box, n_modes=D, **kw)
    return oracle.logprob(prob, th)


@pytest.mark.parametrize('model,D', mb.CASES + [('PolynomialDecomposition', 0)], ids=_id)
def test_the_probe_gives_back_one_residual_of_the_oracle_bit_for_bit(model, D):
    """sqrt(-2 logp) 2^-100 of a probe spectrum IS |oracle.forward| at the probed (part, frequency): 0 ulp, every row whose
    probed part dominates (all real parts; every imaginary part that is not at the subnormal scale)."""
    import oracle
    N = 17
    w = mb.frequencies(N, 'grid')
    rng = np.random.RandomState(5)
    kw = {}
    if model == 'PolynomialDecomposition':
        per = np.log10(1.0 / w)
        lt = np.linspace(np.floor(per.min() - 1), np.floor(per.max() + 1), 2 * N)
        kw = dict(taus=10 ** lt, log_taus=np.array([lt ** i for i in range(4)]), c_exp=1.0)
        box = np.array([[0.9] + [-1.0] * 4, [1.1] + [1.0] * 4])
        th = rng.uniform(box[0], box[1], (500, 5))
        th[:250, 1:] *= 1e-3
    else:
        box = mb.default_box(model, D)
        th = np.concatenate([mb.rows(model, D, w), rng.uniform(box[0], box[1], (244, box.shape[1]))])
    Zo = oracle.forward(oracle.OracleProblem(model, w, np.zeros((2, N)), np.ones((2, N)), box, n_modes=D, **kw), th)
    zmax = 2 * np.abs(Zo).max(axis=(1, 2))
    for part in (0, 1):
        for j in (0, 1, 7, 16):
            r, du = mb.recover(_oracle_probe(model, D, w, box, th, part, j, **kw), N, zmax)
            dom = du == 0
            assert dom.sum() >= (500 if part == 0 else 400), (part, j, dom.sum())
            assert np.array_equal(r[dom], np.abs(Zo[dom, part, j])), (part, j)
            # what does not dominate is small and is read to within du
            assert np.all(np.abs(r[~dom] - np.abs(Zo[~dom, part, j])) <= du[~dom])
            assert np.all(np.abs(Zo[~dom, part, j]) < 2.0 ** -60)


def test_a_probe_at_two_to_the_minus_forty_does_not_dominate():
    """The reason for sigma = 2^-100: at 2^-40 small imaginary parts stay below lconst and `recover` says so."""
    import oracle
    model, D, N = 'PeltonColeCole', 2, 17
    w = mb.frequencies(N, 'grid')
    box = mb.default_box(model, D)
    th = np.random.RandomState(6).uniform(box[0], box[1], (2000, 7))
    Zo = oracle.forward(oracle.OracleProblem(model, w, np.zeros((2, N)), np.ones((2, N)), box, n_modes=D), th)
    zn, zn_err = mb.probes(w, 1, 0, e=40)
    lp = oracle.logprob(oracle.OracleProblem(model, w, zn, zn_err, box, n_modes=D), th)
    r, du = mb.recover(lp, N, 2 * np.abs(Zo).max(axis=(1, 2)), e=40)
    assert (du > 0).sum() > 20
    r100, du100 = mb.recover(_oracle_probe(model, D, w, box, th, 1, 0), N, 2 * np.abs(Zo).max(axis=(1, 2)))
    assert np.all(du100 == 0) and np.array_equal(r100, np.abs(Zo[:, 1, 0]))


@pytest.mark.parametrize('rs', ROWSETS, ids=_id)
def test_the_bound_is_worth_having_and_the_reference_is_sharp(rs):
    """In the default boxes, on the asserted rows (edges included): bound <= 1e-13 of the unit for the residual path of every
    loop and for forward(); the long double's own error under 1/64 of it."""
    s = rowset(*rs)
    for path in ('residual', 'eval'):
        b = mb.bound(s['ex'], rs[2], path)
        assert np.all(np.isfinite(b)) and np.all(b > 0)
        mb.assert_bound_is_worth_having(s['ex'], b)
        mb.assert_reference_is_sharp(s['ex'], b)


@pytest.mark.parametrize('rs', ROWSETS, ids=_id)
def test_the_oracle_stays_inside_the_bound_with_glibc_constants(rs):
    """The reference's doubles, read through the probe at every frequency and part, lie within the bound of the
    one-reciprocal-per-term form with 1 ulp for each of glibc's functions; so does oracle.forward itself."""
    model, D, loop, N = rs
    s = rowset(*rs)
    ex, th, w = s['ex'], s['th'], s['w']
    b = mb.bound(ex, 'safe', 'eval', mb.GLIBC)
    assert mb.signed_excess(s['Zo'], ex, b).max() <= 1.0
    zmax = 2 * np.abs(s['Zo']).max(axis=(1, 2))
    unit = ex['unit'].astype(np.float64)
    got, du = np.empty((len(th), 2, N)), np.empty((len(th), 2, N))
    for part in (0, 1):
        for j in range(N):
            got[:, part, j], du[:, part, j] = mb.recover(_oracle_probe(model, D, w, s['box'], th, part, j), N, zmax)
    mb.assert_recovery_is_sharp(du, b, unit[:, None, :])
    worst = mb.excess(got, ex, b, du).max()
    print(f'{_id(rs)}: oracle through the probe, worst error / bound {worst:.3f}')
    assert worst <= 1.0


@pytest.mark.parametrize('rs', ROWSETS, ids=_id)
def test_a_value_displaced_by_the_parity_tolerance_is_rejected(rs):
    """What assert_Z_close lets through -- 1e-12 max(1, max|Z|) at a single frequency -- the bound of every loop rejects, on
    every row, in either part and in either direction: the defect the suite could not see."""
    model, D, loop, N = rs
    s = rowset(*rs)
    ex = s['ex']
    shift = 1e-12 * np.maximum(1.0, np.abs(s['Zo']).max(axis=(1, 2)))
    rng = np.random.RandomState(N)
    for path in ('residual', 'eval'):
        b = mb.bound(ex, loop, path)
        for part in (0, 1):
            j = rng.randint(N)
            for sign in (-1.0, 1.0):
                Z = s['Zo'].copy()
                Z[:, part, j] += sign * shift
                bad = mb.signed_excess(Z, ex, b)[:, part, j]
                assert bad.min() > 1.0, (path, part, j, sign, bad.min())
                if path == 'residual':                # as the probe reads it: the magnitude
                    assert mb.excess(np.abs(Z), ex, b)[:, part, j].min() > 1.0


def _mp(x):
    """A long double as an mpf, exactly (mantissa as a high and a low double; the exponent apart: below 1e-308 too)."""
    import mpmath as mp
    m, e = np.frexp(LD(x))
    hi = float(m)
    return mp.ldexp(mp.mpf(hi) + mp.mpf(float(m - LD(hi))), int(e))


@pytest.mark.parametrize('model,D', mb.CASES, ids=_id)
def test_long_double_agrees_with_fifty_digits(model, D):
    """exact() against the LITERAL formula of cython_funcs.pyx in 50-digit mpmath on every eighth asserted row (edges and
    uniform rows), five frequencies, both parts: within the long double's own error estimate."""
    w = mb.frequencies(5, 'fast')
    th = mb.rows(model, D, w)
    ex = mb.exact(model, th, w)
    worst = 0.0
    for r in list(range(0, 96)) + list(range(96, 256, 8)):
        zm = mb.exact_mp(model, th[r], w)
        for p in (0, 1):
            for j in range(5):
                d, e = abs(_mp(ex['Z'][r, p, j]) - zm[p][j]), _mp(ex['ref_err'][r, p, j])
                assert d <= e, (r, p, j, float(d / e))
                worst = max(worst, float(d / e))
    print(f'{model} {D}: long double / 50 digits, worst error / own estimate {worst:.3f}')


def test_the_unit_is_the_sum_of_the_terms_not_the_value():
    """The docstring's example: at sum m = 1 the constant part C = r0 - sum A cancels, at high frequency the terms are small,
    and |Z| is a thousandth of the unit.  A bound in |Z| would be false there: the reference's own doubles miss 1e-13 |Z|,
    and stay inside the bound in the unit."""
    import oracle
    w = mb.frequencies(5, 'fast')
    th = np.array([[1.05, 0.4, 0.6, 4.0, 3.0, 0.9, 0.8]])
    assert th[0, 1] + th[0, 2] == 1.0
    rng = np.random.RandomState(3)
    th = np.repeat(th, 64, axis=0)
    th[:, 0] = rng.uniform(0.9, 1.1, 64)
    ex = mb.exact('PeltonColeCole', th, w)
    j = int(np.argmax(w))
    absZ = np.hypot(*ex['Z'][:, :, j].T.astype(np.float64))
    unit = ex['unit'][:, j].astype(np.float64)
    assert np.all(absZ < 2e-3 * unit)
    b = mb.bound(ex, 'fast')
    assert np.all(b[:, 0, j] >= 2 * U * th[:, 0])                   # u r0 from C alone, times the slack
    assert np.all(b[:, 0, j] > 1e-13 * absZ)
    box = mb.default_box('PeltonColeCole', 2)
    Zo = oracle.forward(oracle.OracleProblem('PeltonColeCole', w, np.zeros((2, 5)), np.ones((2, 5)), box, n_modes=2), th)
    err = np.abs(Zo[:, 0, j].astype(LD) - ex['Z'][:, 0, j]).astype(np.float64)
    assert err.max() > 1e-13 * absZ.min() / 2                        # the reference itself, in units of |Z|
    assert mb.signed_excess(Zo, ex, mb.bound(ex, 'safe', 'eval', mb.GLIBC)).max() <= 1.0


def test_the_steps_of_the_grid_are_counted_per_q():
    """Quarter and step add q (dS1 + u) at q = f mod 16: nothing at the block start, 20.9 ulp at q = 15 from the roundings
    alone -- the "<= 22 ulp" of kernels.h -- and 30.1 ulp with the exponent's share (c2: 2u, its product with d: u) at c = 1 on
    33 frequencies (|c2 d| = 0.59)."""
    assert mb.grid_extra(0, 1.0) == 0.0
    assert abs(mb.grid_extra(15, 0.0) / ULP - 15 * (0.89 + 0.5)) < 1e-12
    assert mb.grid_extra(15, 0.0) / ULP <= 22.0
    w = mb.frequencies(33, 'grid')
    d = abs(np.log(w[-1] / w[0])) / 32
    assert 29.5 < mb.grid_extra(15, d / np.log(2.0)) / ULP < 30.5
    # the bound uses it: along a block the exponential's share grows by exactly that much
    th = mb.rows('PeltonColeCole', 1, w)[64:]
    ex = mb.exact('PeltonColeCole', th, w)
    mb.bound(ex, 'grid')
    de = ex['de'].astype(np.float64)
    a2d = (np.abs(th[:, 3]) / np.log(2.0) * d)[:, None, None]
    step = de[:, :, 17:32] - de[:, :, 16:31]
    assert np.all(step > 0)
    assert np.allclose(de[:, :, 31] - de[:, :, 16], mb.grid_extra(15, a2d)[:, :, 0], rtol=1e-6, atol=1e-22)


def test_the_reciprocal_of_every_frequency():
    """Which reciprocal serves a frequency (kernels.h): pairs (2k, 2k + 1) share rcp_joint, a last unpaired frequency and
    three and four modes take rcp_batch_n, the safe loop rcp_nr."""
    assert list(mb._rcp_ulps('PeltonColeCole', 1, 5, 'fast')) == [4.8] * 4 + [2.0]
    assert list(mb._rcp_ulps('PeltonColeCole', 2, 5, 'grid')) == [7.4] * 4 + [4.0]
    assert list(mb._rcp_ulps('PeltonColeCole', 2, 2, 'fast')) == [7.4] * 2
    assert list(mb._rcp_ulps('PeltonColeCole', 3, 5, 'fast')) == [6.0] * 5
    assert list(mb._rcp_ulps('PeltonColeCole', 4, 5, 'fast')) == [8.0] * 5
    assert list(mb._rcp_ulps('Shin2015', 2, 5, 'fast')) == [7.4] * 4 + [4.0]
    assert list(mb._rcp_ulps('Dias2000', 1, 5, 'fast')) == [4.0] * 4 + [2.0]
    for model, D in mb.CASES:
        assert list(mb._rcp_ulps(model, max(D, 1), 5, 'safe')) == [2.0] * 5
