"""PSIS-LOO on the CPU: the definitions of bisip_amd.loo against loop-written ones, the fit of the generalised Pareto
distribution on exact quantiles, the public pieces by hand, and the ordered restatement of the device's sums against the
long-double yardstick of tests/loo_bounds.py, which is itself held against mpmath on a few columns."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import loo_bounds as lb
from bisip_amd import fitquality as fq
from bisip_amd import loo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definitions against loops ---------------------------------------------------------------------------------------
def loop_gpd_fit(x):
    n = len(x)
    m = 30 + int(math.floor(math.sqrt(n)))
    xq = x[int(math.floor(n / 4 + 0.5)) - 1]
    b, L = [], []
    for j in range(1, m + 1):
        bj = 1 / x[n - 1] + (1 - math.sqrt(m / (j - 0.5))) / (3 * xq)
        kj = math.fsum(math.log1p(-bj * v) for v in x) / n
        b.append(bj)
        L.append(n * (math.log(-bj / kj) - kj - 1))
    w = [1 / math.fsum(math.exp(Li - Lj) for Li in L) for Lj in L]
    bp = math.fsum(bj * wj for bj, wj in zip(b, w))
    k = math.fsum(math.log1p(-bp * v) for v in x) / n
    return k * n / (n + 10) + 5 / (n + 10), -k / bp


def loop_column(q, M):
    R = len(q)
    s = sorted(q)
    qmax, u = s[R - 1], s[R - M - 1]
    tail = [v for v in s if v > u]
    n = len(tail)
    r = [math.exp((v - qmax) / 2) for v in tail]
    eu = math.exp((u - qmax) / 2)
    body = math.fsum(math.exp((v - qmax) / 2) for v in s if v <= u)
    if n <= 4:
        return -qmax / 2 + math.log(R) - math.log(body + math.fsum(r)), math.inf, math.nan, n
    khat, sigma = loop_gpd_fit([v - eu for v in r])
    w = [min(eu + sigma * math.expm1(-khat * math.log1p(-(j + 0.5) / n)) / khat, 1) for j in range(n)]
    elpd = -qmax / 2 + math.log((R - n) + math.fsum(wj / rj for wj, rj in zip(w, r))) - math.log(body + math.fsum(w))
    return elpd, khat, sigma, n


def loop_columns(q, reff=1.0):
    M = loo.tail_length(q.shape[0], reff)
    cols = [loop_column(list(q[:, c]), M) for c in range(q.shape[1])]
    return tuple(np.array([c[i] for c in cols], dtype=np.int64 if i == 3 else np.float64) for i in range(4))


def test_tail_length():
    want = {2: 1, 5: 1, 20: 4, 21: 5, 24: 5, 25: 5, 64: 13, 224: 45, 225: 45, 226: 46, 256: 48, 257: 49, 4096: 192,
            10000: 300, 128000: 1074}
    for R, M in want.items():
        assert loo.tail_length(R) == M and 1 <= M <= R - 1
    assert loo.tail_length(10500, 0.01) == 2100 and loo.tail_length(10000, 4.0) == 150
    for R in range(2, 400):
        assert 1 <= loo.tail_length(R) <= R - 1 and 1 <= loo.tail_length(R, 1e-6) <= R - 1
    for bad in (dict(R=1), dict(R=10, reff=0.0), dict(R=10, reff=-1.0), dict(R=10, reff=np.inf), dict(R=10, reff=np.nan)):
        with pytest.raises(ValueError):
            loo.tail_length(**bad)


@pytest.fixture(scope='module')
def families():
    return {kind.__name__: lb.build(kind, seed) for seed, kind in enumerate((lb.chi_square, lb.exponential, lb.quantised))}


def test_the_definition_is_the_loop(families):
    """The loop-written definition (math's functions, every sum exactly rounded by math.fsum: no less accurate than NumPy's
    pairwise sums) is held as anyone who computes the definition is: n_tail exact, the rest within the bounds of
    tests/loo_bounds.py."""
    for fam in families.values():
        for i, block in enumerate(fam.blocks):
            if block.shape[0] <= 4097:
                fam.check(i, loop_columns(block), 'loops')


def test_gpd_fit_is_the_loop():
    rng = np.random.default_rng(5)
    for n in (5, 8, 49, 300):
        x = np.sort(rng.pareto(2.0, size=n))
        got, want = loo.gpd_fit(x), loop_gpd_fit(list(x))
        # the same operations but for the order of the sums: n and m terms of one sign (log1p < 0, exp > 0), so n u and
        # m u relative; L = n (...) carries its rounding into exp(L_i - L_j) as an absolute n u |log|-sized error
        tol = 64 * n * lb.U * max(1.0, abs(want[0]))
        assert abs(got[0] - want[0]) <= tol and abs(got[1] - want[1]) <= tol * abs(want[1]) / max(1.0, abs(want[0])) + tol
    with pytest.raises(ValueError):
        loo.gpd_fit(np.zeros((2, 2)))
    khat, sigma = loo.gpd_fit(np.zeros(6))                              # a division by zero: reported, not raised
    assert np.isposinf(khat) and np.isnan(sigma)


@pytest.mark.parametrize('k', (-0.3, 0.2, 0.7, 1.2))
def test_gpd_fit_recovers_k_on_exact_quantiles(k):
    """x_j = sigma ((1 - p_j)^-k - 1) / k at p_j = (j + 0.5) / n are the quantiles of the distribution itself.  The prior
    pulls the estimate towards 0.5 with the weight of 10 observations: khat = (k n + 5) / (n + 10) = k + 10 (0.5 - k) / (n +
    10), the closed form of the shrinkage.  What is left is the midpoint rule's error on mean(log1p(-b x)), an integrand
    with a logarithmic end-point singularity at p -> 1: of order (1 + ln n) / n, which is allowed on top."""
    sigma = 2.0
    for n in (100, 1000, 20000):
        p = (np.arange(n) + 0.5) / n
        x = sigma * ((1 - p) ** -k - 1) / k
        khat, s = loo.gpd_fit(x)
        shrunk = (k * n + 5) / (n + 10)
        assert abs(shrunk - (k + 10 * (0.5 - k) / (n + 10))) < 1e-15
        assert abs(khat - shrunk) <= (1 + np.log(n)) / n
        assert abs(khat - k) <= 10 * abs(0.5 - k) / (n + 10) + (1 + np.log(n)) / n
        assert abs(s / sigma - 1) <= 4 * (1 + np.log(n)) / n * max(1.0, abs(k))


def test_psis_loo_columns_shapes_and_special_columns():
    rng = np.random.default_rng(2)
    q = rng.chisquare(1, size=(300, 2, 4))
    elpd, khat, sigma, n_tail = loo.psis_loo_columns(q)
    assert elpd.shape == khat.shape == sigma.shape == n_tail.shape == (2, 4) and n_tail.dtype == np.int64
    one = loo.psis_loo_columns(q[:, 1, 2])
    assert one[0].shape == () and one[0] == elpd[1, 2] and one[1] == khat[1, 2]
    # a constant column: nothing exceeds the threshold
    c = loo.psis_loo_columns(np.full((50, 1), 3.5))
    assert c[3][0] == 0 and np.isposinf(c[1][0]) and np.isnan(c[2][0]) and c[0][0] == -3.5 / 2
    # one NaN: its column alone
    dirty = q.copy()
    dirty[17, 0, 1] = np.nan
    d = loo.psis_loo_columns(dirty)
    assert np.isnan(d[0][0, 1]) and np.isnan(d[1][0, 1]) and np.isnan(d[2][0, 1]) and d[3][0, 1] == 0
    mask = np.ones((2, 4), bool)
    mask[0, 1] = False
    for a, b in zip(d, (elpd, khat, sigma, n_tail)):
        np.testing.assert_array_equal(a[mask], b[mask])
    # one huge outlier: eu underflows, the fit meets a division by zero, the plain sum remains
    out = q[:, 0, :1].copy()
    out[5, 0] = 4000.0
    o = loo.psis_loo_columns(out)
    assert o[3][0] == loo.tail_length(300) and np.isposinf(o[1][0]) and np.isfinite(o[0][0])
    assert abs(o[0][0] - (-2000.0 + np.log(300))) < 1e-12                    # exp(q / 2): the outlier is the whole sum
    for bad in (np.zeros(1), np.zeros((1, 3)), np.float64(1.0)):
        with pytest.raises(ValueError):
            loo.psis_loo_columns(bad)


def test_loo_of_log_likelihoods_is_loo_from_columns():
    """With sigma = 1 the log-likelihood is -q / 2 to the bit, so both roads take the same q."""
    rng = np.random.default_rng(3)
    R, N = 400, 5
    q = rng.chisquare(1, size=(R, 2, N)) * rng.uniform(0.5, 4, size=(2, N))
    ll = -0.5 * q - 0.0
    a = loo.loo(ll)
    elpd_rel, khat, _, n_tail = loo.psis_loo_columns(q)
    b = loo.loo_from_columns(elpd_rel, khat, n_tail, fq.fit_sums(q)[2], np.zeros((2, N)), R)
    assert set(a) == set(b) == {'elpd_loo', 'p_loo', 'looic', 'se', 'n_bad', 'k_threshold', 'elpd_i', 'p_loo_i', 'pareto_k',
                                'n_tail'}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert all(isinstance(a[k], float) for k in ('elpd_loo', 'p_loo', 'looic', 'se', 'k_threshold'))
    assert isinstance(a['n_bad'], int) and a['looic'] == -2 * a['elpd_loo']
    assert a['elpd_loo'] == a['elpd_i'].sum() and a['n_bad'] == (a['pareto_k'] > a['k_threshold']).sum()
    assert a['se'] == np.sqrt(2 * N * np.var(a['elpd_i']))
    # with error bars: elpd_i moves by -log sigma^2, p_loo_i not at all
    ls2 = rng.normal(size=(2, N))
    c = loo.loo_from_columns(elpd_rel, khat, n_tail, fq.fit_sums(q)[2], ls2, R)
    np.testing.assert_array_equal(c['elpd_i'], elpd_rel - ls2)
    np.testing.assert_allclose(c['p_loo_i'], b['p_loo_i'], rtol=0, atol=8 * lb.U * (np.abs(ls2) + np.abs(elpd_rel)).max())
    # leading axes are spectra
    e = loo.loo_from_columns(np.stack([elpd_rel] * 3), np.stack([khat] * 3), np.stack([n_tail] * 3),
                             np.stack([fq.fit_sums(q)[2]] * 3), ls2, R)
    assert e['elpd_loo'].shape == e['n_bad'].shape == (3,) and e['elpd_i'].shape == (3, 2, N)
    assert (e['elpd_loo'] == c['elpd_loo']).all()
    # leaving a point out cannot predict it better than keeping it in: importance weights that grow as the likelihood falls
    assert (a['p_loo_i'] > 0).all()
    with pytest.raises(ValueError):
        loo.loo(np.zeros(5))
    with pytest.raises(ValueError):
        loo.loo_from_columns(elpd_rel, khat, n_tail, np.zeros((3, N)), ls2, R)


def test_k_threshold():
    assert loo.k_threshold(100) == 0.5 and loo.k_threshold(1000) == 1 - 1 / 3
    assert loo.k_threshold(2200) == 0.7 and loo.k_threshold(128000) == 0.7
    assert abs(loo.k_threshold(2154) - (1 - 1 / np.log10(2154))) < 1e-15 and loo.k_threshold(2154) < 0.7
    assert loo.k_threshold(5) < 0                     # nothing is reliable from five samples
    with pytest.raises(ValueError):
        loo.k_threshold(1)


def test_compare_loo_by_hand():
    def result(elpd_i, n_bad):
        elpd_i = np.array(elpd_i, dtype=np.float64).reshape(2, 2)
        return dict(elpd_loo=float(elpd_i.sum()), p_loo=1.5, looic=-2 * float(elpd_i.sum()), se=0.25, n_bad=n_bad,
                    elpd_i=elpd_i)
    rows = loo.compare_loo({'a': result([-1, -2, -3, -4], 0), 'b': result([-1, -1, -1, -1], 2), 'c': result([-2, -2, -2, -2], 1)})
    assert [r['name'] for r in rows] == ['b', 'c', 'a']
    assert [r['d_elpd'] for r in rows] == [0.0, 4.0, 6.0] and rows[0]['d_se'] == 0.0
    assert rows[1]['d_se'] == 0.0                                           # a constant difference has no spread
    assert rows[2]['d_se'] == math.sqrt(4 * np.var([0.0, -1.0, -2.0, -3.0]))
    assert rows[0] == dict(name='b', elpd_loo=-4.0, p_loo=1.5, looic=8.0, se=0.25, n_bad=2, d_elpd=0.0, d_se=0.0)
    with pytest.raises(ValueError, match='nothing'):
        loo.compare_loo({})
    with pytest.raises(ValueError, match='same data'):
        loo.compare_loo({'a': result([-1, -2, -3, -4], 0), 'b': dict(result([-1, -2, -3, -4], 0), elpd_i=np.zeros((2, 3)))})
    with pytest.raises(ValueError, match='one spectrum'):
        loo.compare_loo({'a': dict(result([-1, -2, -3, -4], 0), elpd_loo=np.zeros(2))})


# -- the yardstick and the ordered restatement ----------------------------------------------------------------------------
def mp_column(q, M, mp):
    R = len(q)
    s = sorted(mp.mpf(float(v)) for v in q)
    qmax, u = s[R - 1], s[R - M - 1]
    tail = [v for v in s if v > u]
    n = len(tail)
    r = [mp.exp((v - qmax) / 2) for v in tail]
    eu = mp.exp((u - qmax) / 2)
    body = mp.fsum(mp.exp((v - qmax) / 2) for v in s if v <= u)
    x = [v - eu for v in r]
    m = 30 + int(mp.floor(mp.sqrt(n)))
    xq = x[int(math.floor(n / 4 + 0.5)) - 1]
    b = [1 / x[n - 1] + (1 - mp.sqrt(mp.mpf(m) / (j - mp.mpf(1) / 2))) / (3 * xq) for j in range(1, m + 1)]
    k = [mp.fsum(mp.log1p(-bj * v) for v in x) / n for bj in b]
    L = [n * (mp.log(-bj / kj) - kj - 1) for bj, kj in zip(b, k)]
    w = [1 / mp.fsum(mp.exp(Li - Lj) for Li in L) for Lj in L]
    bp = mp.fsum(bj * wj for bj, wj in zip(b, w))
    kp = mp.fsum(mp.log1p(-bp * v) for v in x) / n
    sigma = -kp / bp
    khat = kp * n / (n + 10) + mp.mpf(5) / (n + 10)
    wt = [min(eu + sigma * mp.expm1(-khat * mp.log1p(-(j + mp.mpf(1) / 2) / n)) / khat, mp.mpf(1)) for j in range(n)]
    elpd = -qmax / 2 + mp.log((R - n) + mp.fsum(a / c for a, c in zip(wt, r))) - mp.log(body + mp.fsum(wt))
    return elpd, khat, sigma, n


def test_the_yardstick_against_mpmath():
    """The long-double evaluation measures errors of the size of u = 1.1e-16: its own, against 50 digits, must lie far
    below -- a sixteenth of u is asked (long double carries 2^-64 = u / 2048)."""
    import mpmath as mp
    mp.mp.dps = 50
    for kind, R in ((lb.chi_square, 40), (lb.exponential, 225), (lb.quantised, 300), (lb.chi_square, 4097)):
        q = kind(R, 1, seed=11)
        ref = lb.yardstick(q)
        elpd, khat, sigma, n = mp_column(q[:, 0], loo.tail_length(R), mp.mp)
        assert n == ref['n_tail'][0] and n > 4
        for name, want in (('elpd', elpd), ('khat', khat), ('sigma', sigma)):
            hi = float(ref[name][0])
            got = mp.mpf(hi) + mp.mpf(float(ref[name][0] - lb.LD(hi)))           # the long double, exactly
            assert abs(got - want) <= lb.U / 16 * max(1, abs(want)), (kind.__name__, R, name)


def test_the_ordered_restatement_within_the_bounds(families):
    """loo.ordered_columns -- the device's order with NumPy's functions -- on every length at which a branch turns."""
    worst = {}
    for fam in families.values():
        ratios = [fam.check(i, loo.ordered_columns(block), 'ordered') for i, block in enumerate(fam.blocks)]
        worst[fam.name] = tuple(max(r[i] for r in ratios) for i in range(3))
        assert all(o > 0 for o in fam.own), 'the family has smoothed columns'
    print('ordered restatement / definition, worst (elpd_rel, khat, sigma):', worst)


def test_the_ordered_restatement_on_long_columns_and_with_reff():
    fam = lb.Family('chi-square, long', [lb.chi_square(128000, 2, 4)])
    fam.check(0, loo.ordered_columns(fam.blocks[0]))
    assert (fam.refs[0]['n_tail'] == 1074).all()
    fam = lb.Family('chi-square, reff = 0.01', [lb.chi_square(10500, 2, 5)], reff=0.01)
    fam.check(0, loo.ordered_columns(fam.blocks[0], 0.01))
    assert (fam.refs[0]['n_tail'] == 2100).all()                      # beyond the device's LDS capacity of 2048


def test_special_columns_in_the_device_order():
    q = np.stack([np.full(300, 2.25), lb.chi_square(300, 1, 1)[:, 0], lb.chi_square(300, 1, 2)[:, 0]], axis=1)
    q[7, 1] = np.nan
    q[9, 2] = 5000.0
    got, want = loo.ordered_columns(q), loo.psis_loo_columns(q)
    np.testing.assert_array_equal(got[3], want[3])
    np.testing.assert_array_equal(got[3], [0, 0, 52])
    assert got[0][0] == -2.25 / 2 and np.isposinf(got[1][0]) and np.isnan(got[2][0])
    assert all(np.isnan(g[1]) for g in got[:3])
    assert np.isposinf(got[1][2]) and np.isfinite(got[0][2]) and abs(got[0][2] - want[0][2]) <= 64 * lb.U * abs(want[0][2])


# -- plumbing -------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ('bisip_q_columns_dev', 'bisip_loo_columns_workspace', 'bisip_loo_columns_dev')


def test_entry_points_exist(hip_lib):
    import __graft_entry__ as entry
    from bisip_amd import _hip
    c = _hip.ctypes
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in NEW_ENTRIES:
        assert hasattr(hip_lib, name) and name in _hip.SYMBOLS
        assert re.search(r'\b%s\(' % name, header)
    assert _hip.SYMBOLS['bisip_q_columns_dev'] == (c.c_int, [c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p])
    assert _hip.SYMBOLS['bisip_loo_columns_workspace'] == (c.c_int64, [c.c_int64] * 3)
    assert _hip.SYMBOLS['bisip_loo_columns_dev'] == (c.c_int, [c.c_void_p] + [c.c_int64] * 3 + [c.c_void_p] * 5 + [
        c.c_int64, c.c_void_p])
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6
    assert callable(_hip.HipContext.q_columns_dev) and callable(_hip.loo_columns_dev) and callable(_hip.loo_columns_workspace)


def test_the_workspace_and_the_refusals_need_no_device(hip_lib):
    """The workspace is a formula of the shape; every refusal happens on the host before anything is launched, so the
    pointers (never dereferenced) may be anything."""
    from bisip_amd import _hip
    a256 = lambda x: (x + 255) & ~255
    for n, columns, M in ((2, 1, 1), (300, 7, 60), (128000, 64, 1074), (10500, 2, 2100)):
        chunks = -(-n // 4096)
        items = columns * M
        want = (a256(16 * columns) + 2 * a256(4 * columns) + a256(8 * columns * chunks) + 2 * a256(8 * items)
                + a256(a256(8 * items) + 16 * columns + 65536))
        assert _hip.loo_columns_workspace(n, columns, M) == want
    for n, columns, M in ((1, 1, 1), (10, 0, 2), (10, 1, 0), (10, 1, 10), (2 ** 33, 2 ** 20, 4096), (10 ** 6, 1, 51529),
                          (10, 2 ** 31, 1)):
        assert _hip.loo_columns_workspace(n, columns, M) < 0
    assert _hip.loo_columns_workspace(10 ** 6, 1, 51528) > 0
    ok = dict(q=4096, n=300, columns=2, M=60, elpd=4096, khat=4096, sigma=4096, ntail=4096, work=4096, nbytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        _hip.loo_columns_dev(a['q'], a['n'], a['columns'], a['M'], a['elpd'], a['khat'], a['sigma'], a['ntail'], a['work'],
                             a['nbytes'], 0)

    for match, kw in (('null', dict(q=0)), ('null', dict(work=0)), ('no output', dict(elpd=0, khat=0, sigma=0, ntail=0)),
                      ('bad shape', dict(n=1, M=1)), ('bad shape', dict(columns=0)), ('tail_len', dict(M=0)),
                      ('tail_len', dict(M=300)), ('workspace', dict(nbytes=1024)), ('aligned', dict(khat=4100))):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    for match, kw in (('profile points', dict(n=10 ** 6, M=51529)), ('2\\^31', dict(columns=2 ** 26, n=4096, M=64))):
        with pytest.raises(RuntimeError, match=match):                  # not supported, as opposed to wrong
            call(**kw)


def test_signatures():
    import bisip_amd
    sig = lambda f: str(inspect.signature(f))
    assert sig(loo.tail_length) == '(R, reff=1.0)' and sig(loo.gpd_fit) == '(x)' and sig(loo.k_threshold) == '(R)'
    assert sig(loo.psis_loo_columns) == sig(loo.ordered_columns) == '(q, reff=1.0)'
    assert sig(loo.loo) == '(log_lik, reff=1.0)' and sig(loo.compare_loo) == '(results)'
    assert sig(loo.loo_from_columns) == '(elpd_rel, khat, n_tail, lmeh, log_sigma2, R)'
    assert sig(loo.device_loo) == '(view, ctx, reff=1.0, first_spectrum=0)'
    for cls in (bisip_amd.PolynomialDecomposition, bisip_amd.PeltonColeCole, bisip_amd.Dias2000, bisip_amd.Shin2015):
        assert issubclass(cls, loo.ModelLoo)
        assert sig(cls.get_loo) == '(self, chain=None, reff=1.0, **kwargs)'
        assert 'get_loo' not in vars(cls) and 'get_loo' not in vars(bisip_amd.utils.utils)
    B = bisip_amd.SpectraBatch
    assert issubclass(B, loo.BatchLoo) and sig(B.get_loo) == '(self, discard=0, thin=1, reff=1.0)' and 'get_loo' not in vars(B)
    assert 'compare_loo' in loo.__all__ and not hasattr(bisip_amd, 'compare_loo')
    assert 'PSIS-LOO needs a sort' not in fq.__doc__ and 'get_loo' in fq.ModelFitQuality.get_waic.__doc__


def test_errors_of_an_unfitted_model():
    import bisip_amd
    m = bisip_amd.PeltonColeCole(bisip_amd.DataFiles()['SIP-K389175'], n_modes=1, nwalkers=8, nsteps=5)
    with pytest.raises(AssertionError, match='not fitted'):
        m.get_loo()
    chain = np.tile(0.5 * (m.param_bounds[0] + m.param_bounds[1]), (6, 1))
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_loo(chain=chain, discard=3)
    with pytest.raises(ValueError, match='reff'):
        m.get_loo(chain=chain, reff=0.0)
