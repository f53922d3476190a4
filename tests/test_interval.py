"""bisip_amd.interval on the host: the definition of the highest-density interval against a brute-force loop over all
windows and against hand-made columns whose answer is known, the refusals of ``windows``, the plan and the workspace of the
entry point, its refusals, and the methods of a model with a host sampler."""
import os
import re

import numpy as np
import pytest

from bisip_amd import interval as iv
from fitted import fitted_on_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(col, K):
    """(lo, hi, i*) of one column by the definition, one window after the other."""
    if np.isnan(col).any():
        return np.nan, np.nan, 0
    s = np.sort(col)
    best, at = None, 0
    for i in range(s.size - K):
        with np.errstate(all='ignore'):
            w = s[i + K] - s[i]
        if np.isnan(w):
            w = np.inf
        if best is None or w < best:
            best, at = w, i
    return s[at], s[at + K], at


def same(got, want):
    """Equal, and NaN where the definition gives NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), (got, want)


# -- the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 2, 1), (1, 1, 3, 1), (5, 3, 2, 2), (13, 2, 7, 3), (40, 1, 5, 4)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('mass', [0.5, 0.9, 0.95, (0.5, 0.9, 0.95)], ids=str)
def test_hdi_against_brute_force(shape, mass):
    n, E, Wp, ndim = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.normal(size=(n, E * Wp, ndim)) * rng.exponential(size=ndim)
    x = np.round(x, 1) if n > 5 else x                      # duplicates: ties among the widths
    N = n * Wp
    got, idx = iv.hdi(x, mass, E, index=True)
    masses = np.atleast_1d(mass)
    Ks = iv.windows(mass, N)
    assert idx.dtype == np.int64
    if np.ndim(mass):
        assert got.shape == (masses.size, 2, E, ndim) and idx.shape == (masses.size, E, ndim)
    else:
        assert got.shape == (2, E, ndim) and idx.shape == (E, ndim)
        got, idx = got[None], idx[None]
    for k, K in enumerate(Ks):
        assert K == int(np.floor(masses[k] * N))
        for e in range(E):
            rows = x[:, e * Wp:(e + 1) * Wp].reshape(N, ndim)            # get_chain(flat=True)'s order
            for q in range(ndim):
                lo, hi, at = brute_force(rows[:, q], int(K))
                assert (got[k, 0, e, q], got[k, 1, e, q], idx[k, e, q]) == (lo, hi, at)
    assert (got[:, 0] <= got[:, 1]).all()                   # lo <= hi for finite columns
    if E == 1:
        same(iv.hdi(x.reshape(N, ndim), mass), iv.hdi(x, mass))          # flat, one ensemble


def test_hand_made_columns():
    # skewed: the mass sits at the low end, the HDI starts at the minimum; the equal-tailed interval does not
    skew = np.concatenate([np.linspace(0.0, 1.0, 90), np.linspace(2.0, 100.0, 10)])
    (lo, hi), i = iv.hdi(skew[:, None], 0.9, index=True)
    assert (lo[0, 0], hi[0, 0], i[0, 0]) == (0.0, 2.0, 0)
    p = np.percentile(skew, [5.0, 95.0])
    assert p[0] > lo[0, 0] and p[1] > hi[0, 0] and hi[0, 0] - lo[0, 0] < p[1] - p[0]
    p = np.percentile(skew, [2.5, 97.5])
    out = iv.hdi(skew[:, None], 0.95)
    assert out[0, 0, 0] == 0.0 and out[0, 0, 0] != p[0] and out[1, 0, 0] != p[1]
    # two windows of exactly equal width (K = 2: [0, 2] at i = 0 and [6, 8] at i = 3): the lower i wins
    tie = np.array([8.0, 0.0, 6.0, 1.0, 7.0, 2.0, 20.0, 40.0])
    (lo, hi), i = iv.hdi(tie[:, None], 0.25, index=True)
    assert iv.windows(0.25, 8)[0] == 2
    assert (lo[0, 0], hi[0, 0], i[0, 0]) == (0.0, 2.0, 0)
    # all values equal: width 0 everywhere, i* = 0
    (lo, hi), i = iv.hdi(np.full((9, 1), 0.25), 0.5, index=True)
    assert (lo[0, 0], hi[0, 0], i[0, 0]) == (0.25, 0.25, 0)
    # a planted NaN: that column only
    x = np.random.default_rng(2).normal(size=(30, 3))
    clean = iv.hdi(x, 0.9, index=True)
    x[7, 1] = np.nan
    out, i = iv.hdi(x, 0.9, index=True)
    assert np.isnan(out[:, 0, 1]).all() and i[0, 1] == 0
    for q in (0, 2):
        assert (out[:, 0, q] == clean[0][:, 0, q]).all() and i[0, q] == clean[1][0, q]
    # -inf and +inf in one column: inf - -inf = inf, inf - inf = NaN read as +inf; finite windows win
    col = np.array([-np.inf, -np.inf, 1.0, 1.5, 3.0, np.inf, np.inf])
    (lo, hi), i = iv.hdi(col[:, None], 0.15, index=True)           # K = 1: widths NaN->inf, inf, 0.5, 1.5, inf, NaN->inf
    assert iv.windows(0.15, 7)[0] == 1 and (lo[0, 0], hi[0, 0], i[0, 0]) == (1.0, 1.5, 2)
    (lo, hi), i = iv.hdi(col[:, None], 0.3, index=True)            # K = 2: widths inf, inf, 2, inf, inf
    assert iv.windows(0.3, 7)[0] == 2 and (lo[0, 0], hi[0, 0], i[0, 0]) == (1.0, 3.0, 2)
    (lo, hi), i = iv.hdi(col[:, None], 0.9, index=True)            # K = 6: the only window is inf wide
    assert (lo[0, 0], hi[0, 0], i[0, 0]) == (-np.inf, np.inf, 0)
    (lo, hi), i = iv.hdi(np.array([np.inf, np.inf, np.inf])[:, None], 0.5, index=True)     # every width NaN: i* = 0
    assert (lo[0, 0], hi[0, 0], i[0, 0]) == (np.inf, np.inf, 0)
    # K = 1: the closest pair; K = N - 1: the whole column
    col = np.array([0.0, 10.0, 3.0, 3.5, 7.0])
    (lo, hi), i = iv.hdi(col[:, None], 0.2, index=True)
    assert iv.windows(0.2, 5)[0] == 1 and (lo[0, 0], hi[0, 0], i[0, 0]) == (3.0, 3.5, 1)
    (lo, hi), i = iv.hdi(col[:, None], 0.8, index=True)
    assert iv.windows(0.8, 5)[0] == 4 and (lo[0, 0], hi[0, 0], i[0, 0]) == (0.0, 10.0, 0)


def test_windows_and_value_errors():
    np.testing.assert_array_equal(iv.windows((0.5, 0.9, 0.95), 128000), [64000, 115200, 121600])
    assert iv.windows(0.95, 2).tolist() == [1] and iv.windows(0.5, 3).tolist() == [1]
    assert iv.windows(0.95, 100).dtype == np.int64
    for mass in (0.0, -0.1, 1.0, 1.5, np.nan, (0.5, 1.0)):
        with pytest.raises(ValueError, match='strictly between'):
            iv.windows(mass, 100)
    with pytest.raises(ValueError, match='leaves no interval'):
        iv.windows(0.2, 4)                                   # floor(0.8) = 0
    with pytest.raises(ValueError, match='2 values'):
        iv.windows(0.5, 1)
    with pytest.raises(ValueError, match='2 values'):
        iv.hdi(np.zeros((1, 1, 2)), 0.5)
    with pytest.raises(ValueError, match='divide'):
        iv.hdi(np.zeros((4, 5, 2)), 0.5, n_ensembles=2)
    with pytest.raises(ValueError, match='one ensemble'):
        iv.hdi(np.zeros((10, 2)), 0.5, n_ensembles=2)


# -- plumbing -------------------------------------------------------------------------------------------------------
def test_entry_points_exist(hip_lib):
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in ('bisip_chain_hdi_dev', 'bisip_chain_hdi_workspace'):
        assert hasattr(hip_lib, name)
        assert re.search(r'\b%s\(' % name, header)
        assert callable(getattr(_hip, name[len('bisip_'):]))
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    assert 'bisip_*' in exports                                # every bisip_ symbol leaves the library
    assert hip_lib.bisip_abi_version() == 6                    # symbols were only added


def a256(x):
    return (x + 255) // 256 * 256


def scratch(items, segments):
    return a256(a256(8 * items) + 16 * segments + 65536)


def formula(path, n, E, Wp, ndim, K):
    """The workspace include/bisip_hip.h states."""
    N, columns, m_max = n * Wp, E * ndim, max(n * Wp - k for k in K)
    if path == 'full':
        return 2 * a256(8 * N * columns) + scratch(N * columns, columns)
    return (a256(8 * N * columns) + a256(16 * len(K) * columns) + a256(8 * columns) + a256(4 * columns) +
            2 * a256(16 * columns * m_max) + scratch(2 * columns * m_max, 2 * columns))


def test_plan_and_workspace(monkeypatch):
    from bisip_amd import _hip
    monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    survey = (500, 512, 256, 7)
    K = iv.windows((0.5, 0.9, 0.95), 128000)
    assert iv.plan(*survey, K[2:]) == 'tails' and iv.plan(*survey, K) == 'full'      # mass 0.5 keeps half of the column
    assert iv.plan(5000, 1, 32, 7, iv.windows(0.95, 160000)) == 'tails'
    # the switch: N = 4096 at least, and 8 * M <= N for every window
    assert iv.plan(4096, 1, 1, 2, [3584]) == 'tails' and iv.plan(4096, 1, 1, 2, [3583]) == 'full'
    assert iv.plan(4095, 1, 1, 2, [4000]) == 'full' and iv.plan(4096, 1, 1, 2, [4000, 3583]) == 'full'
    cases = [(survey, K[2:]), (survey, K), ((5, 3, 2, 2), [9]), ((1, 1, 2, 1), [1]), ((4096, 1, 1, 2), [3584]),
             ((4096, 1, 1, 2), [3583]), ((600, 64, 64, 7), [36480, 19200])]
    for shape, k in cases:
        assert _hip.chain_hdi_workspace(*shape, k) == formula(iv.plan(*shape, k), *shape, k), (shape, k)
    for path in ('full', 'tails'):                                                    # forced: plan and workspace follow
        monkeypatch.setenv('BISIP_HDI_PATH', path)
        for shape, k in cases:
            assert iv.plan(*shape, k) == path
            assert _hip.chain_hdi_workspace(*shape, k) == formula(path, *shape, k), (path, shape, k)
    monkeypatch.setenv('BISIP_HDI_PATH', 'neither')                                   # anything else: the rule
    assert iv.plan(*survey, K[2:]) == 'tails'
    assert _hip.chain_hdi_workspace(*survey, K[2:]) == formula('tails', *survey, K[2:])
    monkeypatch.delenv('BISIP_HDI_PATH')
    for bad in ((0, 1, 8, 3), (4, 0, 8, 3), (4, 1, 0, 3), (4, 1, 8, 17), (4, 1, 8, 0), (1 << 31, 1, 8, 3), (4, 1, 1 << 29, 3),
                (1 << 16, 1 << 11, 1, 16)):
        assert _hip.chain_hdi_workspace(*bad, [1]) < 0, bad
    assert _hip.chain_hdi_workspace(1, 1, 1, 3, [1]) < 0                 # N = 1: no window
    assert _hip.chain_hdi_workspace(4, 1, 8, 3, [0]) < 0 and _hip.chain_hdi_workspace(4, 1, 8, 3, [32]) < 0
    assert _hip.chain_hdi_workspace(4, 1, 8, 3, [31]) > 0 and _hip.chain_hdi_workspace(4, 1, 8, 3, [1]) > 0
    assert _hip.chain_hdi_workspace(4, 1, 8, 3, []) < 0 and _hip.chain_hdi_workspace(4, 1, 8, 3, [5] * 9) < 0
    assert _hip.chain_hdi_workspace(4, 1, 8, 3, [5] * 8) > 0


def test_entry_point_checks_its_arguments(monkeypatch):
    from bisip_amd import _hip
    monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    # the pointers are never dereferenced: every call below is refused on the host
    ok = dict(chain=4096, n=8, stride=8 * 3, E=1, Wp=8, ndim=3, K=[60], out=4096, index=4096, work=4096, nbytes=1 << 20)

    def run(**kw):
        a = dict(ok, **kw)
        _hip.chain_hdi_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['K'], a['out'], a['index'],
                           a['work'], a['nbytes'], 0)

    for name in ('chain', 'out', 'work'):
        with pytest.raises(ValueError, match='null'):
            run(**{name: 0})
    with pytest.raises(ValueError, match='ndim'):
        run(ndim=0)
    with pytest.raises(ValueError, match='ndim'):
        run(ndim=17, stride=8 * 17)
    with pytest.raises(ValueError, match='sample_stride'):
        run(stride=23)
    with pytest.raises(ValueError, match='bad chain shape'):
        run(E=0)
    with pytest.raises(ValueError, match='n_windows'):
        run(K=[])
    with pytest.raises(ValueError, match='n_windows'):
        run(K=[5] * 9)
    with pytest.raises(ValueError, match='window'):
        run(K=[0])
    with pytest.raises(ValueError, match='window'):
        run(K=[60, 64])                                      # N = 64
    with pytest.raises(ValueError, match='workspace'):
        run(nbytes=_hip.chain_hdi_workspace(8, 1, 8, 3, [60]) - 1)
    for path in ('full', 'tails'):
        monkeypatch.setenv('BISIP_HDI_PATH', path)
        with pytest.raises(ValueError, match='workspace'):
            run(nbytes=_hip.chain_hdi_workspace(8, 1, 8, 3, [60]) - 1)


# -- the methods ------------------------------------------------------------------------------------------------------
def test_model_method_with_the_host_sampler():
    m = fitted_on_host()
    kw = dict(discard=5, thin=3)
    flat = m.get_chain(flat=True, **kw)
    lo, hi = m.get_param_hdi(**kw)                           # unpacks
    assert lo.shape == hi.shape == (4,)
    want = iv.hdi(flat, 0.95)
    np.testing.assert_array_equal(lo, want[0, 0])
    np.testing.assert_array_equal(hi, want[1, 0])
    assert (lo <= hi).all()
    np.testing.assert_array_equal(m.get_param_hdi(0.9, chain=flat), iv.hdi(flat, 0.9)[:, 0])
    both = m.get_param_hdi((0.5, 0.9), **kw)
    assert both.shape == (2, 2, 4)
    np.testing.assert_array_equal(both, iv.hdi(flat, (0.5, 0.9))[:, :, 0])
    with pytest.warns(UserWarning, match='No samples were discarded'):
        m.get_param_hdi()
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_param_hdi(chain=flat, discard=5)
    with pytest.raises(ValueError, match='Flatten'):
        m.get_param_hdi(chain=m.get_chain())
    with pytest.raises(ValueError, match='strictly between'):
        m.get_param_hdi(1.0, **kw)


class _HostChainSampler:
    """What SpectraBatch asks of its sampler, answered from a host chain (n, E, Wp, ndim) by the definition."""

    def __init__(self, chain):
        self.chain = chain

    def param_hdi(self, mass=0.95, discard=0, thin=1):
        a = self.chain[discard + thin - 1::thin]
        return iv.hdi(a.reshape(a.shape[0], -1, a.shape[3]), mass, self.chain.shape[1])


def test_spectra_batch_method_on_a_host_chain():
    from bisip_amd.batch import SpectraBatch
    chain = np.random.default_rng(8).normal(size=(30, 3, 6, 4))
    b = SpectraBatch.__new__(SpectraBatch)
    b._fitted = lambda: _HostChainSampler(chain)
    out = b.get_param_hdi(0.9, discard=4, thin=2)
    assert out.shape == (2, 3, 4)
    used = chain[5::2]
    for e in range(3):
        np.testing.assert_array_equal(out[:, e], iv.hdi(used[:, e].reshape(-1, 4), 0.9)[:, 0])
    assert b.get_param_hdi((0.5, 0.9), discard=4, thin=2).shape == (2, 2, 3, 4)
