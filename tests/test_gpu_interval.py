"""Highest-density intervals on the device (bisip_chain_hdi_dev), from the C entry point up to the model and SpectraBatch
methods.  The interval is an argmin over differences of two elements of a sorted column: intervals and indices are held to
equality with the NumPy definition (bisip_amd.interval.hdi), NaN where it gives NaN, under both paths of the kernel
(BISIP_HDI_PATH=full and =tails), which must also equal each other."""
import functools

import numpy as np
import pytest

import fitted
from chain_harness import SENTINEL, GuardedCall, shape_id, store
from convergence_bounds import hand_built_chain

pytestmark = pytest.mark.gpu

MASSES = (0.5, 0.9, 0.95)

# (n, E, Wp, ndim).  (1, 1, 2 | 3, 1): N = 2 and 3, M = 1.  (255 | 256 | 257, 1, 1, 2) and (1023 | 1024 | 1025, 1, 1, 1): on
# both sides of the window kernel's workgroup stride (256) and of the selection kernel's width (1024).  (7, 2, 63 | 64 | 65, 7):
# walkers around a wave.  (4, 1, 257, 16): the tiled gather.  (9, 256, 3, 2): many short columns.  (8200, 1, 1, 3) and
# (41000, 1, 1, 2): across the selection kernel's 8 x 1024 and 40 x 1024 template bounds (and two and eleven chunks of the
# compaction).  (4095 | 4096, 1, 1, 2): on both sides of the path switch for mass 0.95 (interval.plan).  (600, 64, 64, 7):
# the largest.
SHAPES = [(1, 1, 2, 1), (1, 1, 3, 1), (5, 3, 2, 2), (255, 1, 1, 2), (256, 1, 1, 2), (257, 1, 1, 2), (1023, 1, 1, 1),
          (1024, 1, 1, 1), (1025, 1, 1, 1), (7, 2, 63, 7), (7, 2, 64, 7), (7, 2, 65, 7), (4, 1, 257, 16), (9, 256, 3, 2),
          (8200, 1, 1, 3), (41000, 1, 1, 2), (4095, 1, 1, 2), (4096, 1, 1, 2), (600, 64, 64, 7)]


def on_device(x):
    """store() of x (n, E * Wp, ndim) with the samples on the device: what run_hdi takes as ``t``."""
    import torch
    stored, offset, stride = store(x)
    return torch.from_numpy(stored).cuda(), offset, stride


@functools.lru_cache(maxsize=3)
def case(n, E, Wp, ndim):
    """(stored samples on the device, the definition's (intervals, indices) for MASSES): computed once per shape."""
    from bisip_amd import interval as iv
    x, _, _ = hand_built_chain(n, E, Wp, ndim)
    want = iv.hdi(x, MASSES, E, index=True)
    return on_device(x), want


def run_hdi(t, n, E, Wp, ndim, K, path, monkeypatch, index=True):
    """One call under BISIP_HDI_PATH=path (None: the rule).  Outputs and workspace are followed by guard values."""
    import torch
    from bisip_amd import _hip
    if path is None:
        monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    else:
        monkeypatch.setenv('BISIP_HDI_PATH', path)
    K = [int(k) for k in K]
    samples, offset, stride = t
    call = GuardedCall()
    out = call.out('the intervals', (len(K), 2, E, ndim))
    idx = call.out('the indices', (len(K), E, ndim), torch.int64, asked=index)
    nbytes = _hip.chain_hdi_workspace(n, E, Wp, ndim, K)
    assert nbytes > 0
    _hip.chain_hdi_dev(samples.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, K, out, idx, call.work(nbytes), nbytes,
                       call.stream)
    return (*call.finish(), nbytes)


def assert_equal(got, want, what):
    """``==``, and NaN where the definition gives NaN (the sign of a zero is not pinned)."""
    (g, gi), (w, wi) = got, want
    assert not (g == SENTINEL).any(), what
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    assert (g[~nan] == w[~nan]).all(), (what, np.argwhere(~nan & (g != w))[:5])
    np.testing.assert_array_equal(gi, wi, err_msg=what)


@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_hdi_entry_point(shape, monkeypatch):
    from bisip_amd import interval as iv
    n, E, Wp, ndim = shape
    t, want = case(*shape)
    K = iv.windows(MASSES, n * Wp)
    got = {}
    for path in ('full', 'tails'):
        got[path] = run_hdi(t, n, E, Wp, ndim, K, path, monkeypatch)[:2]
        assert_equal(got[path], want, f'{shape} {path} {MASSES}')
        one = run_hdi(t, n, E, Wp, ndim, K[2:], path, monkeypatch)[:2]
        assert_equal(one, (want[0][2:], want[1][2:]), f'{shape} {path} 0.95')
    np.testing.assert_array_equal(np.isnan(got['full'][0]), np.isnan(got['tails'][0]))
    fin = ~np.isnan(got['full'][0])
    assert (got['full'][0][fin] == got['tails'][0][fin]).all()
    np.testing.assert_array_equal(got['full'][1], got['tails'][1])
    lo, hi = want[0][:, 0], want[0][:, 1]
    assert (lo[~np.isnan(lo)] <= hi[~np.isnan(lo)]).all()
    if ndim > 1 and E * Wp * ndim >= 24:
        assert np.isnan(lo).any() and not np.isnan(lo).all()          # hand_built_chain planted NaNs, in some columns only


@pytest.mark.parametrize('shape', [(4095, 1, 1, 2), (4096, 1, 1, 2), (600, 64, 64, 7)], ids=shape_id)
def test_path_switch(shape, monkeypatch):
    """Without BISIP_HDI_PATH the rule of interval.plan decides: the workspace is that path's, the results the same."""
    from bisip_amd import interval as iv
    n, E, Wp, ndim = shape
    N = n * Wp
    t, want = case(*shape)
    monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    K = iv.windows(MASSES, N)
    assert iv.plan(n, E, Wp, ndim, K) == 'full'                       # mass 0.5 keeps half of every column
    assert iv.plan(n, E, Wp, ndim, K[2:]) == ('tails' if N >= 4096 else 'full')
    sets = [K, K[2:]]
    if N == 4096:                                                     # 8 * M <= N: M = 512 | 513
        sets += [[3584], [3583]]
        assert iv.plan(n, E, Wp, ndim, [3584]) == 'tails' and iv.plan(n, E, Wp, ndim, [3583]) == 'full'
    for k in sets:
        monkeypatch.delenv('BISIP_HDI_PATH', raising=False)           # (run_hdi leaves the last forced path behind)
        ruled = iv.plan(n, E, Wp, ndim, k)
        g, gi, nbytes = run_hdi(t, n, E, Wp, ndim, k, None, monkeypatch)
        f, fi, forced_bytes = run_hdi(t, n, E, Wp, ndim, k, ruled, monkeypatch)
        assert nbytes == forced_bytes
        o, oi, other_bytes = run_hdi(t, n, E, Wp, ndim, k, 'tails' if ruled == 'full' else 'full', monkeypatch)
        assert other_bytes != nbytes
        for a, ai in ((f, fi), (o, oi)):
            np.testing.assert_array_equal(np.isnan(a), np.isnan(g))
            assert (a[~np.isnan(g)] == g[~np.isnan(g)]).all()
            np.testing.assert_array_equal(ai, gi)
        if len(k) == 1 and k[0] not in K:
            ref = iv.hdi(hand_built_chain(*shape)[0], (k[0] + 0.5) / N, E, index=True)
            assert_equal((g[0], gi[0]), ref, f'{shape} K = {k[0]}')
    assert_equal(run_hdi(t, n, E, Wp, ndim, K[2:], None, monkeypatch)[:2], (want[0][2:], want[1][2:]), f'{shape} rule')


@pytest.mark.parametrize('path', ['full', 'tails'])
def test_extreme_windows_and_null_index(path, monkeypatch):
    """K = N - 1 (M = 1: the whole column) and K = 1 (M = N - 1: the closest pair) on columns of 3000 values, in one call;
    an index that is not asked for is not written."""
    from bisip_amd import interval as iv
    n, E, Wp, ndim = 3000, 1, 1, 3
    N = n * Wp
    rng = np.random.default_rng(11)
    x = rng.normal(size=(n, E * Wp, ndim)) * np.array([1.0, 1e-6, 1e3])
    x[5, 0, 2] = x[900, 0, 2]                                        # a pair of width 0
    x[7, 0, 1] = -0.0
    x[8, 0, 1] = 0.0
    t = on_device(x)
    K = [N - 1, 1]
    g, gi, _ = run_hdi(t, n, E, Wp, ndim, K, path, monkeypatch)
    for k, kk in enumerate(K):
        assert iv.windows((kk + 0.5) / N, N)[0] == kk
        assert_equal((g[k], gi[k]), iv.hdi(x, (kk + 0.5) / N, E, index=True), f'K = {kk} {path}')
    assert (g[0, 0, 0] == x.min(axis=(0, 1))).all() and (g[0, 1, 0] == x.max(axis=(0, 1))).all() and (gi[0] == 0).all()
    assert g[1, 0, 0, 2] == g[1, 1, 0, 2] == x[5, 0, 2]
    g0, gi0, _ = run_hdi(t, n, E, Wp, ndim, K, path, monkeypatch, index=False)
    np.testing.assert_array_equal(g0, g)
    # +-inf in one column: NaN widths are read as +inf
    y = x.copy()
    y[:40, 0, 0] = -np.inf
    y[40:90, 0, 0] = np.inf
    t = on_device(y)
    for mass in (0.01, 0.5, 0.98):
        got = run_hdi(t, n, E, Wp, ndim, iv.windows(mass, N), path, monkeypatch)
        assert_equal((got[0][0], got[1][0]), iv.hdi(y, mass, E, index=True), f'inf {mass} {path}')


def test_hdi_of_a_device_tensor(monkeypatch):
    import torch
    from bisip_amd import interval as iv
    monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    x = np.random.default_rng(5).normal(size=(40, 6, 3))
    for E in (1, 2):
        for mass in (0.9, (0.5, 0.9)):
            for got, want in zip(iv.hdi(torch.from_numpy(x).cuda(), mass, E, index=True), iv.hdi(x, mass, E, index=True)):
                np.testing.assert_array_equal(got, want)
    flat = x.reshape(-1, 3)
    np.testing.assert_array_equal(iv.hdi(torch.from_numpy(flat).cuda(), 0.9), iv.hdi(flat, 0.9))
    masses = np.linspace(0.05, 0.95, 19)                               # more than 8 windows: several calls
    np.testing.assert_array_equal(iv.hdi(torch.from_numpy(x).cuda(), masses, 2), iv.hdi(x, masses, 2))


# -- through the layers ---------------------------------------------------------------------------------------------
KW = dict(discard=20, thin=2)


fitted_model = functools.lru_cache(maxsize=None)(fitted.fitted_model)         # (where='device': asserted there)


def test_model_methods(monkeypatch):
    from bisip_amd import interval as iv
    monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    m = fitted_model()
    flat = m.get_chain(flat=True, **KW)
    lo, hi = m.get_param_hdi(0.9, **KW)
    assert lo.shape == hi.shape == (m.ndim,) and (lo < hi).all()
    want = iv.hdi(flat, 0.9)
    np.testing.assert_array_equal(lo, want[0, 0])
    np.testing.assert_array_equal(hi, want[1, 0])
    np.testing.assert_array_equal(m.get_param_hdi(**KW), iv.hdi(flat, 0.95)[:, 0])
    np.testing.assert_array_equal(m.get_param_hdi(MASSES, **KW), iv.hdi(flat, MASSES)[:, :, 0])
    np.testing.assert_array_equal(m.get_param_hdi(0.9, chain=flat), want[:, 0])
    assert (((flat >= lo) & (flat <= hi)).mean(axis=0) >= 0.9).all()            # the interval holds the mass asked for
    with pytest.warns(UserWarning, match='No samples were discarded'):
        m.get_param_hdi()
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_param_hdi(chain=flat, discard=5)
    with pytest.raises(ValueError, match='no samples'):
        m.get_param_hdi(discard=120)
    # the integrating parameters (ndim = 3), in the order of get_integrating_percentile
    ichain = m.get_integrating_chain(flat=True, **KW)
    got = m.get_integrating_hdi(0.9, **KW)
    assert got.shape == (2, 3)
    np.testing.assert_array_equal(got, iv.hdi(ichain, 0.9)[:, 0])
    np.testing.assert_array_equal(m.get_integrating_hdi(MASSES, **KW), iv.hdi(ichain, MASSES)[:, :, 0])
    med = m.get_integrating_percentile(50, **KW)
    assert (got[0] <= med).all() and (med <= got[1]).all()
    for path in ('full', 'tails'):
        monkeypatch.setenv('BISIP_HDI_PATH', path)
        np.testing.assert_array_equal(m.get_param_hdi(0.9, **KW), want[:, 0])


@pytest.mark.parametrize('where', ['device', 'host'])
def test_spectra_batch_methods(where, monkeypatch):
    import bisip_amd
    from bisip_amd import interval as iv
    from bisip_amd.synthetic import synthetic_columns
    monkeypatch.delenv('BISIP_HDI_PATH', raising=False)
    spectra = [bisip_amd.DataFiles()['SIP-K389175']] + [synthetic_columns(20, i) for i in range(2)]
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=16, nsteps=60, poly_deg=2)
    np.random.seed(5)
    b.fit(seed=11, chain=where)
    flat = b.get_chain(flat=True, **KW)                               # (E, n * Wp, ndim)
    got = b.get_param_hdi(0.9, **KW)
    assert got.shape == (2, 3, b.ndim)
    for e in range(3):
        np.testing.assert_array_equal(got[:, e], iv.hdi(flat[e], 0.9)[:, 0])
    many = b.get_param_hdi(MASSES, **KW)
    assert many.shape == (3, 2, 3, b.ndim)
    np.testing.assert_array_equal(many[1], got)
    iflat = b.get_integrating_chain(flat=True, **KW)                  # (E, n * Wp, 3)
    igot = b.get_integrating_hdi(0.9, **KW)
    assert igot.shape == (2, 3, 3)
    for e in range(3):
        np.testing.assert_array_equal(igot[:, e], iv.hdi(iflat[e], 0.9)[:, 0])
    np.testing.assert_array_equal(b.gather(np.moveaxis(got, -2, 0)), np.moveaxis(got, -2, 0))      # a single process
    with pytest.raises(ValueError, match='no samples'):
        b.get_param_hdi(discard=60)
