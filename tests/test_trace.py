"""Walker traces on the host: the NumPy definition of bisip_amd.trace, the x axis, the argument checks of the Inversion
methods with a host sampler, the entry points' own argument checks, and plot_traces."""
import math

import numpy as np
import pytest

from bisip_amd import trace as tr
from fitted import fitted_on_host

P_SETS = [[50], [0, 100], [2.5, 50, 97.5], [0, 2.5, 16, 33.3, 50, 84, 97.5, 100]]


@pytest.mark.parametrize('p', P_SETS)
@pytest.mark.parametrize('shape', [(5, 2, 1), (4, 1, 2), (3, 63, 7), (6, 8, 4)])
def test_host_trace_is_np_percentile_per_step(p, shape):
    rng = np.random.default_rng(sum(shape) + len(p))
    chain = rng.normal(size=shape) * 10.0 ** rng.integers(-8, 3, shape[2])
    chain[-1, :, 0] = 0.25                   # a constant column
    pct, mean = tr.host_trace(chain, p)
    n, W, ndim = shape
    assert pct.shape == (len(p), n, ndim) and mean.shape == (n, ndim)
    for s in range(n):
        for q in range(ndim):
            np.testing.assert_array_equal(pct[:, s, q], np.percentile(chain[s, :, q], p))
            # any summation order is within (W - 1) 2^-53 sum|x| / W of the exact mean, to first order
            exact = math.fsum(chain[s, :, q]) / W
            assert abs(mean[s, q] - exact) <= W * 2.0 ** -52 * np.mean(np.abs(chain[s, :, q]))
    np.testing.assert_array_equal(mean, np.mean(chain, axis=1))
    assert tr.host_trace(chain, 50)[0].shape == (1, n, ndim)
    assert tr.host_trace(chain, ())[0].shape == (0, n, ndim)


def test_host_trace_nan_and_shape():
    chain = np.random.default_rng(0).normal(size=(4, 6, 2))
    chain[1, 3, 0] = np.nan
    pct, mean = tr.host_trace(chain, [25, 75])
    assert np.isnan(pct[:, 1, 0]).all() and np.isnan(mean[1, 0])
    assert np.isfinite(np.delete(pct, 1, axis=1)).all() and np.isfinite(pct[:, 1, 1]).all()
    with pytest.raises(ValueError, match='unflattened'):
        tr.host_trace(chain.reshape(-1, 2), [50])
    with pytest.raises(ValueError, match='no samples'):
        tr.host_trace(np.empty((0, 6, 2)), [50])


@pytest.mark.parametrize('bad', [[-0.1], [50, 100.5], [np.nan], [[1, 2], [3, 4]]])
def test_percentiles_are_checked(bad):
    with pytest.raises(ValueError, match='percentiles'):
        tr.check_percentiles(bad)
    with pytest.raises(ValueError, match='percentiles'):
        tr.host_trace(np.zeros((2, 3, 1)), bad)


def test_check_percentiles_accepts():
    np.testing.assert_array_equal(tr.check_percentiles(50), [50.0])
    np.testing.assert_array_equal(tr.check_percentiles((0, 100)), [0.0, 100.0])
    assert tr.check_percentiles([]).shape == (0,)


@pytest.mark.parametrize('n_total', [1, 7, 40])
def test_used_steps(n_total):
    for discard in (0, 1, 5, 39):
        for thin in (1, 2, 3, 7):
            want = np.arange(n_total)[discard + thin - 1::thin]
            if want.size == 0:
                with pytest.raises(ValueError, match='no samples'):
                    tr.used_steps(n_total, discard, thin)
            else:
                np.testing.assert_array_equal(tr.used_steps(n_total, discard, thin), want)


# -- the Inversion methods on a model fitted with the host sampler ------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(discard=5, thin=3)])
def test_inversion_traces_with_the_host_sampler(kw):
    m = fitted_on_host()
    chain = m.get_chain(**kw)
    p = [2.5, 50, 97.5]
    pct = m.get_trace_percentile(p, **kw)
    assert pct.shape == (3, chain.shape[0], 4)
    np.testing.assert_array_equal(pct, np.percentile(chain, p, axis=1))
    np.testing.assert_array_equal(m.get_trace_percentile(**kw), pct)
    np.testing.assert_array_equal(m.get_trace_percentile(50, **kw), pct[1])
    np.testing.assert_array_equal(m.get_trace_mean(**kw), np.mean(chain, axis=1))
    np.testing.assert_array_equal(m.get_trace_percentile(p, chain=chain), pct)
    np.testing.assert_array_equal(m.get_trace_mean(chain=chain), np.mean(chain, axis=1))
    lp = m._sampler.get_log_prob(**kw)
    got = m.get_log_prob_trace(p, **kw)
    assert got.shape == (3, chain.shape[0])
    np.testing.assert_array_equal(got, np.percentile(lp, p, axis=1))
    np.testing.assert_array_equal(m.get_log_prob_trace(16, **kw), np.percentile(lp, 16, axis=1))


@pytest.mark.parametrize('method', ['get_trace_percentile', 'get_trace_mean', 'get_log_prob_trace'])
def test_inversion_trace_argument_checks(method):
    m = fitted_on_host()
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=20)
    with pytest.raises(TypeError, match='flat'):
        f(flat=True)
    with pytest.raises(TypeError, match='unexpected keyword'):
        f(bins=3)
    if method != 'get_trace_mean':
        with pytest.raises(ValueError, match='percentiles'):
            f([50, 101])
        with pytest.raises(ValueError, match='percentiles'):
            f(-1)
    if method != 'get_log_prob_trace':
        with pytest.raises(ValueError, match='unflattened'):        # a flat chain
            f(chain=m.get_chain(flat=True))
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=m.get_chain(), discard=5)
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=m.get_chain(), thin=2)


def test_unfitted_model_refuses():
    import bisip_amd
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=8)
    for f in (m.plot_traces, m.get_trace_percentile, m.get_trace_mean, m.get_log_prob_trace):
        with pytest.raises(AssertionError, match='not fitted'):
            f()
    with pytest.raises(NotImplementedError):      # the other plots of the reference are still refused
        m.plot_fit()


# -- the library ----------------------------------------------------------------------------------------------------
def test_entry_points_exist(hip_lib):
    from __graft_entry__ import header_abi_version
    for name in ('bisip_chain_trace_dev', 'bisip_chain_trace_workspace', 'bisip_chain_trace_lds_walkers'):
        assert hasattr(hip_lib, name)
    assert hip_lib.bisip_abi_version() == header_abi_version()


def test_lds_walkers_and_workspace():
    from bisip_amd import _hip
    for ndim in range(1, 17):
        w = _hip.chain_trace_lds_walkers(ndim)
        assert w >= 8 and w & (w - 1) == 0
        # the padded columns of one ensemble fit 64 KiB, those of the next power of two do not
        pitch = lambda n: (n + n // 32) | 1
        assert ndim * pitch(w) * 8 <= 65536 < ndim * pitch(2 * w) * 8
        assert _hip.chain_trace_workspace(10, 3, w, ndim, 3) == 0
        assert _hip.chain_trace_workspace(10, 3, w + 1, ndim, 3) == 10 * 3 * (w + 1) * ndim * 8
    assert _hip.chain_trace_lds_walkers(0) == 0 and _hip.chain_trace_lds_walkers(17) == 0
    assert _hip.chain_trace_lds_walkers(7) >= 256          # the survey's ensembles are sorted in LDS
    # bounded: slabs of samples, not the chain
    assert _hip.chain_trace_workspace(10 ** 6, 1, 32768, 7, 3) <= 256 << 20
    assert _hip.chain_trace_workspace(200, 1, 1 << 23, 7, 3) == (1 << 23) * 7 * 8       # one sample, if that is larger
    for bad in ((0, 1, 8, 3, 1), (4, 0, 8, 3, 1), (4, 1, 0, 3, 1), (4, 1, 8, 17, 1), (4, 1, 8, 3, 9), (4, 1, 8, 3, -1)):
        assert _hip.chain_trace_workspace(*bad) < 0


def test_entry_point_checks_its_arguments():
    from bisip_amd import _hip
    ok = dict(n=4, stride=8 * 3, E=1, Wp=8, ndim=3, p=[50.0], pct=4096, mean=4096, chain=4096)
    # the pointers are never dereferenced: every call below is refused on the host

    def trace(**kw):
        a = dict(ok, **kw)
        _hip.chain_trace_dev(a['chain'], a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], a['p'], a['pct'], a['mean'], 0, 0, 0)

    with pytest.raises(ValueError, match='ndim'):
        trace(ndim=17, stride=8 * 17)
    with pytest.raises(ValueError, match='ndim'):
        trace(ndim=0)
    with pytest.raises(ValueError, match='sample_stride'):
        trace(stride=23)
    with pytest.raises(ValueError, match='bad chain shape'):
        trace(n=0)
    with pytest.raises(ValueError, match='bad chain shape'):
        trace(Wp=0)
    with pytest.raises(ValueError, match='null'):
        trace(chain=0)
    with pytest.raises(ValueError, match='null'):
        trace(pct=0)
    with pytest.raises(ValueError, match='n_percentiles=9'):
        trace(p=np.linspace(0, 100, 9))
    with pytest.raises(ValueError, match='neither'):
        trace(p=None, mean=0)
    with pytest.raises(ValueError, match=r'\[0, 100\]'):
        trace(p=[101.0])
    with pytest.raises(ValueError, match='workspace'):        # beyond the LDS kernel, without its workspace
        trace(Wp=5000, stride=5000 * 3)


# -- the plot -------------------------------------------------------------------------------------------------------
@pytest.fixture
def agg():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    yield plt
    plt.close('all')


def check_frame(m, fig, xlim):
    assert len(fig.axes) == 4
    for i, ax in enumerate(fig.axes):
        assert ax.get_ylabel() == m.param_names[i]
        assert tuple(ax.get_ylim()) == tuple(m.param_bounds[:, i])
        assert tuple(ax.get_xlim()) == xlim
        assert ax.get_xlabel() == ('Steps' if i == 3 else '')
        assert ax.yaxis.label.get_position() == (-0.1, 0.5)
    assert fig.axes[0].get_shared_x_axes().joined(fig.axes[0], fig.axes[3])


@pytest.mark.parametrize('style', ['lines', 'auto'])
def test_plot_traces_lines(agg, style):
    m = fitted_on_host()
    chain = m.get_chain(discard=4)
    for fig in (m.plot_traces(style=style, discard=4), m.plot_traces(chain=chain, style=style)):
        check_frame(m, fig, (0, 16))
        for i, ax in enumerate(fig.axes):
            assert len(ax.lines) == 8 and not ax.collections
            for w, line in enumerate(ax.lines):
                np.testing.assert_array_equal(line.get_ydata(), chain[:, w, i])
                np.testing.assert_array_equal(line.get_xdata(), np.arange(16))
                assert line.get_alpha() == 0.3
    with pytest.raises(ValueError, match='Do not pass both'):
        m.plot_traces(chain=chain, style='lines', discard=2)
    with pytest.raises(ValueError, match='unflattened'):
        m.plot_traces(chain=m.get_chain(flat=True), style='lines')


def test_plot_traces_band(agg):
    from matplotlib.collections import PolyCollection
    m = fitted_on_host()
    kw = dict(discard=5, thin=3)
    fig = m.plot_traces(style='band', **kw)
    x = tr.used_steps(20, **kw)
    np.testing.assert_array_equal(x, [7, 10, 13, 16, 19])
    check_frame(m, fig, (7, 20))
    pct = m.get_trace_percentile([2.5, 50, 97.5], **kw)
    for i, ax in enumerate(fig.axes):
        fills = [c for c in ax.collections if isinstance(c, PolyCollection)]
        assert len(fills) == 1 and len(ax.collections) == 1
        assert len(ax.lines) == 1
        np.testing.assert_array_equal(ax.lines[0].get_ydata(), m.get_trace_percentile(50, **kw)[:, i])
        np.testing.assert_array_equal(ax.lines[0].get_xdata(), x)
        assert ax.lines[0].get_color() == 'C3'
        verts = fills[0].get_paths()[0].vertices
        assert verts[:, 1].min() == pct[0, :, i].min() and verts[:, 1].max() == pct[2, :, i].max()
    # five percentiles: a band and three lines; an explicit chain is drawn against its own steps
    fig = m.plot_traces(chain=m.get_chain(discard=10), p=[84, 16, 50, 2.5, 97.5], style='band')
    check_frame(m, fig, (0, 10))
    for ax in fig.axes:
        assert len(ax.lines) == 3 and len(ax.collections) == 1
        assert [ln.get_color() for ln in ax.lines] == ['k', 'C3', 'k']
    with pytest.raises(ValueError, match='style'):
        m.plot_traces(style='walkers')
    m.nwalkers = 129                                 # more walkers than lines are drawn for: auto -> the band
    assert len(m.plot_traces(discard=4).axes[0].collections) == 1
