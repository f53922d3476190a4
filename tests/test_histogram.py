"""Posterior histograms on the host: the NumPy definition of bisip_amd.histogram is np.histogram's and
np.histogram2d's, integer for integer; argument checks; the Inversion methods with a host sampler; the plots."""
import numpy as np
import pytest

from bisip_amd import histogram as hg
from fitted import fitted_on_host

BINS = [1, 2, 20, 25, 64]
WIDTHS = [1e-8, 1e-5, 1e-2, 1.0, 1e2]


def planted_column(rng, lo, hi, bins, n=400):
    """Random values in [lo, hi] with every edge of the range planted, and their neighbours in floating point."""
    edges = np.linspace(lo, hi, bins + 1)
    x = rng.uniform(lo, hi, n)
    return np.concatenate([x, edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


@pytest.mark.parametrize('bins', BINS)
@pytest.mark.parametrize('width', WIDTHS)
def test_definition_is_np_histogram(bins, width):
    rng = np.random.default_rng(bins * 1000 + int(-np.log10(width)) + 20)
    for centre in (0.0, 1.0, -3.7, 123.456):
        lo, hi = centre - width / 2, centre + width / 2
        x = planted_column(rng, lo, hi, bins)
        edges = hg.edges_from_range([lo, hi], bins)
        want, want_edges = np.histogram(x, bins, (lo, hi))
        np.testing.assert_array_equal(edges, want_edges)
        got = hg.histogram_by_edges(x, edges)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want)
        # range=None: the edges come from the column's own min and max
        edges = hg.edges_from_range([x.min(), x.max()], bins)
        want, want_edges = np.histogram(x, bins)
        np.testing.assert_array_equal(edges, want_edges)
        np.testing.assert_array_equal(hg.histogram_by_edges(x, edges), want)


@pytest.mark.parametrize('bins', BINS)
def test_sub_range_with_values_outside(bins):
    rng = np.random.default_rng(bins)
    x = np.concatenate([rng.normal(0.0, 1.0, 2000), np.linspace(-0.5, 0.75, bins + 1)])
    edges = hg.edges_from_range([-0.5, 0.75], bins)
    want = np.histogram(x, bins, (-0.5, 0.75))[0]
    got = hg.histogram_by_edges(x, edges)
    np.testing.assert_array_equal(got, want)
    assert got.sum() < x.size


@pytest.mark.parametrize('bins', BINS)
def test_constant_column(bins):
    x = np.full(50, 0.3)
    want, want_edges = np.histogram(x, bins)
    edges = hg.edges_from_range([0.3, 0.3], bins)
    np.testing.assert_array_equal(edges, want_edges)
    assert edges[0] == 0.3 - 0.5 and edges[-1] == 0.3 + 0.5
    np.testing.assert_array_equal(hg.histogram_by_edges(x, edges), want)


@pytest.mark.parametrize('bins', BINS)
def test_nan_and_inf_with_an_explicit_range(bins):
    rng = np.random.default_rng(7 + bins)
    x = np.concatenate([rng.uniform(-1, 2, 500), [np.nan, np.inf, -np.inf, np.nan, 0.0, 1.0]])
    rng.shuffle(x)
    edges = hg.edges_from_range([0.0, 1.0], bins)
    with np.errstate(invalid='ignore'):
        want = np.histogram(x, bins, (0.0, 1.0))[0]
    np.testing.assert_array_equal(hg.histogram_by_edges(x, edges), want)
    y = rng.uniform(-1, 2, x.size)
    y[::17] = np.nan
    with np.errstate(invalid='ignore'):
        want2 = np.histogram2d(x, y, bins, [(0.0, 1.0), (0.0, 1.0)])[0]
    got2 = hg.pair_histograms_by_edges(np.stack([x, y], axis=1), np.stack([edges, edges]))
    np.testing.assert_array_equal(got2[0], want2.astype(np.int64))


@pytest.mark.parametrize('bins', BINS)
def test_pairs_are_np_histogram2d(bins):
    rng = np.random.default_rng(100 + bins)
    ndim = 4
    ranges = np.array([[0.9, 1.1], [-1e-8, 1e-8], [-50.0, 50.0], [0.25, 0.25 + 1e-5]])
    cols = [planted_column(rng, lo, hi, bins, n=300) for lo, hi in ranges]
    x = np.stack([rng.permutation(c) for c in cols], axis=1)
    x[::11, 2] = 77.0                        # outside in one coordinate: dropped from the pairs with it only
    edges = hg.edges_from_range(ranges, bins)
    for q in range(ndim):
        np.testing.assert_array_equal(edges[q], np.linspace(ranges[q, 0], ranges[q, 1], bins + 1))
    got = hg.pair_histograms_by_edges(x, edges)
    jj, kk = hg.pair_index(ndim)
    assert got.shape == (6, bins, bins) and got.dtype == np.int64
    for q, (j, k) in enumerate(zip(jj, kk)):
        want, ex, ey = np.histogram2d(x[:, j], x[:, k], bins, [tuple(ranges[j]), tuple(ranges[k])])
        np.testing.assert_array_equal(ex, edges[j])
        np.testing.assert_array_equal(ey, edges[k])
        np.testing.assert_array_equal(got[q], want.astype(np.int64))
    inside = (x >= ranges[:, 0]) & (x <= ranges[:, 1])
    assert not inside[::11, 2].any()
    for q, (j, k) in enumerate(zip(jj, kk)):
        assert got[q].sum() == np.sum(inside[:, j] & inside[:, k])
    np.testing.assert_array_equal(hg.histogram_by_edges(x, edges),
                                  np.stack([np.histogram(x[:, q], bins, tuple(ranges[q]))[0] for q in range(ndim)]))


def test_range_none_with_a_nan_raises():
    flat = np.random.default_rng(0).normal(size=(50, 3))
    flat[7, 1] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        hg.host_histograms(flat, 10)
    with pytest.raises(ValueError, match='not finite'):
        hg.host_pair_histograms(flat, 10)
    with pytest.raises(ValueError):           # NumPy's own refusal
        np.histogram(flat[:, 1], 10)
    flat[7, 1] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        hg.host_histograms(flat, 10)
    counts, _ = hg.host_histograms(flat, 10, [[-1, 1]] * 3)      # an explicit range counts the rest
    assert counts[1].sum() == np.sum(np.abs(flat[:, 1]) <= 1)


def test_pair_index_order():
    jj, kk = hg.pair_index(4)
    assert list(zip(jj.tolist(), kk.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for ndim in (2, 7, 12, 16):
        a, b = hg.pair_index(ndim)
        ta, tb = np.triu_indices(ndim, 1)
        np.testing.assert_array_equal(a, ta)
        np.testing.assert_array_equal(b, tb)
        assert a.size == ndim * (ndim - 1) // 2
    assert hg.pair_index(1)[0].size == 0


@pytest.mark.parametrize('bins', [0, -3, 2.5, '7', None, True, 20.0])
def test_bins_must_be_a_positive_integer(bins):
    with pytest.raises((TypeError, ValueError), match='bins'):
        hg.check_bins(bins)
    with pytest.raises((TypeError, ValueError), match='bins'):
        hg.edges_from_range([0.0, 1.0], bins)
    with pytest.raises((TypeError, ValueError), match='bins'):
        hg.host_histograms(np.zeros((4, 2)), bins)


def test_bins_accepts_numpy_integers():
    assert hg.check_bins(np.int64(25)) == 25 and isinstance(hg.check_bins(np.int32(3)), int)


def test_range_checks():
    bounds = np.array([[0.0, -1.0, 2.0], [1.0, 1.0, 3.0]])
    for bad in ([[0, 1], [np.nan, 1], [0, 1]], [[0, 1], [0, np.inf], [0, 1]], [[0, 1], [-np.inf, 0], [0, 1]]):
        with pytest.raises(ValueError, match='finite'):
            hg.resolve_range(bad, 2, 3)
    with pytest.raises(ValueError, match='lo must be <= hi'):
        hg.resolve_range([[0, 1], [1, 0], [0, 1]], 2, 3)
    for shape in ((2,), (3,), (2, 2), (3, 3), (4, 3, 2), (2, 3, 3), (1, 2, 3, 2)):
        with pytest.raises(ValueError, match='range must|a range must'):
            hg.resolve_range(np.zeros(shape), 2, 3)
    with pytest.raises(ValueError, match="None, 'bounds' or an array"):
        hg.resolve_range('prior', 2, 3, bounds)
    with pytest.raises(ValueError, match='needs parameter bounds'):
        hg.resolve_range('bounds', 2, 3)
    with pytest.raises(ValueError, match='bounds must have shape'):
        hg.resolve_range('bounds', 2, 2, bounds)
    r = hg.resolve_range('bounds', 2, 3, bounds)
    assert r.shape == (2, 3, 2)
    np.testing.assert_array_equal(r[1], bounds.T)
    r = hg.resolve_range([[0, 1], [0, 0], [-1, 1]], 2, 3)
    np.testing.assert_array_equal(r[0], r[1])
    per = np.arange(12.0).reshape(2, 3, 2)
    np.testing.assert_array_equal(hg.resolve_range(per, 2, 3), per)
    # range=None goes to the data
    r = hg.resolve_range(None, 1, 2, data_range=lambda: (np.array([[[0.0, 1.0], [2.0, 2.0]]]), np.zeros((1, 2), int)))
    np.testing.assert_array_equal(r, [[[0.0, 1.0], [2.0, 2.0]]])
    np.testing.assert_array_equal(hg.edges_from_range(r, 2)[0, 1], [1.5, 2.0, 2.5])


def test_edges_of_many_ranges_are_the_scalar_linspace():
    rng = np.random.default_rng(3)
    lo = rng.normal(size=(5, 7)) * 10.0 ** rng.integers(-8, 3, (5, 7))
    r = np.stack([lo, lo + 10.0 ** rng.integers(-8, 3, (5, 7))], axis=-1)
    r[0, 0] = [2.0, 2.0]
    r[1, 1] = [0.0, 5e-324]           # a step that underflows: np.linspace's other route
    for bins in BINS:
        edges = hg.edges_from_range(r, bins)
        assert edges.shape == (5, 7, bins + 1)
        for e in range(5):
            for q in range(7):
                a, b = r[e, q]
                if a == b:
                    a, b = a - 0.5, b + 0.5
                np.testing.assert_array_equal(edges[e, q], np.linspace(a, b, bins + 1))


def test_sample_and_edge_shapes_are_checked():
    with pytest.raises(ValueError, match='expected samples'):
        hg.histogram_by_edges(np.zeros((5, 3)), np.zeros((2, 4)))
    with pytest.raises(ValueError, match='expected samples'):
        hg.pair_histograms_by_edges(np.zeros((5, 3)), np.zeros((3, 1)))
    with pytest.raises(ValueError, match='Flatten'):
        hg.host_histograms(np.zeros((5, 3, 2)), 4)


# -- the Inversion methods on a model fitted with the host sampler ------------------------------------------------
def range_kinds(m, flat):
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    explicit = np.stack([lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo)], axis=1)     # cuts samples off on either side
    return {None: np.stack([lo, hi], axis=1), 'bounds': m.param_bounds.T, 'explicit': explicit}


@pytest.mark.parametrize('kind', [None, 'bounds', 'explicit'])
@pytest.mark.parametrize('kw', [dict(discard=0, thin=1), dict(discard=5, thin=3)])
def test_inversion_histograms_with_the_host_sampler(kind, kw):
    m = fitted_on_host()
    flat = m.get_chain(flat=True, **kw)
    r = range_kinds(m, flat)[kind]
    arg = r if kind == 'explicit' else kind
    counts, edges = m.get_param_histogram(range=arg, **kw)
    assert counts.shape == (4, 25) and edges.shape == (4, 26) and counts.dtype == np.int64
    for q in range(4):
        want, want_edges = np.histogram(flat[:, q], 25, tuple(r[q]))
        np.testing.assert_array_equal(counts[q], want)
        np.testing.assert_array_equal(edges[q], want_edges)
    if kind is None:
        assert (counts.sum(axis=1) == flat.shape[0]).all()
    pc, pe, (jj, kk) = m.get_corner_histograms(bins=7, range=arg, **kw)
    assert pc.shape == (6, 7, 7) and pe.shape == (4, 8)
    for q, (j, k) in enumerate(zip(jj, kk)):
        want, ex, ey = np.histogram2d(flat[:, j], flat[:, k], 7, [tuple(r[j]), tuple(r[k])])
        np.testing.assert_array_equal(pc[q], want.astype(np.int64))
        np.testing.assert_array_equal(pe[j], ex)
        np.testing.assert_array_equal(pe[k], ey)
    # an explicit chain counts the same
    c2, e2 = m.get_param_histogram(range=arg, chain=flat)
    np.testing.assert_array_equal(c2, counts)
    np.testing.assert_array_equal(e2, edges)


@pytest.mark.parametrize('method', ['get_param_histogram', 'get_corner_histograms'])
def test_inversion_histogram_argument_checks(method):
    m = fitted_on_host()
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=20)
    with pytest.raises(ValueError, match='Do not pass both'):
        f(chain=m.get_chain(flat=True), discard=5)
    with pytest.raises(ValueError, match='Flatten'):
        f(chain=m.get_chain())
    with pytest.raises((TypeError, ValueError), match='bins'):
        f(bins=0, discard=1)
    with pytest.raises((TypeError, ValueError), match='bins'):
        f(bins=2.5, discard=1)
    with pytest.raises(ValueError, match='range must'):
        f(range=np.zeros((3, 2)), discard=1)
    with pytest.raises(ValueError, match='range must'):
        f(range=np.zeros((2, 4, 2)), discard=1)
    with pytest.raises(ValueError, match='lo must be <= hi'):
        f(range=[[1, 0]] * 4, discard=1)
    with pytest.raises(ValueError, match='finite'):
        f(range=[[0, np.nan]] * 4, discard=1)
    with pytest.raises(ValueError, match="None, 'bounds' or an array"):
        f(range='prior', discard=1)


def test_unfitted_model_refuses_to_plot():
    import bisip_amd
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=8)
    with pytest.raises(AssertionError, match='not fitted'):
        m.plot_histograms()
    with pytest.raises(AssertionError, match='not fitted'):
        m.plot_corner()


# -- the library ----------------------------------------------------------------------------------------------------
def test_entry_points_exist(hip_lib):
    from __graft_entry__ import header_abi_version
    for name in ('bisip_chain_range_dev', 'bisip_chain_histograms_dev', 'bisip_chain_pair_histograms_dev'):
        assert hasattr(hip_lib, name)
    assert hip_lib.bisip_abi_version() == header_abi_version()


def test_entry_points_check_their_arguments():
    from bisip_amd import _hip
    ok = dict(n=4, stride=8 * 3, E=1, Wp=8, ndim=3)
    ptr = 4096              # never dereferenced: every call below is refused on the host

    def hist(entry, bins=5, **kw):
        a = dict(ok, **kw)
        entry(ptr, a['n'], a['stride'], a['E'], a['Wp'], a['ndim'], ptr, bins, ptr, 0)

    for entry in (_hip.chain_histograms_dev, _hip.chain_pair_histograms_dev):
        with pytest.raises(ValueError, match='bins'):
            hist(entry, bins=0)
        with pytest.raises(ValueError, match='ndim'):
            hist(entry, ndim=17, stride=8 * 17)
        with pytest.raises(ValueError, match='sample_stride'):
            hist(entry, stride=23)
        with pytest.raises(ValueError, match='bad chain shape'):
            hist(entry, n=0)
        with pytest.raises(ValueError, match='null'):
            entry(0, 4, 24, 1, 8, 3, ptr, 5, ptr, 0)
        with pytest.raises(RuntimeError, match='LDS'):
            hist(entry, bins=100000)
    with pytest.raises(ValueError, match='no pairs'):
        hist(_hip.chain_pair_histograms_dev, ndim=1, stride=8)
    with pytest.raises(ValueError, match='sample_stride'):
        _hip.chain_range_dev(ptr, 4, 23, 1, 8, 3, ptr, ptr, 0)
    with pytest.raises(ValueError, match='null'):
        _hip.chain_range_dev(ptr, 4, 24, 1, 8, 3, 0, ptr, 0)


# -- the plots ------------------------------------------------------------------------------------------------------
@pytest.fixture
def agg():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    yield plt
    plt.close('all')


def stair_values(ax):
    from matplotlib.patches import StepPatch
    steps = [p for p in ax.patches if isinstance(p, StepPatch)]
    assert len(steps) == 1
    return steps[0].get_data()


def test_plot_histograms(agg):
    m = fitted_on_host()
    fig = m.plot_histograms(bins=11, discard=4)
    counts, edges = m.get_param_histogram(bins=11, discard=4)
    assert len(fig.axes) == 4
    for q, ax in enumerate(fig.axes):
        assert ax.get_xlabel() == m.param_names[q]
        values, drawn_edges, _ = stair_values(ax)
        np.testing.assert_array_equal(values, counts[q])
        np.testing.assert_array_equal(drawn_edges, edges[q])
        np.testing.assert_array_equal(values, np.histogram(m.get_chain(flat=True, discard=4)[:, q], 11)[0])
    fig = m.plot_histograms(chain=m.get_chain(flat=True, discard=10))
    assert stair_values(fig.axes[0])[0].size == 25


def test_plot_corner(agg):
    from matplotlib.collections import QuadMesh
    m = fitted_on_host()
    flat = m.get_chain(flat=True, discard=4)
    fig = m.plot_corner(discard=4)
    pc, edges, (jj, kk) = m.get_corner_histograms(discard=4)
    counts, _ = m.get_param_histogram(bins=20, discard=4)
    assert pc.shape == (6, 20, 20)
    assert len(fig.axes) == 16
    axes = np.array(fig.axes).reshape(4, 4)
    names = m.param_names
    for i in range(4):
        for j in range(4):
            ax = axes[i, j]
            if j > i:
                assert not ax.axison
                continue
            assert ax.axison
            assert ax.get_xlabel() == (names[j] if i == 3 else '')
            assert ax.get_ylabel() == (names[i] if (j == 0 and i > 0) else '')
            if j == i:
                values, drawn_edges, _ = stair_values(ax)
                np.testing.assert_array_equal(values, counts[i])
                np.testing.assert_array_equal(values, np.histogram(flat[:, i], 20)[0])
                np.testing.assert_array_equal(drawn_edges, edges[i])
            else:
                mesh = [c for c in ax.collections if isinstance(c, QuadMesh)]
                assert len(mesh) == 1
                q = int(np.flatnonzero((jj == j) & (kk == i))[0])
                want = np.histogram2d(flat[:, j], flat[:, i], 20)[0]
                np.testing.assert_array_equal(pc[q], want.astype(np.int64))
                # pcolormesh(x = parameter j, y = parameter i): rows of the drawn array run along y
                np.testing.assert_array_equal(np.asarray(mesh[0].get_array()).reshape(20, 20), pc[q].T)
    fig = m.plot_corner(chain=flat, bins=5)
    assert len(fig.axes) == 16
