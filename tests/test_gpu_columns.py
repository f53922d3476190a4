"""The column toolkit of the chain summaries (bisip_amd/csrc/chain_columns.hip) at its edges: the selection kernel at every
dispatch length and down every path of its narrowing loop, the sort path on the same columns, and the column / grouped
entry points with the tiled gather behind them.  Every expected value is np.percentile of the same doubles; which path a
column takes is shown without a GPU in tests/test_select_cases.py."""
import numpy as np
import pytest

import select_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0        # what the outputs hold before a call: no percentile of any column here


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _select(cols, p):
    """``(len(p), columns)``: bisip_columns_percentiles_dev (always the selection) of host columns ``(columns, n)``."""
    import torch
    from bisip_amd import _hip
    cols = np.atleast_2d(cols)
    d = torch.from_numpy(np.array(cols, dtype=np.float64, order='C')).cuda()       # a copy: the shared columns are read-only
    out = torch.full((len(p), cols.shape[0]), SENTINEL, dtype=torch.float64, device='cuda')
    _hip.columns_percentiles_dev(d.data_ptr(), cols.shape[0], cols.shape[1], p, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _grouped(rows, p, single=False):
    """``(len(p), n_groups, n_cols)``: bisip_grouped_percentiles_dev of host rows ``(n_groups, n_rows, n_cols)``, or
    bisip_column_percentiles_dev of the one group (``single``)."""
    import torch
    from bisip_amd import _hip
    G, n_rows, n_cols = rows.shape
    d = torch.from_numpy(np.array(rows, dtype=np.float64, order='C')).cuda()       # a copy: the shared columns are read-only
    out = torch.full((len(p), G, n_cols), SENTINEL, dtype=torch.float64, device='cuda')
    if single:
        assert G == 1
        nbytes = _hip.column_percentiles_workspace(n_rows, n_cols, len(p))
    else:
        nbytes = _hip.grouped_percentiles_workspace(G, n_rows, n_cols, len(p))
    assert nbytes > 0
    work = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    if single:
        _hip.column_percentiles_dev(d.data_ptr(), n_rows, n_cols, p, out.data_ptr(), work.data_ptr(), nbytes, _stream())
    else:
        _hip.grouped_percentiles_dev(d.data_ptr(), G, n_rows, n_cols, p, out.data_ptr(), work.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b, what=''):
    """Bit for bit, the sign of a zero included; NaN where the other has NaN, whatever its payload."""
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)), (what, 'NaN pattern')
    ia, ib = a.view(np.int64)[~nan], b.view(np.int64)[~nan]
    bad = np.flatnonzero(ia != ib)
    assert bad.size == 0, (what, 'first differences', [(a[~nan][i], b[~nan][i]) for i in bad[:5]], np.argwhere(~nan)[bad[:5]])


# ---------------------------------------------------------------------------------------------------------------------
# (a) the selection on prepared columns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sc.LENGTHS)
def test_selection_at_every_length_and_kind(n):
    """One column of every kind in one launch, at the lengths on either side of every change of path: NumPy's doubles."""
    cols = sc.columns(n)
    lists = [sc.P8] + ([sc.P13, sc.P17] if n in sc.DISPATCH_LENGTHS else [])
    for p in lists:
        sc.assert_matches_numpy(_select(cols, p), sc.reference(cols, p), (n, len(p), sc.KINDS))
    c = sc.clusters(n)
    if c is not None:
        p = sc.cluster_percentiles(c.size)
        sc.assert_matches_numpy(_select(c, p), sc.reference(c, p)[:, None], (c.size, 'clusters'))
        sc.assert_matches_numpy(_select(c, sc.P8), sc.reference(c, sc.P8)[:, None], (c.size, 'clusters', 'P8'))


@pytest.mark.parametrize('p', [[33.3], [0], [100]])
def test_selection_of_one_percentile(p):
    """Two ranks in all (R = 2); the minimum alone and the maximum alone, where both ranks are the same key."""
    for n in (193, 8193):
        cols = sc.columns(n)
        sc.assert_matches_numpy(_select(cols, p), sc.reference(cols, p), (n, p))


# ---------------------------------------------------------------------------------------------------------------------
# (b) selection, sort and NumPy agree
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sc.DISPATCH_LENGTHS)
def test_selection_and_sort_agree_on_every_kind(n, monkeypatch):
    """The same columns as rows ``(n, kinds)`` through bisip_grouped_percentiles_dev, by selection (few columns) and by the
    segmented sort with k_percentile_lerp (BISIP_PERCENTILE_SORT=1): the same bits, the sign of a zero included since both
    order the keys, and NumPy's doubles -- with infinities, subnormals and neighbours decades apart ('clusters': t = 0.5
    takes the ``y - d * (1 - t)`` branch).  'tiny' with the 40th percentile is the case that needs k_order_zeros: both
    neighbours are -0.0 by the keys and t >= 0.5, so the percentile is -0.0, while the library sort alone leaves the zeros of
    either sign in the order they came."""
    cols = sc.columns(n)
    c = sc.clusters(n)
    cases = [(cols, p) for p in (sc.P8, sc.P13, sc.P17)] + [(c[None, :], sc.cluster_percentiles(c.size)), (c[None, :], sc.P13)]
    for k, (x, p) in enumerate(cases):
        rows = np.ascontiguousarray(x.T)[None]              # (1, n, kinds)
        outs = {}
        for mode in ('select', 'sort'):
            if mode == 'sort':
                monkeypatch.setenv('BISIP_PERCENTILE_SORT', '1')
            else:
                monkeypatch.delenv('BISIP_PERCENTILE_SORT', raising=False)
            outs[mode] = _grouped(rows, p)[:, 0, :]
        monkeypatch.delenv('BISIP_PERCENTILE_SORT', raising=False)
        want = sc.reference(x, p)
        sc.assert_matches_numpy(outs['select'], want, (n, k, 'select'))
        sc.assert_matches_numpy(outs['sort'], want, (n, k, 'sort'))
        _same_bits(outs['select'], outs['sort'], (n, k))


def test_the_sort_path_orders_zeros_as_the_selection_does():
    """64 columns and 17 percentiles: sorted without being forced to.  Zeros of both signs in random order -- a column of
    nothing else, a run of zeros at the end of the sorted column, one at its start, one in the middle, two zeros the wrong
    way round -- give the bits of the selection, which orders -0.0 before 0.0 by its keys."""
    rng = np.random.RandomState(64)
    n_rows, n_cols = 301, 64
    zeros = np.where(rng.random_sample((n_rows, n_cols)) < 0.5, -0.0, 0.0)
    other = rng.standard_normal((n_rows, n_cols))
    keep = rng.random_sample((n_rows, n_cols)) < 0.7                          # 70 % zeros
    c = np.arange(n_cols) % 4
    rows = np.where(c == 0, zeros, np.where(keep, zeros, np.where(c == 1, -np.abs(other), np.where(c == 2, np.abs(other), other))))
    rows[:, 63] = np.arange(n_rows) - 150.0                                   # no zero run: one 0.0 ...
    rows[:, 62] = np.arange(n_rows) - 150.0
    rows[7, 62], rows[200, 62] = 0.0, -0.0                                    # ... and 0.0 before -0.0 among distinct values
    got = _grouped(rows[None], sc.P17)[:, 0, :]
    sel = _select(rows.T, sc.P17)
    sc.assert_matches_numpy(got, sc.reference(rows.T, sc.P17).reshape(got.shape), 'sort')
    _same_bits(sel, got, 'zeros')
    zero = got == 0
    assert np.signbit(got[zero]).any() and not np.signbit(got[zero]).all()


# ---------------------------------------------------------------------------------------------------------------------
# (c) the column and grouped entry points, and the tiled gather
# ---------------------------------------------------------------------------------------------------------------------
ROWS = (1, 63, 64, 65, 200)
PC = [0, 100, 50, 2.5, 97.5, 33.3, 16, 84, 99.99, 25, 75, 5, 95]      # 13: sorted from 64 columns on, selected as 8 + 5 below


def _distinct_rows(G, n_rows, n_cols, seed):
    """``(G, n_rows, n_cols)`` of distinct values: column (g, c) holds a permutation of n_rows consecutive integers, its
    own, times a scale that grows with c -- a value from another column lies outside this one's range, so a value gathered
    into the wrong column or left unwritten moves the 0th or the 100th percentile."""
    rng = np.random.RandomState(seed)
    first = (np.arange(G)[:, None] * n_cols + np.arange(n_cols)[None, :]) * n_rows + 1             # (G, n_cols)
    perm = np.stack([rng.permutation(n_rows) for _ in range(G * n_cols)]).reshape(G, n_cols, n_rows).transpose(0, 2, 1)
    rows = (first[:, None, :] + perm) * (1.0 + np.arange(n_cols) / 1024.0)
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize('n_groups', [1, 3])
@pytest.mark.parametrize('n_cols', [1, 15, 16, 17, 63, 64, 65, 130])
def test_column_and_grouped_percentiles(n_cols, n_groups):
    """np.percentile(rows, p, axis=-2) of (n_groups, n_rows, n_cols) rows, layout (n_p, n_groups, n_cols): the plain gather
    below 16 columns, the tiled one from 16 on with one, two and three tiles of columns, whole and ragged in both directions."""
    for n_rows in ROWS:
        rows = _distinct_rows(n_groups, n_rows, n_cols, n_cols * 7 + n_rows)
        for p in (PC, PC[:5]):
            want = np.percentile(rows, p, axis=-2)
            assert want.shape == (len(p), n_groups, n_cols)
            got = _grouped(rows, p)
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert bad.size == 0, (n_rows, len(p), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
            if n_groups == 1:
                assert np.array_equal(_grouped(rows, p, single=True), want), (n_rows, len(p), 'column_percentiles_dev')


def test_column_and_grouped_percentiles_refuse_what_they_cannot_do():
    import torch
    from bisip_amd import _hip
    n_rows, n_cols, G = 20, 5, 2
    d = torch.from_numpy(_distinct_rows(G, n_rows, n_cols, 1)).cuda()
    out = torch.empty((3, G, n_cols), dtype=torch.float64, device='cuda')
    p = [2.5, 50, 97.5]
    nb1 = _hip.column_percentiles_workspace(n_rows, n_cols, 3)
    nbg = _hip.grouped_percentiles_workspace(G, n_rows, n_cols, 3)
    assert nb1 > 0 and nbg >= nb1
    work = torch.empty(nbg, dtype=torch.uint8, device='cuda')
    a, o, w = d.data_ptr(), out.data_ptr(), work.data_ptr()
    for bad_cols in (0, 65537):
        with pytest.raises(ValueError, match=f'bisip_hip: n_cols={bad_cols} out of range'):
            _hip.column_percentiles_dev(a, n_rows, bad_cols, p, o, w, nb1)
        with pytest.raises(ValueError, match=f'bisip_hip: n_cols={bad_cols} out of range'):
            _hip.grouped_percentiles_dev(a, G, n_rows, bad_cols, p, o, w, nbg)
    with pytest.raises(ValueError, match='bisip_hip: n_groups=0'):
        _hip.grouped_percentiles_dev(a, 0, n_rows, n_cols, p, o, w, nbg)
    with pytest.raises(ValueError, match=r'bisip_hip: percentiles must be in \[0, 100\]'):
        _hip.column_percentiles_dev(a, n_rows, n_cols, [50, 101], o, w, nb1)
    with pytest.raises(ValueError, match=r'bisip_hip: percentiles must be in \[0, 100\]'):
        _hip.grouped_percentiles_dev(a, G, n_rows, n_cols, [101], o, w, nbg)
    with pytest.raises(ValueError, match=f'bisip_hip: workspace of {nb1 - 1} bytes, need {nb1}'):
        _hip.column_percentiles_dev(a, n_rows, n_cols, p, o, w, nb1 - 1)
    with pytest.raises(ValueError, match=f'bisip_hip: workspace of {nbg - 1} bytes, need {nbg}'):
        _hip.grouped_percentiles_dev(a, G, n_rows, n_cols, p, o, w, nbg - 1)
    with pytest.raises(ValueError, match='bisip_hip: '):
        _hip.column_percentiles_dev(a, n_rows, n_cols, [], o, w, nb1)
    with pytest.raises(ValueError, match='bisip_hip: '):
        _hip.grouped_percentiles_dev(a, G, n_rows, n_cols, [], o, w, nbg)
    # more than 2^31 values: no workspace, and the last shape below it has one
    assert _hip.column_percentiles_workspace(1 << 15, 1 << 16, 3) == 0
    assert _hip.grouped_percentiles_workspace(2, 1 << 14, 1 << 16, 3) == 0
    assert _hip.grouped_percentiles_workspace(1 << 16, 1 << 10, 1 << 6, 3) == 0
    assert _hip.column_percentiles_workspace((1 << 15) - 1, 1 << 16, 3) > 0
    _hip.grouped_percentiles_dev(a, G, n_rows, n_cols, p, o, w, nbg)          # the arguments above were good but for the one named
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.percentile(d.cpu().numpy(), p, axis=-2))


@pytest.mark.parametrize('Wp', [63, 65])
@pytest.mark.parametrize('ndim', [15, 16])
def test_chain_percentiles_skip_the_padding_between_samples(ndim, Wp):
    """bisip_chain_percentiles_dev with a sample_stride larger than one sample: what lies between the samples is NaN and
    must not be read, by the plain gather (ndim 15) or the tiled one (ndim 16), with ragged tiles of walkers."""
    import torch
    from bisip_amd import _hip
    n, E, pad = 5, 3, 7
    rng = np.random.RandomState(ndim * 100 + Wp)
    used = rng.standard_normal((n, E * Wp, ndim)) * rng.uniform(0.1, 50, ndim) + rng.uniform(-20, 20, ndim)
    row = E * Wp * ndim
    stored = np.full((n, row + pad), np.nan)
    stored[:, :row] = used.reshape(n, row)
    d = torch.from_numpy(stored).cuda()
    p = np.array(PC[:6], dtype=np.float64)
    nbytes = _hip.chain_percentiles_workspace(n, E, Wp, ndim, p.size)
    work = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    out = torch.full((p.size, E, ndim), SENTINEL, dtype=torch.float64, device='cuda')
    _hip.chain_percentiles_dev(d.data_ptr(), n, row + pad, E, Wp, ndim, p, out.data_ptr(), work.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    want = np.percentile(used.reshape(n, E, Wp, ndim).transpose(1, 0, 2, 3).reshape(E, n * Wp, ndim), p, axis=1)
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError, match='bisip_hip: sample_stride smaller than one sample'):
        _hip.chain_percentiles_dev(d.data_ptr(), n, row - 1, E, Wp, ndim, p, out.data_ptr(), work.data_ptr(), nbytes, 0)
