"""The inputs of tests/test_gpu_columns.py reach the paths of the selection kernel they are meant for -- shown without a GPU
by ``select_cases.census``, which mirrors the narrowing loop of bisip_amd/csrc/chain_columns.hip and must follow its SEL_CAP.
Nothing here is compared with device output: the expected percentiles of the GPU tests are np.percentile's."""
import numpy as np
import pytest

import select_cases as sc

# a length in the smallest register form and the first length of the next one ('clusters': the multiple of 9 below)
CENSUS_LENGTHS = (1000, 8193)


def _census(kind, n):
    if kind == 'clusters':
        col = sc.clusters(n)
        return sc.census(col, sc.cluster_percentiles(col.size))
    return sc.census(sc.columns(n)[sc.KINDS.index(kind)], sc.P8)


@pytest.mark.parametrize('n', CENSUS_LENGTHS)
def test_every_kind_reaches_its_path(n):
    c = {kind: _census(kind, n) for kind in sc.KINDS + ('clusters',)}
    print(c)
    assert c['dup'].passes >= 6 and c['dup'].ends == 'exact'              # a rank inside more than SEL_CAP equal values
    assert c['nested'].s == 64 and c['nested'].passes >= 5 and c['nested'].ends == 'counting'
    assert c['lowbits'].s <= 8 and c['lowbits'].passes == 1 and c['lowbits'].ends == 'exact'     # shift == 0 at once
    assert c['clusters'].ranges == 16                                     # sixteen ranks, sixteen groups
    assert c['tiny'].ends == 'exact'
    assert c['constant'].s == 0 and c['constant'].passes == 0
    assert 2 <= c['normal'].passes <= 4
    assert c['nan_pos'].ends == 'nan' and c['nan_neg'].ends == 'nan'


@pytest.mark.parametrize('n', [n for n in sc.LENGTHS if n <= sc.SEL_CAP])
def test_short_columns_finish_at_once(n):
    for kind in sc.KINDS + ('clusters',):
        if kind == 'clusters' and n < 9:
            continue
        assert _census(kind, n).passes == 0, kind


def test_the_dispatch_lengths_take_more_than_one_pass():
    """At the first length of every other path the loop runs: 'dup' still ends exact from 8,193 values on, where the
    constant fills more than SEL_CAP places."""
    for n in sc.DISPATCH_LENGTHS:
        assert _census('normal', n).passes >= 1
        assert _census('nested', n).s == 64 and _census('nested', n).ends == 'counting'
        assert _census('lowbits', n).ends == 'exact' or n <= 200
    for n in sc.DISPATCH_LENGTHS[1:]:
        assert _census('dup', n).ends == 'exact'


def test_the_builders_hold_what_they_promise():
    n = 1000
    cols = sc.columns(n)
    k = {kind: cols[i] for i, kind in enumerate(sc.KINDS)}
    assert (k['dup'] == sc.DUP_VALUE).sum() > 3 * sc.SEL_CAP
    assert set(np.unique(k['tiny']).tolist()) <= set(sc.TINY_VALUES) and np.signbit(k['tiny'][k['tiny'] == 0]).any()
    assert not np.signbit(k['tiny'][k['tiny'] == 0]).all()
    assert np.unique(k['constant']).size == 1
    assert np.isnan(k['nan_pos']).sum() == 1 and not np.signbit(k['nan_pos'][np.isnan(k['nan_pos'])]).any()
    assert np.isnan(k['nan_neg']).sum() == 1 and np.signbit(k['nan_neg'][np.isnan(k['nan_neg'])]).all()
    for m in sc.LENGTHS:
        x = np.sort(sc.columns(m)[sc.KINDS.index('infs')])
        lo, hi = sc.ranks(m, [2.5, 99.99])
        assert x[lo[0]] == -np.inf                                          # a rank on an infinity ...
        if m > 2:
            assert np.isfinite(x[hi[0]]) and np.isfinite(x[lo[1]])          # ... and one next to it, at either end
            assert x[hi[1]] == np.inf
    c = sc.clusters(n)
    lo, hi = sc.ranks(c.size, sc.cluster_percentiles(c.size))
    srt = np.sort(c)
    assert c.size == 999 and (srt[hi] > 5 * srt[lo]).all()                  # the neighbours straddle a gap
    v = (c.size - 1) * (np.asarray(sc.cluster_percentiles(c.size)) / 100.0)
    assert ((v - lo >= 0.4) & (v - lo <= 0.6)).all()


def test_sort_then_lerp_is_numpys_percentile_on_the_columns():
    """The reference of the GPU tests and the kernels' formula agree on the host -- finite values bit for bit, NaN in the same
    places, the same infinities -- so a device difference is the device's."""
    for n in (2, 193, 1000):
        for p in (sc.P8, sc.P13, sc.P17):
            sc.assert_matches_numpy(sc.sort_then_lerp(sc.columns(n), p), sc.reference(sc.columns(n), p), (n, len(p)))
    c = sc.clusters(1000)
    p = sc.cluster_percentiles(c.size)
    sc.assert_matches_numpy(sc.sort_then_lerp(c, p), sc.reference(c, p), 'clusters')


@pytest.mark.parametrize('n,E,Wp,ndim', [(60, 9, 50, 9), (41, 8, 1000, 8)])
def test_the_signs_data_has_numpys_nan_pattern_under_the_kernels_formula(n, E, Wp, ndim):
    """The 'signs' cases of test_percentiles_by_selection_equal_the_sorted_ones (tests/test_gpu_batch.py), same generator and
    seed: sort, then NumPy's _lerp formula as the kernels evaluate it, gives NaN exactly where np.percentile does (inf - inf
    and inf * 0 next to the planted infinities) -- which is why that test asserts the pattern without an exception."""
    rng = np.random.RandomState(n + E + ndim)
    full = rng.standard_normal((n, E * Wp, ndim)) * rng.uniform(0.1, 50, ndim) + rng.uniform(-20, 20, ndim)
    sc.plant_signs(full)
    used = full.reshape(n, E, Wp, ndim).transpose(1, 0, 2, 3).reshape(E, n * Wp, ndim).transpose(0, 2, 1)    # (E, ndim, n * Wp)
    want = sc.reference(used, sc.P8)
    got = sc.sort_then_lerp(used, sc.P8)
    assert np.isnan(want).sum() in (27, 16) and np.isnan(want).sum() == (27 if n == 60 else 16)
    sc.assert_matches_numpy(got, want, 'signs')
