"""The summation order of bisip_chain_moments_dev as include/bisip_hip.h states it, in NumPy
(bisip_amd.chainview.moment_splits, exact_fma, ordered_moments), held on the CPU to the long-double reference and the
first-order bound of tests/moments_bounds.py.  tests/test_gpu_moments.py holds the kernel to the same bits and bound."""
import math

import numpy as np
import pytest

from bisip_amd.chainview import exact_fma, moment_splits, ordered_moments
from moments_bounds import (EXTREMES, BOTH_INFINITIES, MIRRORED, assert_agrees_with_numpy, assert_within_bounds, case,
                            has_extremes)

ids = dict(ids=lambda s: 'x'.join(map(str, s)))


def test_moment_splits_and_split_ranges():
    want = {1: [1] * 7 + [2, 2, 9, 4096], 5: [1] * 7 + [2, 2, 9, 820], 4095: [1] * 7 + [2, 2, 2, 2],
            4096: [1] * 11, 4097: [1] * 11}
    ns = list(range(1, 10)) + [37, 4096 * 4]
    for E, row in want.items():
        assert [moment_splits(n, E) for n in ns] == row, E
        for n in ns:
            splits = moment_splits(n, E)
            assert splits == max(1, min((4096 + E - 1) // E, n // 4))
            ranges = [(n * sp // splits, n * (sp + 1) // splits) for sp in range(splits)]
            assert ranges[0][0] == 0 and ranges[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            assert all(4 <= s1 - s0 for s0, s1 in ranges) or splits == 1
    assert [(9 * sp // 2, 9 * (sp + 1) // 2) for sp in range(2)] == [(0, 4), (4, 9)]
    lengths = [37 * (sp + 1) // 9 - 37 * sp // 9 for sp in range(9)]
    assert sorted(lengths) == [4] * 8 + [5]


def test_exact_fma():
    inf, nan = math.inf, math.nan
    # a * a = 1 + 2^-26 + 2^-54.  Rounded on its own it is 1 + 2^-26, and adding 2^-53 is then a tie that goes to the even
    # neighbour, down; the exact sum lies above the tie and goes up
    a, c = 1.0 + 2.0 ** -27, 2.0 ** -53
    assert a * a + c == 1.0 + 2.0 ** -26
    assert exact_fma(a, a, c) == 1.0 + 2.0 ** -26 + 2.0 ** -52
    # the product's low half survives a cancellation: (1 + 2^-30)^2 - (1 + 2^-29) = 2^-60
    a = 1.0 + 2.0 ** -30
    assert a * a - (1.0 + 2.0 ** -29) == 0.0 and exact_fma(a, a, -(1.0 + 2.0 ** -29)) == 2.0 ** -60
    assert exact_fma(3.0, 5.0, 7.0) == 22.0 and exact_fma(0.1, 10.0, -1.0) == 2.0 ** -54
    # overflow: only of the rounded result.  1e200^2 is far outside, and 2^1023 * 2 - 2^1023 is inside
    assert exact_fma(1e200, 1e200, 1.0) == inf and exact_fma(-1e200, 1e200, 1.0) == -inf
    assert exact_fma(2.0 ** 1023, 2.0, -2.0 ** 1023) == 2.0 ** 1023
    assert exact_fma(1e200, 1e200, -inf) == -inf and exact_fma(1e200, 1e200, inf) == inf
    # underflow: 1e-300^2 rounds to 0, a subnormal result is rounded once
    assert exact_fma(1e-300, 1e-300, 0.0) == 0.0 and not math.copysign(1.0, exact_fma(1e-300, 1e-300, 0.0)) < 0
    assert exact_fma(2.0 ** -537, 2.0 ** -537, 0.0) == 2.0 ** -1074 and exact_fma(2.0 ** -538, 2.0 ** -538, 0.0) == 0.0
    assert exact_fma(1.5 * 2.0 ** -537, 2.0 ** -537, 2.0 ** -1074) == 2.0 ** -1073          # 2.5 ulp: tie to even
    # not finite
    for args in ((nan, 1.0, 1.0), (1.0, nan, 1.0), (1.0, 1.0, nan), (inf, 0.0, 1.0), (inf, 1.0, -inf), (-inf, -inf, -inf)):
        assert math.isnan(exact_fma(*args)), args
    assert exact_fma(inf, 2.0, 1.0) == inf and exact_fma(-inf, -inf, 5.0) == inf and exact_fma(-inf, 2.0, 1e308) == -inf
    # signed zeros
    assert math.copysign(1.0, exact_fma(-0.0, 1.0, -0.0)) == -1.0 and math.copysign(1.0, exact_fma(-0.0, 1.0, 0.0)) == 1.0
    assert math.copysign(1.0, exact_fma(2.0, 3.0, -6.0)) == 1.0


@pytest.mark.parametrize('shape', MIRRORED, **ids)
def test_ordered_moments_within_the_bound_and_as_numpy(shape):
    n, E, Wp, ndim = shape
    c = case(*shape)
    mean, std = c['ordered']
    assert mean.shape == std.shape == (E, ndim) and mean.dtype == std.dtype == np.float64
    ref = c['ref']
    worst = assert_within_bounds(mean, std, ref, label=str(shape))
    assert_agrees_with_numpy(mean, std, ref, c['ref_numpy'], c['np_mean'], c['np_std'], label=str(shape))
    # parameter 0 is centred at 0 and finite: it is checked, and there the bound itself is small, else the inputs are wrong
    assert ref['checked'][:, 0].all()
    with np.errstate(all='ignore'):
        pos = ref['var'][:, 0] > 0
        rel = (ref['dvar'][:, 0] / ref['var'][:, 0])[pos]
    assert rel.size == 0 or rel.max() < 1e-9
    print(f'shape {shape}: error at most {worst:.3f} of its bound; {int(ref["checked"].sum())} of {E * ndim} checked')
    if ndim > 1:
        assert mean[E - 1, ndim - 1] == 0.25 and std[E - 1, ndim - 1] == 0.0
    if has_extremes(E, ndim):
        e, q, _ = EXTREMES['tiny']
        assert ref['checked'][e, q] and 1e-141 < std[e, q] < 1e-139
        e, q, _ = EXTREMES['huge']
        assert not ref['checked'][e, q] and std[e, q] == np.inf and np.isfinite(mean[e, q])
        e, q, _ = EXTREMES['vanishing']
        assert not ref['checked'][e, q] and std[e, q] == 0.0 and mean[e, q] > 1e-300
        assert np.isnan(mean[BOTH_INFINITIES]) and np.isnan(std[BOTH_INFINITIES])


def test_the_data_leave_three_quarters_to_the_bound_and_hold_every_kind_of_value():
    checked = sum(int(case(*s)['ref']['checked'].sum()) for s in MIRRORED)
    total = sum(s[1] * s[3] for s in MIRRORED)
    assert 4 * checked >= 3 * total, (checked, total)
    means = np.concatenate([case(*s)['np_mean'].ravel() for s in MIRRORED])
    assert np.isnan(means).sum() >= 4 and (means == np.inf).sum() >= 2 and (means == -np.inf).sum() >= 2
    # narrow posteriors around large centres: what tells a two-pass variance from a one-pass one
    narrow = 0
    for s in MIRRORED:
        c = case(*s)
        ok = c['ref']['checked'] & (c['np_std'] > 0)
        narrow += int((c['np_std'][ok] < 1e-8 * np.abs(c['np_mean'][ok])).sum())
    assert narrow >= 20, narrow


def test_a_constant_column_is_exact():
    for n, E, Wp, ndim in [(1, 1, 1, 1), (9, 1, 5, 3), (37, 2, 100, 4)]:
        mean, std = ordered_moments(np.full((n, E * Wp, ndim), 0.25), E)
        assert (mean == 0.25).all() and (std == 0.0).all()


def test_ordered_moments_refuses_what_the_entry_point_refuses():
    with pytest.raises(ValueError):
        ordered_moments(np.zeros((4, 5, 2)), 2)
    with pytest.raises(ValueError):
        ordered_moments(np.zeros((4, 6)), 1)
    with pytest.raises(ValueError):
        ordered_moments(np.zeros((0, 6, 2)), 1)
