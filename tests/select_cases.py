"""What tests/test_select_cases.py and tests/test_gpu_columns.py share: the columns that drive the selection kernel of
bisip_amd/csrc/chain_columns.hip (k_segmented_select) down every path of its narrowing loop, the percentile lists, and a
census that shows on the host which path a column takes.

The expected percentiles of every column are ``np.percentile`` of the same doubles.  ``census`` mirrors the narrowing loop
of chain_columns.hip and must follow its ``SEL_CAP``; it says which inputs reach which path and is never compared with
what the device returns.
"""
import collections
import functools

import numpy as np

SEL_CAP = 192         # chain_columns.hip: survivors that are finished by counting
SEL_MAX_P = 8         # chain_columns.hip: percentiles per launch of the selection

KINDS = ('normal', 'dup', 'nested', 'lowbits', 'tiny', 'constant', 'infs', 'nan_pos', 'nan_neg')    # 'clusters': own n, own p
P8 = [0, 2.5, 50, 33.3, 97.5, 99.99, 100, 16]
P13 = P8 + [40, 45, 60, 84, 5]                        # selected as 8 + 5
P17 = P13 + [1, 66.6, 99, 75]                         # selected as 8 + 8 + 1
DUP_VALUE = 0.25
CONSTANT_VALUE = -3.75
TINY_VALUES = (0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, np.finfo(np.float64).tiny, -np.finfo(np.float64).tiny)

# Where the kernel changes its path: finish at once (n <= 192), registers <8> | <16> | <40> | from memory <0>, and in the
# memory form 0, 1, 2, 3 single blocks of 1024 after the four-loads-in-flight loop (43009 ... 45057) and a full multiple.
LENGTHS = (1, 2, 191, 192, 193, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385, 40959, 40960, 40961, 43009, 44033, 45057,
           46080)
DISPATCH_LENGTHS = (193, 8193, 16385, 40961)          # the first length of every path but <8>'s own start


def ranks(n, p):
    """``(lo, hi)`` of every percentile: the two order statistics NumPy's 'linear' rule interpolates between."""
    v = (n - 1) * (np.asarray(p, dtype=np.float64) / 100.0)
    lo = np.floor(v).astype(np.int64)
    return lo, np.minimum(lo + 1, n - 1)


def infs_planted(n):
    """``(n_neg, n_pos)`` of 'infs': with ``n_neg`` times -inf the lower neighbour of the 2.5th percentile is the last -inf
    and its upper neighbour the smallest finite value; with ``n_pos`` times +inf the upper neighbour of the 99.99th is the
    first +inf and its lower neighbour the largest finite value."""
    lo, hi = ranks(n, [2.5, 99.99])
    n_neg = int(lo[0]) + 1
    n_pos = n - int(hi[1]) if n > 1 else 0
    return n_neg, min(n_pos, n - n_neg)


def column(kind, n, seed):
    """One float64 column of ``n`` values."""
    rng = np.random.RandomState(seed)
    if kind == 'normal':
        return rng.standard_normal(n)
    if kind == 'dup':                 # a rank inside hundreds of equal values
        x = rng.standard_normal(n)
        x[rng.random_sample(n) < 0.6] = DUP_VALUE
        return x
    if kind == 'nested':              # the bulk stays in one slice of the range pass after pass
        x = 1.0 + rng.randint(0, 1 << 20, size=n) * 2.0 ** -52
        if n >= 2:
            at = rng.choice(n, 2, replace=False)
            x[at[0]] = -1e300
            if n >= 3:
                x[at[1]] = 1e300
        return x
    if kind == 'lowbits':             # an occupied range of at most 8 bits
        return 1.0 + rng.randint(0, 200, size=n) * 2.0 ** -52
    if kind == 'clusters':            # every percentile of cluster_percentiles between two clusters
        assert n % 9 == 0 and n > 0
        x = np.concatenate([10.0 ** (j - 4) * (1.0 + 1e-9 * rng.random_sample(n // 9)) for j in range(9)])
        rng.shuffle(x)
        return x
    if kind == 'tiny':                # subnormals, the smallest normals and both zeros
        return np.array(TINY_VALUES)[rng.randint(0, len(TINY_VALUES), size=n)]
    if kind == 'constant':
        return np.full(n, CONSTANT_VALUE)
    if kind == 'infs':
        x = rng.standard_normal(n)
        n_neg, n_pos = infs_planted(n)
        at = rng.choice(n, n_neg + n_pos, replace=False)
        x[at[:n_neg]] = -np.inf
        x[at[n_neg:]] = np.inf
        return x
    if kind in ('nan_pos', 'nan_neg'):
        x = rng.standard_normal(n)
        x[rng.randint(0, n)] = np.copysign(np.nan, 1.0 if kind == 'nan_pos' else -1.0)
        return x
    raise ValueError(kind)


def cluster_percentiles(n):
    """The eight percentiles of a 'clusters' column of ``n = 9 m`` values whose neighbours are the largest value of cluster
    k - 1 and the smallest of cluster k (virtual index ``k m - 0.5``)."""
    m = n // 9
    return [100.0 * (k * m - 0.5) / (n - 1) for k in range(1, 9)]


@functools.lru_cache(maxsize=None)
def columns(n, seed=0):
    """``(len(KINDS), n)``: one column of every kind but 'clusters', read-only."""
    cols = np.stack([column(kind, n, seed + 17 * i) for i, kind in enumerate(KINDS)])
    cols.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def clusters(n, seed=0):
    """The 'clusters' column of the largest multiple of 9 up to ``n`` (None below 9), read-only."""
    if n < 9:
        return None
    x = column('clusters', n // 9 * 9, seed + 1000)
    x.setflags(write=False)
    return x


def reference(cols, p):
    """``np.percentile(cols, p, axis=-1)`` without NumPy's warnings about inf - inf."""
    with np.errstate(invalid='ignore'):
        return np.percentile(cols, p, axis=-1)


def assert_matches_numpy(got, want, what=''):
    """The same doubles wherever NumPy's are finite, NaN in the same places, the same infinities.  The sign of a zero is not
    compared: NumPy's sort does not order -0.0 and 0.0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = np.isfinite(want)
    bad = np.argwhere(ok & (got != want))
    assert bad.size == 0, (what, 'first differences (index, got, want)',
                           [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:5]])
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN at', np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (what, 'infinities differ')


def plant_signs(full):
    """The 'signs' data of test_percentiles_by_selection_equal_the_sorted_ones (tests/test_gpu_batch.py), in place on a
    chain ``(n, E * Wp, ndim)``: tiny values of both signs, one +inf and one -inf per parameter, a sample of zeros."""
    full[::3] *= -1e-300
    full[1, 1, :] = np.inf
    full[2, 2, :] = -np.inf
    full[3, :, 0] = 0.0
    return full


def sort_then_lerp(cols, p):
    """The percentiles of ``cols (..., n)`` as the kernels take them: sort, then numpy.lib._function_base_impl._lerp
    between the two neighbours, one scalar at a time."""
    cols = np.asarray(cols, dtype=np.float64)
    n = cols.shape[-1]
    v = (n - 1) * (np.asarray(p, dtype=np.float64) / 100.0)
    lo, hi = ranks(n, p)
    srt = np.sort(cols, axis=-1)
    out = np.empty((len(p),) + cols.shape[:-1])
    with np.errstate(invalid='ignore'):
        for k in range(len(p)):
            x, y, t = srt[..., lo[k]], srt[..., hi[k]], v[k] - lo[k]
            d = y - x
            out[k] = y - d * (1.0 - t) if t >= 0.5 else x + d * t
        out[:, np.isnan(cols).any(axis=-1)] = np.nan
    return out


Census = collections.namedtuple('Census', 's passes ends ranges')


def select_keys(x):
    """The order-preserving 64-bit image of doubles (select_key.h)."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def census(col, p):
    """Which way ``col`` goes through the narrowing loop of k_segmented_select for the percentiles ``p`` (at most 8: one
    launch): ``s`` (open bits of key - min) at entry, the number of histogram passes, how it ends -- 'counting' (at most
    SEL_CAP survivors go to LDS), 'exact' (``s == 0``: every range is one key) or 'nan' -- and the number of distinct
    ranges the ranks end in.  A model of the loop only, to show what the inputs reach."""
    assert 1 <= len(p) <= SEL_MAX_P
    keys = select_keys(col)
    n = keys.size
    kmin, kmax = int(keys.min()), int(keys.max())
    if kmax > 0xfff0000000000000 or kmin < 0x000fffffffffffff:
        return Census(None, 0, 'nan', 0)
    s = (kmax - kmin).bit_length()
    s0 = s
    lo, hi = ranks(n, p)
    rem = [int(r) for pair in zip(lo, hi) for r in pair]
    base = [kmin] * len(rem)
    surv = [n] * len(rem)
    finish = n <= SEL_CAP
    passes = 0
    while not finish and s > 0:
        shift = s - 8 if s > 8 else 0
        hist = {}
        for b in set(base):
            d = keys - np.uint64(b)                     # wraps below the base, as the kernel's unsigned difference
            inside = d if s >= 64 else d[(d >> np.uint64(s)) == 0]
            hist[b] = np.bincount((inside >> np.uint64(shift)).astype(np.int64), minlength=256)
        for r in range(len(rem)):
            cum = np.cumsum(hist[base[r]])
            b = int(np.searchsorted(cum, rem[r], side='right'))
            rem[r] -= int(cum[b - 1]) if b else 0
            surv[r] = int(hist[base[r]][b])
            base[r] += b << shift
        s = shift
        passes += 1
        finish = sum(surv) <= SEL_CAP                   # ranks that share a range counted twice, as in the kernel
    return Census(s0, passes, 'exact' if s == 0 else 'counting', len(set(base)))
