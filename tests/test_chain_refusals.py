"""What the chain-summary entry points of libbisip_hip.so refuse, and in which words: one table with a row per entry point
(a sound argument list at a tiny shape, the entry's rules in the order it applies them with one fault each, and further
faults), walked fault by fault with the exception type and the whole message of each; pairs of faults adjacent in an
entry's order, of which the earlier rule must be the one reported; and what every ``..._workspace`` function returns for
the bad shapes of the table and for two sound ones.

Every call is refused on the host from its arguments alone, before the device is touched: the device pointers are made
up (4096) and never dereferenced, so the test needs no GPU.  A row that the library accepted would launch a kernel on
such a pointer; every row below is a refusal.  The host entry points (``..._host``) get real arrays.

Rows marked NEW pin the one rule that changed when the checks moved into csrc/chain_check.h: the product E * Wp * ndim of
the stride rule no longer overflows, and a product beyond int64 is refused as a stride that is too small."""
import ctypes

import numpy as np
import pytest

from bisip_amd import _hip

P = 4096                                   # a made-up device pointer
I31 = 0x7fffffff
V, U = ValueError, RuntimeError            # BISIP_EINVAL, BISIP_EUNSUPPORTED


def text(kind, message):
    return ('bisip_hip: ' if kind is V else 'bisip_hip (status -4): ') + message


NULL = 'null argument'
SHAPE = 'bad chain shape'
STRIDE = 'sample_stride smaller than one sample'
ITEMS = 'chain exceeds the 2^31 items of one sort'


def row(a):
    return a['E'] * a['Wp'] * a['ndim']


def short(a):
    return row(a) - 1


def ndim_text(a, tail=''):
    return f"ndim={a['ndim']} out of range{tail}"


def rtd_ndim_text(a):
    return ndim_text(a, ' (r0 and a_0 at least)')


def rows_text(a):
    return f"{a['E'] * a['Wp']} rows per sample exceed 2^31"


def grid_segments_text(a):                 # cov, best sample, bridge: segments of at most 2^30 rows from 256 ensembles on
    return f"{-(-a['n'] * a['Wp'] // (1 << 30))} segments of {a['E']} ensembles exceed one grid"


def hist_grid_text(a):
    return f"{a['E']} ensembles in 1 x 1 parts exceed one grid"


def short_work(a):
    return f"workspace of {a['nbytes']} bytes, need {a['nbytes'] + 1}"


def null_work(a):
    return f"workspace of 0 bytes, need {a['nbytes']}"


CHAIN = dict(chain=P, n=8, stride=row, E=1, Wp=8, ndim=3)
BIG = dict(n=1 << 20, E=1 << 10)                               # 2^20 x 8 x 2^10 x 3 values: more than 2^31
ROWS31 = dict(E=1 << 16, Wp=1 << 15)                           # 2^31 rows per sample
SEGMENTS = dict(n=I31, E=I31, Wp=I31 // 32)                    # the largest chain cov / best sample / bridge take
OVERFLOW = dict(E=I31, Wp=1 << 40, ndim=16, stride=1 << 62)    # NEW: E * Wp * ndim beyond int64


class Entry:
    """``name``: the C entry point without bisip_; ``order``: its arguments; ``ok``: a sound argument list (a callable is
    worked out from the others); ``rules``: (type, message, what to lay over ``ok``) in the entry's own order, one fault
    per rule; ``more``: further faults; ``new``: faults whose refusal is new with the shared stride rule."""

    def __init__(self, name, order, ok, rules, more=(), new=()):
        self.name, self.order, self.ok, self.rules, self.more, self.new = name, order.split(), ok, rules, more, new

    def args(self, over):
        a = dict(self.ok, **over)
        for k in sorted(a, key=lambda k: (k == 'nbytes', k != 'Wp')):       # Wp first, the bytes last: they follow the shape
            if callable(a[k]):
                a[k] = a[k](a)
        return a

    def call(self, a):
        keep, c = [], []
        for k in self.order:
            v = a[k]
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte if v.dtype == np.uint8 else ctypes.c_double))
            elif isinstance(v, list):
                v = (ctypes.c_int64 * max(1, len(v)))(*v)
            elif isinstance(v, int) and v == 0 and k in self.pointers:
                v = None
            c.append(v)
        _hip._check(getattr(_hip.load_library(), 'bisip_' + self.name)(*c))

    @property
    def pointers(self):
        return {k for k, v in self.ok.items() if isinstance(v, (np.ndarray, list)) or v == P} | {'work', 'window', 'index', 'thr'}

    def refused(self, kind, message, over):
        a = self.args(over)
        with pytest.raises(kind) as info:
            self.call(a)
        want = text(kind, message(a) if callable(message) else message)
        assert type(info.value) is kind and str(info.value) == want, (self.name, over)


def nulls(*names):
    return tuple((V, NULL, {k: 0}) for k in names)


def zeros(*names, message=SHAPE):
    return tuple((V, message, {k: 0}) for k in names)


def past(message=SHAPE, kind=V, **caps):
    """One past the cap the entry applies today."""
    return tuple((kind, message, {k: cap + 1}) for k, cap in caps.items())


def moments(name, extra):
    ok = dict(CHAIN, **{k: P for k in extra.split()}, work=P, stream=0)
    return Entry(name, 'chain n stride E Wp ndim ' + extra + ' work stream', ok,
                 rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short))),
                 more=nulls(*extra.split(), 'work') + ((V, ndim_text, dict(ndim=17)),) + zeros('E', 'Wp') + past(E=I31),
                 new=((V, STRIDE, OVERFLOW),))          # (no cap on Wp, none on n)


def rtd_descriptors(name, host):
    if host:
        ok = dict(CHAIN, chain=np.zeros(8 * 24), log_tau=np.zeros(4), n_tau=4, q=np.full(2, 0.5), n_q=2, out=np.zeros(8 * 8 * 4))
    else:
        ok = dict(CHAIN, log_tau=P, n_tau=4, q=P, n_q=2, out=P, stream=0)
    return Entry(name, 'chain n stride E Wp ndim log_tau n_tau q n_q out' + ('' if host else ' stream'), ok,
                 rules=((V, NULL, dict(chain=0)), (V, 'n_tau=0', dict(n_tau=0)), (V, 'n_q=0 out of range [1, 8]', dict(n_q=0)),
                        (V, rtd_ndim_text, dict(ndim=1)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short)),
                        (U, rows_text, ROWS31)),
                 more=nulls('log_tau', 'q', 'out') + ((V, 'n_q=9 out of range [1, 8]', dict(n_q=9)), (V, rtd_ndim_text, dict(ndim=17)))
                 + zeros('E', 'Wp'),
                 new=((V, STRIDE, OVERFLOW),))          # (no caps at all before the stride)


def mode_row(a):
    return a['E'] * a['Wp'] * (1 + 3 * a['n_modes'])


def mode_order(name, host):
    if host:
        ok = dict(chain=np.zeros(8 * 32), n=8, stride=mode_row, E=1, Wp=8, n_modes=1, key_group=1, ordered=np.zeros(8 * 32),
                  desc=np.zeros(8 * 24), moved=np.zeros(64, dtype=np.uint8))
    else:
        ok = dict(chain=P, n=8, stride=mode_row, E=1, Wp=8, n_modes=1, key_group=1, ordered=P, desc=P, moved=P, stream=0)
    return Entry(name, 'chain n stride E Wp n_modes key_group ordered desc moved' + ('' if host else ' stream'), ok,
                 rules=((V, NULL, dict(chain=0)), (V, 'no output asked for', dict(ordered=0, desc=0, moved=0)),
                        (V, 'n_modes=0 out of range [1, 5]', dict(n_modes=0)), (V, 'key_group=3 (0: m, 1: log_tau, 2: c)', dict(key_group=3)),
                        (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=lambda a: mode_row(a) - 1)), (U, rows_text, ROWS31)),
                 more=((V, 'n_modes=6 out of range [1, 5]', dict(n_modes=6)), (V, 'key_group=-1 (0: m, 1: log_tau, 2: c)', dict(key_group=-1)))
                 + zeros('E', 'Wp'),
                 new=((V, STRIDE, dict(E=I31, Wp=1 << 40, n_modes=5, stride=1 << 62)),))


def hist(name, extra, ok_extra, rules_after, more=()):
    ok = dict(CHAIN, **ok_extra, stream=0)
    return Entry(name, 'chain n stride E Wp ndim ' + extra + ' stream', ok,
                 rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short)))
                 + rules_after + ((U, hist_grid_text, dict(E=1 << 31)),),
                 more=nulls(*(k for k, v in ok_extra.items() if v == P)) + ((V, ndim_text, dict(ndim=17)),) + zeros('E', 'Wp') + more,
                 new=((V, STRIDE, OVERFLOW),))          # (no caps before the stride; the grid rule comes after it)


def ess_need(a):
    return _hip.chain_ess_workspace(a['n'], a['E'], a['Wp'], a['ndim'], a['splits'], a.get('n_thr', 0))


def samples_text(a):
    return f"n_samples={a['n']}: a chain needs 2 samples, a half too"


ESS_RULES = ((V, ndim_text, dict(ndim=0)), (V, 'splits=3: 1 or 2', dict(splits=3)), (V, samples_text, dict(n=1)), (V, SHAPE, dict(E=0)),
             (V, STRIDE, dict(stride=short)), (V, short_work, dict(nbytes=lambda a: ess_need(a) - 1)))
# n: 32-bit sample numbers; E: a scan workgroup per (threshold, ensemble, parameter) of up to 8 thresholds; Wp: the groups
# of 256 chains of both halves within grid dimension y
ESS_MORE = ((V, ndim_text, dict(ndim=17)), (V, 'splits=0: 1 or 2', dict(splits=0)), (V, samples_text, dict(n=3)), (V, samples_text, dict(n=0))) \
    + zeros('Wp') + past(n=I31, E=I31 // (3 * 8), Wp=65535 * 256 // 2)


def ess(name, extra, ok_extra, first_rules=(), more=()):
    ok = dict(CHAIN, splits=2, **ok_extra, ess=P, work=P, nbytes=ess_need, stream=0)
    return Entry(name, 'chain n stride E Wp ndim splits ' + extra + ' ess work nbytes stream', ok,
                 rules=((V, NULL, dict(chain=0)),) + first_rules + ESS_RULES, more=nulls('ess', 'work') + ESS_MORE + more)


def rank_need(a):
    return _hip.chain_rank_normalize_workspace(a['n'], a['E'], a['Wp'], a['ndim'])


def rank(name, extra):
    ok = dict(CHAIN, **{k: P for k in extra.split()}, z=P, work=P, nbytes=rank_need, stream=0)
    return Entry(name, 'chain n stride E Wp ndim ' + extra + ' z work nbytes stream', ok,
                 rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(Wp=0)), (U, ITEMS, BIG),
                        (V, STRIDE, dict(stride=short)), (V, short_work, dict(nbytes=lambda a: rank_need(a) - 1))),
                 more=nulls(*extra.split(), 'z', 'work') + ((V, ndim_text, dict(ndim=17)),) + zeros('n', 'E')
                 + past(ITEMS, U, n=I31, E=I31, Wp=I31))


def trace_need(a):
    return _hip.chain_trace_workspace(a['n'], a['E'], a['Wp'], a['ndim'], a['n_p'])


def gathered(a):
    return _hip.chain_trace_lds_walkers(a['ndim']) + 1           # the first ensemble too wide for the LDS path


def hdi_need(a):
    return _hip.chain_hdi_workspace(a['n'], a['E'], a['Wp'], a['ndim'], a['windows'])


def cov_need(a):
    return _hip.chain_cov_workspace(a['n'], a['E'], a['Wp'], a['ndim'])


def best_need(a):
    return _hip.chain_best_sample_workspace(a['n'], a['E'], a['Wp'])


def rhat_need(a):
    return _hip.chain_rhat_workspace(a['n'], a['E'], a['Wp'], a['ndim'], a['splits'])


def window_text(a):
    return f"window 0 of {a['windows'][0]} steps outside [1, N - 1], N = {a['n'] * a['Wp']}"


ENTRIES = (
    moments('chain_moments_dev', 'mean std'),
    moments('chain_central_moments_dev', 'center m2 m4'),
    Entry('chain_percentiles_dev', 'chain n stride E Wp ndim pct n_p out work nbytes stream',
          dict(CHAIN, pct=np.array([50.0]), n_p=1, out=P, work=P, nbytes=1 << 40, stream=0),
          rules=((V, ndim_text, dict(ndim=0)), (V, NULL, dict(chain=0)), (V, 'bad shape', dict(n=0)), (V, STRIDE, dict(stride=short)),
                 (U, lambda a: f"chain of {a['n'] * row(a)} values exceeds the 2^31 items of one sort", BIG),
                 (V, 'percentiles must be in [0, 100]', dict(pct=np.array([101.0])))),
          more=nulls('pct', 'out', 'work') + ((V, ndim_text, dict(ndim=17)),) + zeros('E', 'Wp', 'n_p', message='bad shape')
          + past('bad shape', n_p=1024) + ((V, 'percentiles must be in [0, 100]', dict(pct=np.array([np.nan]))),),
          new=((V, STRIDE, OVERFLOW),)),                 # (no caps before the stride)
    Entry('chain_autocorr_time_dev', 'chain n stride E Wp ndim c tau window work stream',
          dict(CHAIN, c=5.0, tau=P, window=0, work=P, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short)),
                 (V, 'c=0: the window factor must be finite and > 0', dict(c=0.0))),
          # E: a window workgroup per (ensemble, parameter); Wp: the groups of 256 walkers within grid dimension y
          more=nulls('tau', 'work') + ((V, ndim_text, dict(ndim=17)),) + zeros('E', 'Wp') + past(E=I31 // 3, Wp=65535 * 256)
          + ((V, 'c=inf: the window factor must be finite and > 0', dict(c=float('inf'))),
             (V, 'c=-1: the window factor must be finite and > 0', dict(c=-1.0)))),
    Entry('rtd_integrals_dev', 'chain n stride E Wp ndim power_sums norm_factor out stream',
          dict(CHAIN, power_sums=P, norm_factor=P, out=P, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, rtd_ndim_text, dict(ndim=1)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short)),
                 (U, rows_text, ROWS31)),
          more=nulls('power_sums', 'norm_factor', 'out') + ((V, rtd_ndim_text, dict(ndim=17)),) + zeros('E', 'Wp'),
          new=((V, STRIDE, OVERFLOW),)),
    Entry('rtd_columns_dev', 'chain n stride E Wp ndim first count log_tau n_tau cols stream',
          dict(CHAIN, first=0, count=1, log_tau=P, n_tau=4, cols=P, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, 'n_tau=0', dict(n_tau=0)),
                 (V, lambda a: f"ensembles [{a['first']}, {a['first'] + a['count']}) outside [0, {a['E']})", dict(count=0)),
                 (U, rows_text, ROWS31), (V, rtd_ndim_text, dict(ndim=1)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short))),
          more=nulls('log_tau', 'cols') + ((V, 'ensembles [1, 2) outside [0, 1)', dict(first=1)),
                                           (V, 'ensembles [-1, 0) outside [0, 1)', dict(first=-1)),
                                           (V, 'ensembles [0, 1) outside [0, 0)', dict(E=0)),       # (before the shape)
                                           (V, rtd_ndim_text, dict(ndim=17))) + zeros('Wp'),
          # NEW: here the rows of a sample come before the stride, and their product is taken without overflow as well
          new=((U, f'{(1 << 63) - 1} rows per sample exceed 2^31', OVERFLOW),)),
    rtd_descriptors('rtd_descriptors_dev', False),
    rtd_descriptors('rtd_descriptors_host', True),
    mode_order('mode_order_dev', False),
    mode_order('mode_order_host', True),
    hist('chain_range_dev', 'out nonfinite', dict(out=P, nonfinite=P), ()),
    hist('chain_histograms_dev', 'edges bins counts', dict(edges=P, bins=4, counts=P),
         ((V, 'bins=0', dict(bins=0)),
          (U, 'bins=2000: the edges and counters of 3 parameters take 72024 bytes of LDS, more than 65536', dict(bins=2000)))),
    hist('chain_pair_histograms_dev', 'edges bins counts', dict(edges=P, bins=4, counts=P),
         ((V, 'ndim=1 has no pairs', dict(ndim=1)), (V, 'bins=0', dict(bins=0)),
          (U, 'bins=1025: the 1025 x 1025 counters of one pair do not fit 65536 bytes of LDS', dict(bins=1025))),
         more=((U, 'bins=128: the 128 x 128 counters of one pair do not fit 65536 bytes of LDS', dict(bins=128)),)),
    Entry('chain_trace_dev', 'chain n stride E Wp ndim pct n_p out mean work nbytes stream',
          dict(CHAIN, pct=np.array([50.0]), n_p=1, out=P, mean=P, work=0, nbytes=0, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, 'n_percentiles=9: 0 ... 8 per call', dict(n_p=9)),
                 (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short)),
                 (V, 'neither percentiles nor the mean asked for', dict(pct=0, n_p=0, mean=0)),
                 (V, 'percentiles must be in [0, 100]', dict(pct=np.array([101.0]))),
                 (V, short_work, dict(Wp=gathered, work=P, nbytes=lambda a: trace_need(a) - 1))),
          more=nulls('pct', 'out') + ((V, ndim_text, dict(ndim=17)), (V, 'n_percentiles=-1: 0 ... 8 per call', dict(n_p=-1)))
          + zeros('E', 'Wp') + past(E=I31, Wp=I31)
          + ((V, null_work, dict(Wp=gathered, nbytes=trace_need)),
             (U, '2147483648 samples x 1 workgroups exceed one grid', dict(n=1 << 31)),
             (U, lambda a: f"one sample of {I31} x {a['Wp']} walkers exceeds one grid", dict(E=I31, Wp=gathered)))),
    Entry('chain_rhat_dev', 'chain n stride E Wp ndim splits mean var rhat work nbytes stream',
          dict(CHAIN, splits=2, mean=P, var=P, rhat=P, work=P, nbytes=rhat_need, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, 'none of mean, variance and R-hat asked for', dict(mean=0, var=0, rhat=0)),
                 (V, ndim_text, dict(ndim=0)), (V, 'splits=3: 1 or 2', dict(splits=3)), (V, SHAPE, dict(E=0)), (V, samples_text, dict(n=1)),
                 (V, 'R-hat needs 2 chains', dict(splits=1, Wp=1)), (V, STRIDE, dict(stride=short)),
                 (V, short_work, dict(nbytes=lambda a: rhat_need(a) - 1))),
          # E: grid dimension x of the R-hat stage; Wp: 32-bit column numbers of 2 * BISIP_MAX_NDIM columns per walker
          more=((V, ndim_text, dict(ndim=17)), (V, samples_text, dict(n=3)), (V, samples_text, dict(n=0))) + zeros('Wp')
          + past(E=I31, Wp=I31 // 32)
          + ((V, null_work, dict(work=0)),
             (U, lambda a: f'{row(a)} columns exceed one grid', dict(E=I31, Wp=I31 // 32)))),
    Entry('chain_cov_dev', 'chain n stride E Wp ndim mean cov work nbytes stream',
          dict(CHAIN, mean=P, cov=P, work=0, nbytes=0, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(E=0)),
                 (V, 'a covariance needs 2 rows, got n_samples * walkers_per_ensemble = 1', dict(n=1, Wp=1)),
                 (V, STRIDE, dict(stride=short)), (U, grid_segments_text, SEGMENTS)),
          # n, E: 32-bit; Wp: 32-bit element numbers within 2 * BISIP_MAX_NDIM walkers' rows
          more=nulls('cov') + ((V, ndim_text, dict(ndim=17)),) + zeros('n', 'Wp') + past(n=I31, E=I31, Wp=I31 // 32)
          + ((V, short_work, dict(n=200, work=P, nbytes=lambda a: cov_need(a) - 1)), (V, null_work, dict(n=200, nbytes=cov_need)))),
    Entry('chain_best_sample_dev', 'chain stride logp lstride n E Wp ndim theta best index work nbytes stream',
          dict(CHAIN, logp=P, lstride=lambda a: a['E'] * a['Wp'], theta=P, best=P, index=P, work=0, nbytes=0, stream=0),
          rules=((V, NULL, dict(logp=0)), (V, 'none of theta, log-probability and index asked for', dict(theta=0, best=0, index=0)),
                 (V, 'theta asked for without a chain', dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(n=0)),
                 (V, 'logp_stride smaller than one sample', dict(lstride=lambda a: a['E'] * a['Wp'] - 1)),
                 (V, 'chain_stride smaller than one sample', dict(stride=short)), (U, grid_segments_text, SEGMENTS)),
          more=((V, ndim_text, dict(ndim=17)),) + zeros('E', 'Wp') + past(n=I31, E=I31, Wp=I31 // 32)
          + ((V, short_work, dict(n=20000, work=P, nbytes=lambda a: best_need(a) - 1)), (V, null_work, dict(n=20000, nbytes=best_need)))),
    Entry('chain_hdi_dev', 'chain n stride E Wp ndim windows n_w out index work nbytes stream',
          dict(CHAIN, windows=[32], n_w=lambda a: len(a['windows'] or [0]), out=P, index=0, work=P, nbytes=hdi_need, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(E=0)),
                 (V, 'n_windows=0 out of range (1 ... 8)', dict(n_w=0)), (U, ITEMS, dict(n=1 << 31)), (V, window_text, dict(windows=[0])),
                 (V, STRIDE, dict(stride=short)), (V, short_work, dict(nbytes=lambda a: hdi_need(a) - 1))),
          # (no cap is a bad shape: beyond 32 bits the chain is unsupported, after the windows are counted)
          more=nulls('windows', 'out', 'work') + ((V, ndim_text, dict(ndim=17)),) + zeros('n', 'Wp')
          + ((V, 'n_windows=9 out of range (1 ... 8)', dict(windows=[32] * 9)), (V, window_text, dict(windows=[64])))
          + past(ITEMS, U, E=I31, Wp=I31) + ((U, ITEMS, BIG),)),
    ess('chain_ess_dev', 'thr n_thr', dict(thr=0, n_thr=0),
        first_rules=((V, 'n_threshold=1: 1 ... 8 with thresholds, 0 without', dict(n_thr=1)),),
        more=((V, 'n_threshold=0: 1 ... 8 with thresholds, 0 without', dict(thr=P)),
              (V, 'n_threshold=9: 1 ... 8 with thresholds, 0 without', dict(thr=P, n_thr=9)))),
    ess('chain_ess_squares_dev', 'center', dict(center=P), more=nulls('center')),
    rank('chain_rank_normalize_dev', ''),
    rank('chain_rank_normalize_folded_dev', 'center'),
    Entry('bridge_logg_dev', 'chain n stride E Wp ndim logp lstride mean chol const l stream',
          dict(CHAIN, logp=P, lstride=lambda a: a['E'] * a['Wp'], mean=P, chol=P, const=P, l=P, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, ndim_text, dict(ndim=0)), (V, SHAPE, dict(n=0)), (V, STRIDE, dict(stride=short)),
                 (V, 'logp_stride smaller than one sample', dict(lstride=lambda a: a['E'] * a['Wp'] - 1)),
                 (U, grid_segments_text, SEGMENTS)),
          # the caps of chain_cov_dev: the kernel walks rows as the covariance does
          more=nulls('logp', 'mean', 'chol', 'const', 'l') + ((V, ndim_text, dict(ndim=17)),) + zeros('E', 'Wp')
          + past(n=I31, E=I31, Wp=I31 // 32)),
    Entry('chain_shell_rows_dev', 'chain logp n E Wp ndim k n_stride ties out work stream',
          dict(chain=P, logp=P, n=8, E=1, Wp=8, ndim=3, k=2, n_stride=0, ties=1, out=P, work=P, stream=0),
          rules=((V, NULL, dict(chain=0)), (V, SHAPE, dict(n=0)), (V, ndim_text, dict(ndim=0)),
                 (V, 'k=0 / n_stride=0 out of range', dict(k=0)), (U, 'more than 2^31 samples per ensemble', dict(n=1 << 20, Wp=1 << 12))),
          more=nulls('logp', 'out', 'work') + zeros('E', 'Wp') + past(E=I31) + ((V, ndim_text, dict(ndim=17)),)
          + tuple((V, f"k={o.get('k', 2)} / n_stride={o.get('n_stride', 0)} out of range", o)
                  for o in (dict(k=(1 << 20) + 1), dict(n_stride=-1), dict(n_stride=257), dict(n_stride=9)))),
)

# the entry points of the issue, one row each
assert [e.name for e in ENTRIES] == (
    'chain_moments_dev chain_central_moments_dev chain_percentiles_dev chain_autocorr_time_dev rtd_integrals_dev rtd_columns_dev '
    'rtd_descriptors_dev rtd_descriptors_host mode_order_dev mode_order_host chain_range_dev chain_histograms_dev '
    'chain_pair_histograms_dev chain_trace_dev chain_rhat_dev chain_cov_dev chain_best_sample_dev chain_hdi_dev chain_ess_dev '
    'chain_ess_squares_dev chain_rank_normalize_dev chain_rank_normalize_folded_dev bridge_logg_dev chain_shell_rows_dev').split()

by_name = pytest.mark.parametrize('entry', ENTRIES, ids=lambda e: e.name)


@by_name
def test_one_fault(entry):
    for kind, message, over in entry.rules + tuple(entry.more):
        entry.refused(kind, message, over)


@by_name
def test_one_fault_new_with_the_shared_stride_rule(entry):
    """NEW: these argument lists overflowed the product of the stride rule before (undefined behaviour)."""
    for kind, message, over in entry.new:
        entry.refused(kind, message, over)


@by_name
def test_of_two_faults_the_earlier_rule_is_reported(entry):
    """Every pair of rules adjacent in the entry's order, both broken at once.  (A pair whose faults need the same argument
    cannot be laid over one another and is left out.)"""
    walked = 0
    for (kind, message, first), (_, _, second) in zip(entry.rules, entry.rules[1:]):
        if set(first) & set(second):
            continue
        entry.refused(kind, message, dict(second, **first))
        walked += 1
    assert walked >= len(entry.rules) - 2, entry.name


def test_the_number_of_refusals():
    """What the summary of the change that moved the checks quotes."""
    single = sum(len(e.rules) + len(e.more) for e in ENTRIES)
    new = sum(len(e.new) for e in ENTRIES)
    pairs = sum(not set(a[2]) & set(b[2]) for e in ENTRIES for a, b in zip(e.rules, e.rules[1:]))
    print(f'{single} single faults, {new} new ones, {pairs} pairs')
    assert (single, new, pairs) == (349, 12, 129)


# ---------------------------------------------------------------------------------------------------------------------------
# the ..._workspace functions: what they return for the bad shapes of the table (0 for some, negative for others) and the
# bytes (doubles, for the two moments functions) of two sound shapes.  bisip_chain_percentiles_workspace is not here, and
# bisip_chain_percentiles_dev has no row for a short workspace: both ask the sort for its scratch, which needs a device.
# ---------------------------------------------------------------------------------------------------------------------------
def bad_shapes(sound, caps=(), lo_ndim=0):
    """``sound`` (n, E, Wp, ndim) with each count at 0, ndim at lo_ndim and 17, and each count one past its cap."""
    n, E, Wp, ndim = sound
    out = [(0, E, Wp, ndim), (n, 0, Wp, ndim), (n, E, 0, ndim), (n, E, Wp, lo_ndim), (n, E, Wp, 17)]
    for at, cap in caps:
        s = list(sound)
        s[at] = cap + 1
        out.append(tuple(s))
    return out


S = (8, 1, 8, 3)
WORKSPACES = (
    # function, arguments after (n, E, Wp, ndim), what is dropped of those four, bad shapes -> value, sound shapes -> value
    ('chain_moments_workspace', (), (2,), {s: 0 for s in bad_shapes(S)[:2] + bad_shapes(S)[3:4]}, {S: 6, (400, 3, 8, 5): 1500}),
    ('chain_central_moments_workspace', (), (2,), {s: 0 for s in bad_shapes(S)[:2] + bad_shapes(S)[3:4]}, {S: 12, (400, 3, 8, 5): 3000}),
    ('chain_autocorr_time_workspace', (), (), {s: 0 for s in bad_shapes(S, ((1, I31 // 3), (2, 65535 * 256)))},
     {S: 14848, (400, 3, 8, 5): 486400}),
    ('chain_trace_workspace', (1,), (), {s: -1 for s in bad_shapes(S, ((1, I31), (2, I31)))}, {S: 0, (40, 3, 2000, 5): 9600000}),
    ('chain_rhat_workspace', (2,), (), {s: -1 for s in bad_shapes(S, ((1, I31), (2, I31 // 32)))}, {S: 768, (400, 3, 8, 5): 30720}),
    ('chain_cov_workspace', (), (), {s: -1 for s in bad_shapes(S, ((0, I31), (1, I31), (2, I31 // 32)))}, {S: 0, (400, 3, 8, 5): 1920}),
    ('chain_best_sample_workspace', (), (3,), {s: -1 for s in bad_shapes(S, ((0, I31), (1, I31), (2, I31 // 32)))[:3]
                                              + bad_shapes(S, ((0, I31), (1, I31), (2, I31 // 32)))[5:]}, {S: 0, (40000, 3, 8, 5): 3792}),
    ('chain_hdi_workspace', ([32],), (), {s: -1 for s in bad_shapes(S, ((0, I31), (1, I31), (2, I31)))}, {S: 70400, (400, 3, 8, 5): 1217792}),
    ('chain_ess_workspace', (2, 0), (), {s: 0 for s in bad_shapes(S, ((0, I31), (1, I31 // (3 * 8)), (2, 65535 * 256 // 2)))},
     {S: 28416, (400, 3, 8, 5): 529920}),
    ('chain_rank_normalize_workspace', (), (), {s: 0 for s in bad_shapes(S, ((0, I31), (1, I31), (2, I31)))}, {S: 70400, (400, 3, 8, 5): 1217792}),
)


@pytest.mark.parametrize('row_', WORKSPACES, ids=lambda r: r[0])
def test_workspace_functions(row_):
    name, extra, dropped, bad, sound = row_
    for shape, want in list(bad.items()) + list(sound.items()):
        args = [v for i, v in enumerate(shape) if i not in dropped]
        assert getattr(_hip, name)(*args, *extra) == want, (name, shape)


def test_workspace_functions_with_rules_of_their_own():
    assert _hip.chain_rhat_workspace(8, 1, 8, 3, 3) == -1 and _hip.chain_rhat_workspace(3, 1, 8, 3, 2) == -1
    assert _hip.chain_rhat_workspace(8, 1, 1, 3, 1) == -1                       # one chain
    assert _hip.chain_rhat_workspace(8, I31, I31 // 32, 3, 2) == -1             # the columns exceed one grid
    assert _hip.chain_cov_workspace(1, 1, 1, 3) == -1                           # one row
    assert _hip.chain_cov_workspace(I31, I31, I31 // 32, 3) == -1 and _hip.chain_best_sample_workspace(I31, I31, I31 // 32) == -1
    assert _hip.chain_trace_workspace(8, 1, 8, 3, 9) == -1 and _hip.chain_trace_workspace(8, 1, 8, 3, -1) == -1
    assert _hip.chain_trace_workspace(8, 1, 8, 3, 0) == 0
    assert _hip.chain_trace_workspace(8, I31, _hip.chain_trace_lds_walkers(3) + 1, 3, 1) == -1      # one sample exceeds a grid
    for windows in ([], [32] * 9, [0], [64]):
        assert _hip.chain_hdi_workspace(8, 1, 8, 3, windows) == -1
    assert _hip.chain_hdi_workspace(1 << 20, 1 << 10, 8, 3, [32]) == -1 and _hip.chain_rank_normalize_workspace(1 << 20, 1 << 10, 8, 3) == 0
    assert _hip.chain_ess_workspace(8, 1, 8, 3, 3) == 0 and _hip.chain_ess_workspace(3, 1, 8, 3, 2) == 0
    assert _hip.chain_ess_workspace(8, 1, 8, 3, 2, 9) == 0 and _hip.chain_ess_workspace(8, 1, 8, 3, 2, -1) == 0
    assert _hip.chain_ess_workspace(8, 1, 8, 3, 2, 8) > _hip.chain_ess_workspace(8, 1, 8, 3, 2, 1) == _hip.chain_ess_workspace(8, 1, 8, 3, 2, 0)
    assert _hip.chain_shell_rows_workspace(0) == 0 and _hip.chain_shell_rows_workspace(512) == 16
    assert _hip.chain_shell_rows_workspace(1) > 0 and _hip.chain_shell_rows_workspace(511) == 511 * _hip.chain_shell_rows_workspace(1)
