#!/usr/bin/env python3
"""Effective sample size of device-resident chains (bisip_chain_ess_dev, bisip_chain_rank_normalize_dev).

The three shapes of trace_bench.py: the survey (512 spectra x 256 walkers x 500 samples x 7), the quickstart (one
ensemble of 32 walkers x 5000 x 7) and cfg4 (one ensemble of 32,768 walkers x 200 x 7).  The chain is CORRELATED: an AR(1)
made on the device with rho spread over 0 ... 0.95 across the parameters (an iid chain ends every Geyer sequence at lag 1
and measures nothing).  Per shape, in one run with the calls alternating, device events around each call after warm-up,
medians of --reps (5):
  * ess_mean_ms: bisip_chain_ess_dev on the values (splits = 2); rank_ms: bisip_chain_rank_normalize_dev;
  * ess_bulk_ms: both, as ess.device_ess(kind='bulk') takes them; ess_tail_ms: ess.device_ess(kind='tail'), the
    quantiles, one thresholded call for both indicators, and the copies back;
  * the yardsticks from code that was there before, on the same chain: autocorr_ms (bisip_chain_autocorr_time_dev: the
    same lag-sum work, stopped by emcee's window), sort_ms (bisip_chain_percentiles_dev forced through its sort: gather
    plus sort, the floor of the rank pass), moments_ms (bisip_chain_moments_dev);
  * the host path: bisip_amd.ess.ess (NumPy) on a get_chain-like copy of 8 spectra (or 1/16 of the walkers of a lone
    ensemble), extrapolated linearly and labelled as such; and the last lag the sequences of that subset took.
  * the diagnostics (bisip_amd.diagnostics) beside the call each is built on: rank_folded_ms
    (bisip_chain_rank_normalize_folded_dev about the medians) beside rank_ms, ess_squares_ms (bisip_chain_ess_squares_dev
    about the mean) beside ess_mean_ms, central_moments_ms (bisip_chain_central_moments_dev) beside moments_ms,
    rank_rhat_ms (device_rank_rhat), summary_ms (device_summary) beside separate_ms, the seven getters' drivers one after
    the other (moments, HDI, bulk and tail ESS, mcse_mean, mcse_sd, rank_rhat); every one with the spread of its repeats
    (``*_ms_spread``: largest minus smallest) and the last lag the squares' sequences of the host subset took.
With --profile a separate `rocprofv3 --kernel-trace --stats` run of the calls alone gives the time per kernel, and one of a
single device_summary says how its time splits into rank passes, ESS rounds, HDI and the rest (summary_split_ms).
Prints one JSON line per shape; with --out DIR also writes them (and the traces) there."""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_bench import SHAPES      # noqa: E402


def make_ar1_chain(E, Wp, ndim, n, seed=0):
    """AR(1) in stationarity, rho = linspace(0, 0.95, ndim) across the parameters, a centre per (ensemble, parameter)."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    rho = torch.linspace(0.0, 0.95, ndim, dtype=torch.float64, device='cuda')
    centre = torch.rand((E, 1, ndim), generator=g, dtype=torch.float64, device='cuda')
    x = torch.empty((n, E * Wp, ndim), dtype=torch.float64, device='cuda')
    cur = torch.randn((E, Wp, ndim), generator=g, dtype=torch.float64, device='cuda') / torch.sqrt(1.0 - rho * rho)
    for s in range(n):
        if s:
            cur = rho * cur + torch.randn((E, Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
        x[s] = (centre + 0.01 * cur).reshape(E * Wp, ndim)
    return x


class Calls:
    """The calls on one chain, outputs and workspaces of the C entry points allocated once."""

    def __init__(self, x, E, Wp, ndim):
        import torch
        from bisip_amd import _hip, diagnostics, ess
        from bisip_amd.chainview import ChainView
        self.hip, self.ess, self.dg, self.x, self.E, self.Wp, self.ndim = _hip, ess, diagnostics, x, E, Wp, ndim
        self.n = n = int(x.shape[0])
        self.ptr, self.stride = x.data_ptr(), E * Wp * ndim
        self.st = torch.cuda.current_stream().cuda_stream
        self.view = ChainView(x, n, E, Wp, ndim)
        dev = x.device

        def scratch(nbytes):
            return torch.empty((max(1, nbytes),), dtype=torch.uint8, device=dev)

        self.out = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.out2 = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.ess_bytes = _hip.chain_ess_workspace(n, E, Wp, ndim, 2)
        self.ess_work = scratch(self.ess_bytes)
        self.rank_bytes = _hip.chain_rank_normalize_workspace(n, E, Wp, ndim)
        self.rank_work = scratch(self.rank_bytes)
        self.z = torch.empty_like(x) if self.rank_bytes > 0 else None
        self.tau = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.ac_work = scratch(_hip.chain_autocorr_time_workspace(n, E, Wp, ndim))
        self.p = np.linspace(1.0, 99.0, 9)          # (the forced sort takes any count; 9 is past the selection's 8)
        self.pct = torch.empty((self.p.size, E, ndim), dtype=torch.float64, device=dev)
        self.pct_bytes = _hip.chain_percentiles_workspace(n, E, Wp, ndim, self.p.size)
        self.pct_work = scratch(self.pct_bytes)
        self.mean = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.std = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.mwork = torch.empty((max(1, _hip.chain_moments_workspace(n, E, ndim)),), dtype=torch.float64, device=dev)
        # the diagnostics: the medians and the means they are taken about, once
        from bisip_amd.chainview import device_moments, device_percentiles
        self.median = self.view.upload(device_percentiles(self.view, (50.0,))[0])
        self.centre = self.view.upload(device_moments(self.view)[0])
        self.m2 = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.m4 = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.cwork = torch.empty((max(1, _hip.chain_central_moments_workspace(n, E, ndim)),), dtype=torch.float64, device=dev)

    def ess_mean(self):
        self.hip.chain_ess_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, 2, 0, 0, self.out.data_ptr(),
                               self.ess_work.data_ptr(), self.ess_bytes, self.st)

    def rank(self):
        if self.z is None:
            self.ess.device_rank_normalize(self.view)
        else:
            self.hip.chain_rank_normalize_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.z.data_ptr(),
                                              self.rank_work.data_ptr(), self.rank_bytes, self.st)

    def ess_bulk(self):
        self.bulk = self.ess.device_ess(self.view, 'bulk')

    def ess_tail(self):
        self.tail = self.ess.device_ess(self.view, 'tail')

    def autocorr(self):
        self.hip.chain_autocorr_time_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, 5.0,
                                         self.tau.data_ptr(), 0, self.ac_work.data_ptr(), self.st)

    def sort(self):
        os.environ['BISIP_PERCENTILE_SORT'] = '1'
        try:
            self.hip.chain_percentiles_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.p,
                                           self.pct.data_ptr(), self.pct_work.data_ptr(), self.pct_bytes, self.st)
        finally:
            del os.environ['BISIP_PERCENTILE_SORT']

    def moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                                   self.std.data_ptr(), self.mwork.data_ptr(), self.st)


    def rank_folded(self):
        if self.z is None:
            self.ess.device_rank_normalize(self.view, center=self.median.cpu().numpy())
        else:
            self.hip.chain_rank_normalize_folded_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim,
                                                     self.median.data_ptr(), self.z.data_ptr(), self.rank_work.data_ptr(),
                                                     self.rank_bytes, self.st)

    def ess_squares(self):
        self.hip.chain_ess_squares_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, 2, self.centre.data_ptr(),
                                       self.out2.data_ptr(), self.ess_work.data_ptr(), self.ess_bytes, self.st)

    def central_moments(self):
        self.hip.chain_central_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.centre.data_ptr(),
                                           self.m2.data_ptr(), self.m4.data_ptr(), self.cwork.data_ptr(), self.st)

    def rank_rhat(self):
        self.rhat = self.dg.device_rank_rhat(self.view)

    def summary(self):
        self.table = self.dg.device_summary(self.view)

    def separate(self):
        """What the seven getters run: get_param_mean, get_param_hdi, get_ess('bulk'), get_ess('tail'), get_mcse_mean,
        get_mcse_sd, get_rank_rhat."""
        from bisip_amd.chainview import device_moments
        from bisip_amd.interval import device_hdi
        device_moments(self.view)
        device_hdi(self.view, 0.95)
        self.ess.device_ess(self.view, 'bulk')
        self.ess.device_ess(self.view, 'tail')
        self.ess.device_mcse_mean(self.view)
        self.dg.device_mcse_sd(self.view)
        self.dg.device_rank_rhat(self.view)


NAMES = ('ess_mean', 'rank', 'ess_bulk', 'ess_tail', 'autocorr', 'sort', 'moments', 'rank_folded', 'ess_squares',
         'central_moments', 'rank_rhat', 'summary', 'separate')


def time_alternating(c, reps):
    """Every call once per repetition, in turn; device events around each.  ``{name: (median, best)}`` in ms."""
    import torch
    for name in NAMES:                      # warm-up: code objects, the sort's plan, the allocator's blocks
        getattr(c, name)()
    torch.cuda.synchronize()
    times = {name: [] for name in NAMES}
    for _ in range(reps):
        for name in NAMES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            getattr(c, name)()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: (float(np.median(v)), float(np.min(v)), float(np.max(v) - np.min(v))) for name, v in times.items()}


def host_path(c, host_subset):
    """ess.ess in NumPy on a host copy of a subset of the chain, extrapolated by its share."""
    es = c.ess
    E, Wp, ndim = c.E, c.Wp, c.ndim
    if E > 1:
        k = min(E, host_subset)
        part, scale, wk = c.x[:, :k * Wp], E / k, Wp
    else:
        k, wk = 1, max(2, Wp // 16)
        part, scale = c.x[:, :wk], Wp / wk
    t0 = time.perf_counter()
    sub = part.cpu().numpy()
    copy_s = time.perf_counter() - t0
    res = dict(host_subset_values=int(sub.size), host_copy_subset_s=copy_s, host_copy_extrapolated_s=copy_s * scale,
               host_note='extrapolated linearly from the subset, not measured on the whole chain')
    got = {}
    for kind in es.KINDS:
        t0 = time.perf_counter()
        got[kind] = np.stack([es.ess(sub[:, e * wk:(e + 1) * wk], kind) for e in range(k)])
        s = time.perf_counter() - t0
        res[f'host_ess_{kind}_subset_s'], res[f'host_ess_{kind}_extrapolated_s'] = s, s * scale
    last = [es.ess_of_chains(es._chains(sub[:, e * wk:(e + 1) * wk], True)[:, :, d], margins=True)[3]
            for e in range(k) for d in range(ndim)]
    res['host_subset_last_lag_max'] = int(max(last))
    res['host_subset_last_lag_by_parameter'] = [int(max(last[d::ndim])) for d in range(ndim)]
    centre = c.centre.cpu().numpy()
    sq = [(sub[:, e * wk:(e + 1) * wk] - centre[e if E > 1 else 0]) ** 2 for e in range(k)]
    last = [es.ess_of_chains(es._chains(sq[e], True)[:, :, d], margins=True)[3] for e in range(k) for d in range(ndim)]
    res['host_subset_squares_last_lag_max'] = int(max(last))
    res['host_subset_squares_last_lag_by_parameter'] = [int(max(last[d::ndim])) for d in range(ndim)]
    if E > 1:               # (a subset of a lone ensemble's walkers has another ESS)
        assert np.allclose(c.out[:k].cpu().numpy(), got['mean'], rtol=1e-9, atol=0), 'device ESS differs from the definition'
        assert np.allclose(c.bulk[:k], got['bulk'], rtol=1e-9, atol=0) and np.allclose(c.tail[:k], got['tail'], rtol=1e-9, atol=0)
    return res


def run(name, reps, host_subset):
    import torch
    from bisip_amd import ess as es
    E, Wp, ndim, n = SHAPES[name]
    x = make_ar1_chain(E, Wp, ndim, n)
    c = Calls(x, E, Wp, ndim)
    chain_bytes = 8 * n * E * Wp * ndim
    Lr = es.round_lags(n, E, Wp, ndim)
    res = dict(shape=name, E=E, Wp=Wp, ndim=ndim, samples=n, chain_bytes=chain_bytes, reps=reps, rho=[0.0, 0.95],
               ess_workspace_bytes=c.ess_bytes, rank_workspace_bytes=c.rank_bytes, lags_per_round=Lr,
               rounds_enqueued=-(-(n // 2) // Lr))
    for what, (med, best, spread) in time_alternating(c, reps).items():
        res[what + '_ms'], res[what + '_ms_best'], res[what + '_ms_spread'] = med, best, spread
    res['rank_folded_over_rank'] = res['rank_folded_ms'] / res['rank_ms']
    res['ess_squares_over_ess_mean'] = res['ess_squares_ms'] / res['ess_mean_ms']
    res['central_moments_over_moments'] = res['central_moments_ms'] / res['moments_ms']
    res['summary_saves_ms'] = res['separate_ms'] - res['summary_ms']
    res['ess_mean_over_autocorr'] = res['ess_mean_ms'] / res['autocorr_ms']
    res['rank_over_sort'] = res['rank_ms'] / res['sort_ms']
    res['ess_mean_over_moments'] = res['ess_mean_ms'] / res['moments_ms']
    res['ess_min'] = [float(np.nanmin(v)) for v in (c.out.cpu().numpy(), c.bulk, c.tail)]
    res.update(host_path(c, host_subset))
    for kind in es.KINDS:
        res[f'ess_{kind}_speedup_vs_host_extrapolated'] = res[f'host_ess_{kind}_extrapolated_s'] * 1e3 / res[f'ess_{kind}_ms']
    del x, c
    torch.cuda.empty_cache()
    return res


def kernel_times(name, reps, outdir):
    """Per-call time of every kernel from a separate rocprofv3 run of the calls alone."""
    import csv
    d = os.path.join(outdir, f'rocprof_{name}')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', name, '--',
           sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(reps)]
    try:
        rc = subprocess.run(cmd, timeout=600, capture_output=True, text=True).returncode
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(profile_error=str(e))
    if rc != 0:
        return dict(profile_error=f'rocprofv3 exit {rc}')
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        return dict(profile_error='no kernel_stats.csv')
    per = {}
    for row in csv.DictReader(open(files[0])):
        for key in ('k_ess_prep', 'k_ess_lags', 'k_ess_chain_sums', 'k_ess_scan', 'k_rank_z', 'k_gather_columns',
                    'k_ac_lags', 'k_fold_columns', 'k_central_partial', 'k_moments_partial'):
            if key in row['Name']:
                per[key] = per.get(key, 0.0) + float(row['TotalDurationNs']) / int(row['Calls']) / 1e6
    return dict(kernel_ms_per_launch=per)


SUMMARY_GROUPS = (('rank passes', ('k_rank_z', 'k_fold_columns', 'k_gather_columns', 'rocprim', 'k_order_zeros')),
                  ('ESS rounds', ('k_ess_',)), ('HDI', ('k_hdi',)), ('R-hat', ('k_rhat',)),
                  ('moments', ('k_moments', 'k_central')), ('selection', ('k_segmented_select', 'k_percentile_lerp')))


def summary_split(name, outdir):
    """How one device_summary splits over its kernels: a separate rocprofv3 run of a warmed-up single call."""
    import csv
    d = os.path.join(outdir, f'rocprof_summary_{name}')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', name, '--',
           sys.executable, os.path.abspath(__file__), '--child-summary', name]
    try:
        rc = subprocess.run(cmd, timeout=600, capture_output=True, text=True).returncode
    except (OSError, subprocess.TimeoutExpired) as e:
        return dict(summary_profile_error=str(e))
    if rc != 0:
        return dict(summary_profile_error=f'rocprofv3 exit {rc}')
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        return dict(summary_profile_error='no kernel_stats.csv')
    split = {g: 0.0 for g, _ in SUMMARY_GROUPS}
    split['the rest'] = 0.0
    for row in csv.DictReader(open(files[0])):
        ms = float(row['TotalDurationNs']) / 1e6 / 2          # (the child makes two calls: warm-up and one more)
        for g, keys in SUMMARY_GROUPS:
            if any(k in row['Name'] for k in keys):
                split[g] += ms
                break
        else:
            if 'make_ar1' not in row['Name'] and 'at::native' not in row['Name']:       # (not the chain's generation)
                split['the rest'] += ms
    return dict(summary_split_ms=split)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles the host path times')
    ap.add_argument('--profile', action='store_true', help='also a rocprofv3 kernel trace of every shape')
    ap.add_argument('--out', help='directory for the JSON lines and the kernel-trace CSVs (default: stdout only)')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    ap.add_argument('--child-summary', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('ess_bench needs a GPU')
    if args.child:                   # under rocprofv3: the calls only
        E, Wp, ndim, n = SHAPES[args.child]
        c = Calls(make_ar1_chain(E, Wp, ndim, n), E, Wp, ndim)
        for _ in range(args.reps):
            c.ess_mean(); c.rank(); c.autocorr(); c.rank_folded(); c.ess_squares(); c.central_moments()
        torch.cuda.synchronize()
        return
    if args.child_summary:           # under rocprofv3: device_summary twice
        from bisip_amd import diagnostics
        from bisip_amd.chainview import ChainView
        E, Wp, ndim, n = SHAPES[args.child_summary]
        view = ChainView(make_ar1_chain(E, Wp, ndim, n), n, E, Wp, ndim)
        for _ in range(2):
            diagnostics.device_summary(view)
        torch.cuda.synchronize()
        return
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory(prefix='ess_bench_') as tmp:
        outdir = args.out or tmp
        os.makedirs(outdir, exist_ok=True)
        for name in args.shapes.split(','):
            r = run(name, args.reps, args.host_subset)
            if args.profile:
                r.update(kernel_times(name, args.reps, outdir))
                r.update(summary_split(name, outdir))
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(os.path.join(args.out, 'ess_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
