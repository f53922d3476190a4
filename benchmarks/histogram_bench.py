#!/usr/bin/env python3
"""Posterior histograms of device-resident chains (bisip_chain_range_dev, bisip_chain_histograms_dev,
bisip_chain_pair_histograms_dev).

Four shapes: the cfg5 slice (512 spectra x 256 walkers x 7, 1000 stored, discard 500), one ensemble of 32 walkers x
5000 samples x 7, one ensemble of 131,072 walkers x 200 x 7, and a batch of 128 spectra x 256 walkers x 500 x 12
(polynomial degree 10: 66 pairs in two groups).  Each shape runs on two chains made on the device:
  * 'spread': uniform in the prior box, range=None (edges from the chain's own min and max): the counters are spread;
  * 'narrow': a Gaussian of 1 % of the box around a centre per ensemble, range='bounds': every value of a parameter
    falls in one or two bins, the counters are contended.
Per shape and chain, device events around each call after warm-up (outputs allocated once, edges uploaded once):
  * range_ms, hist_ms (25 bins), pair_ms (20 bins), and moments_ms: bisip_chain_moments_dev on the same chain in the
    same run -- existing code that reads the chain twice without atomics, the yardstick;
  * the chain's bytes n * E * Wp * ndim * 8 over each time, and that as a fraction of the 8 TB/s HBM peak;
  * the host path: np.histogram / np.histogram2d on a copy of the used samples of a subset (8 ensembles, or 1/16 of
    the walkers of a lone ensemble), extrapolated linearly (labelled as such; the device-to-host copy is timed apart).
With --profile a separate `rocprofv3 --kernel-trace --stats` run of the calls alone gives the time per kernel.
Prints one JSON line per (shape, chain); with --out DIR also writes them (and the traces) there."""
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

SHAPES = {   # name: (E, Wp, ndim, stored, discard)
    'cfg5_slice': (512, 256, 7, 1000, 500),
    'lone_32x5000': (1, 32, 7, 5000, 0),
    'big_131072x200': (1, 131072, 7, 200, 0),
    'deg10_batch': (128, 256, 12, 500, 0),
}
CHAINS = ('spread', 'narrow')
HBM_PEAK = 8.0e12          # bytes/s, MI355X spec
BINS_1D, BINS_2D = 25, 20


def box(ndim):
    """The prior box of the polynomial decomposition: r0 in [0.9, 1.1], coefficients in [-1, 1]."""
    lo = np.full(ndim, -1.0)
    hi = np.full(ndim, 1.0)
    lo[0], hi[0] = 0.9, 1.1
    return np.stack([lo, hi])


def make_chain(kind, E, Wp, ndim, stored, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    b = torch.from_numpy(box(ndim)).cuda()
    lo, width = b[0], b[1] - b[0]
    x = torch.empty((stored, E * Wp, ndim), dtype=torch.float64, device='cuda')
    centre = lo + width * (0.2 + 0.6 * torch.rand((E, 1, ndim), generator=g, dtype=torch.float64, device='cuda'))
    step = max(1, min(stored, (1 << 26) // (E * Wp * ndim)))
    for s0 in range(0, stored, step):
        k = min(step, stored - s0)
        if kind == 'spread':
            u = torch.rand((k, E * Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
            x[s0:s0 + k] = lo + width * u
        else:
            z = torch.randn((k, E, Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
            x[s0:s0 + k] = (centre + 0.01 * width * z).reshape(k, E * Wp, ndim)
    return x


class Calls:
    """The four calls on one chain, outputs and workspace allocated once."""

    def __init__(self, x, kind, E, Wp, ndim, discard):
        import torch
        from bisip_amd import _hip
        from bisip_amd import histogram as hg
        self.hip, self.E, self.Wp, self.ndim = _hip, E, Wp, ndim
        W = E * Wp
        self.n = int(x.shape[0]) - discard
        self.ptr, self.stride = x.data_ptr() + 8 * discard * W * ndim, W * ndim
        self.st = torch.cuda.current_stream().cuda_stream
        dev = x.device
        self.minmax = torch.empty((E, ndim, 2), dtype=torch.float64, device=dev)
        self.bad = torch.empty((E, ndim), dtype=torch.int64, device=dev)
        self.range()
        torch.cuda.synchronize()
        if kind == 'spread':        # range=None
            r = hg.resolve_range(None, E, ndim, data_range=lambda: (self.minmax.cpu().numpy(), self.bad.cpu().numpy()))
        else:
            r = hg.resolve_range('bounds', E, ndim, box(ndim))
        self.ranges = r
        self.e1 = torch.from_numpy(np.ascontiguousarray(hg.edges_from_range(r, BINS_1D))).to(dev)
        self.e2 = torch.from_numpy(np.ascontiguousarray(hg.edges_from_range(r, BINS_2D))).to(dev)
        self.c1 = torch.empty((E, ndim, BINS_1D), dtype=torch.int64, device=dev)
        self.c2 = torch.empty((E, ndim * (ndim - 1) // 2, BINS_2D, BINS_2D), dtype=torch.int64, device=dev)
        self.mean = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.std = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.work = torch.empty((max(1, _hip.chain_moments_workspace(self.n, E, ndim)),), dtype=torch.float64, device=dev)

    def range(self):
        self.hip.chain_range_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.minmax.data_ptr(),
                                 self.bad.data_ptr(), self.st)

    def hist(self):
        self.hip.chain_histograms_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.e1.data_ptr(),
                                      BINS_1D, self.c1.data_ptr(), self.st)

    def pair(self):
        self.hip.chain_pair_histograms_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim,
                                           self.e2.data_ptr(), BINS_2D, self.c2.data_ptr(), self.st)

    def moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                                   self.std.data_ptr(), self.work.data_ptr(), self.st)


def time_call(f, reps):
    import torch
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.min(times)), float(np.median(times))


def host_path(x, c, discard, host_subset):
    """np.histogram / np.histogram2d on a host copy of a subset of the used samples, extrapolated by its share."""
    E, Wp, ndim = c.E, c.Wp, c.ndim
    if E > 1:
        k = min(E, host_subset)
        rows, scale = slice(0, k * Wp), E / k
    else:
        k = 1
        w = max(32, Wp // 16)
        rows, scale = slice(0, min(Wp, w)), Wp / min(Wp, w)
    t0 = time.perf_counter()
    sub = x[discard:, rows].cpu().numpy()
    copy_s = time.perf_counter() - t0
    per = sub.shape[1] // k
    jj, kk = np.triu_indices(ndim, 1)
    t0 = time.perf_counter()
    for e in range(k):
        flat = sub[:, e * per:(e + 1) * per].reshape(-1, ndim)
        r = c.ranges[e]
        for q in range(ndim):
            np.histogram(flat[:, q], BINS_1D, tuple(r[q]))
    t1 = time.perf_counter()
    for e in range(k):
        flat = sub[:, e * per:(e + 1) * per].reshape(-1, ndim)
        r = c.ranges[e]
        for j, l in zip(jj, kk):
            np.histogram2d(flat[:, j], flat[:, l], BINS_2D, [tuple(r[j]), tuple(r[l])])
    t2 = time.perf_counter()
    return dict(host_subset_values=int(sub.size), host_copy_subset_s=copy_s, host_hist_subset_s=t1 - t0,
                host_pair_subset_s=t2 - t1, host_hist_extrapolated_s=(t1 - t0) * scale,
                host_pair_extrapolated_s=(t2 - t1) * scale, host_copy_extrapolated_s=copy_s * scale,
                host_note='extrapolated linearly from the subset, not measured on the whole chain')


def run(name, kind, reps, host_subset):
    import torch
    E, Wp, ndim, stored, discard = SHAPES[name]
    x = make_chain(kind, E, Wp, ndim, stored)
    c = Calls(x, kind, E, Wp, ndim, discard)
    chain_bytes = 8 * c.n * E * Wp * ndim
    res = dict(shape=name, chain=kind, range='None' if kind == 'spread' else 'bounds', E=E, Wp=Wp, ndim=ndim,
               samples=c.n, bins_1d=BINS_1D, bins_2d=BINS_2D, chain_bytes=chain_bytes, reps=reps)
    for what in ('moments', 'range', 'hist', 'pair', 'moments'):       # (the yardstick before and after: best of both)
        best, med = time_call(getattr(c, what), reps)
        if what + '_ms' in res:
            best, med = min(best, res[what + '_ms']), min(med, res[what + '_ms_median'])
        res[what + '_ms'], res[what + '_ms_median'] = best, med
    for what in ('moments', 'range', 'hist', 'pair'):
        rate = chain_bytes / (res[what + '_ms'] * 1e-3)
        res[what + '_chain_TBps'] = rate / 1e12
        res[what + '_frac_of_hbm_peak'] = rate / HBM_PEAK
    res['hist_over_moments'] = res['hist_ms'] / res['moments_ms']
    res['pair_over_moments'] = res['pair_ms'] / res['moments_ms']
    counts = c.c1.cpu().numpy()
    res['hist_total'] = int(counts.sum())
    res['fullest_bin_share'] = float((counts.max(axis=2) / np.maximum(1, counts.sum(axis=2))).mean())
    res['pair_total'] = int(c.c2.sum().item())
    # both chains lie inside their edges: every value and every row is counted
    assert res['hist_total'] == c.n * E * Wp * ndim, (res['hist_total'], c.n * E * Wp * ndim)
    assert res['pair_total'] == c.n * E * Wp * (ndim * (ndim - 1) // 2), res['pair_total']
    res.update(host_path(x, c, discard, host_subset))
    res['hist_speedup_vs_host_extrapolated'] = res['host_hist_extrapolated_s'] * 1e3 / res['hist_ms']
    res['pair_speedup_vs_host_extrapolated'] = res['host_pair_extrapolated_s'] * 1e3 / res['pair_ms']
    del x, c
    torch.cuda.empty_cache()
    return res


def kernel_times(name, kind, reps, outdir):
    """Per-call time of every kernel from a separate rocprofv3 run of the calls alone."""
    import csv
    d = os.path.join(outdir, f'rocprof_{name}_{kind}')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', f'{name}_{kind}', '--',
           sys.executable, os.path.abspath(__file__), '--child', f'{name}:{kind}', '--reps', str(reps)]
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
        for key in ('k_chain_range', 'k_chain_histograms', 'k_pair_histograms', 'k_moments_partial'):
            if key in row['Name'] and 'init' not in row['Name'] and 'finish' not in row['Name']:
                # (one row per instantiation: the two passes of the moments add up)
                per[key] = per.get(key, 0.0) + float(row['TotalDurationNs']) / int(row['Calls']) / 1e6
    return dict(kernel_ms=per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--chains', default=','.join(CHAINS))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles the host path times')
    ap.add_argument('--profile', action='store_true', help='also a rocprofv3 kernel trace of every (shape, chain)')
    ap.add_argument('--out', help='directory for the JSON lines and the kernel-trace CSVs (default: stdout only)')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('histogram_bench needs a GPU')
    if args.child:                   # under rocprofv3: the calls only
        name, kind = args.child.split(':')
        E, Wp, ndim, stored, discard = SHAPES[name]
        c = Calls(make_chain(kind, E, Wp, ndim, stored), kind, E, Wp, ndim, discard)
        for _ in range(args.reps):
            c.range(); c.hist(); c.pair(); c.moments()
        torch.cuda.synchronize()
        return
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory(prefix='histogram_bench_') as tmp:
        outdir = args.out or tmp
        os.makedirs(outdir, exist_ok=True)
        for name in args.shapes.split(','):
            for kind in args.chains.split(','):
                r = run(name, kind, args.reps, args.host_subset)
                if args.profile:
                    r.update(kernel_times(name, kind, args.reps, outdir))
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if args.out:
        with open(os.path.join(args.out, 'histogram_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
