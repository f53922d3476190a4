#!/usr/bin/env python3
"""Per-step walker statistics of device-resident chains (bisip_chain_trace_dev).

Three shapes: the survey (512 spectra x 256 walkers x 500 samples x 7), the quickstart (one ensemble of 32 walkers x
5000 x 7) and cfg4 (one ensemble of 32,768 walkers x 200 x 7: beyond the LDS kernel, the gather + select path).  The
chain is a Gaussian around a centre per ensemble, made on the device.  Per shape, device events around each call after
warm-up (outputs and workspace allocated once), p = [2.5, 50, 97.5] and the mean:
  * trace_ms: bisip_chain_trace_dev; trace_mean_only_ms: the same without percentiles;
  * the chain's bytes n * E * Wp * ndim * 8 over that time, and that as a fraction of the 8 TB/s HBM peak;
  * moments_ms: bisip_chain_moments_dev on the same chain in the same run (reads the chain twice), the yardstick;
  * composed_ms: what the entry points before this one could do -- a contiguous copy of the used samples, then
    bisip_grouped_percentiles_dev with one group per (sample, ensemble), in slabs whose workspace fits --workspace-gib
    (percentiles only: it has no mean);
  * the host path: np.percentile / np.mean over the walker axis of a host copy of a subset (8 ensembles, or 1/16 of the
    samples of a lone ensemble), extrapolated linearly (labelled as such; the device-to-host copy is timed apart).
With --profile a separate `rocprofv3 --kernel-trace --stats` run of the calls alone gives the time per kernel.
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

SHAPES = {   # name: (E, Wp, ndim, samples)
    'survey_512x256x500': (512, 256, 7, 500),
    'quickstart_32x5000': (1, 32, 7, 5000),
    'cfg4_32768x200': (1, 32768, 7, 200),
}
P = [2.5, 50.0, 97.5]
HBM_PEAK = 8.0e12          # bytes/s, MI355X spec


def make_chain(E, Wp, ndim, n, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.empty((n, E * Wp, ndim), dtype=torch.float64, device='cuda')
    centre = torch.rand((E, 1, ndim), generator=g, dtype=torch.float64, device='cuda')
    step = max(1, min(n, (1 << 26) // (E * Wp * ndim)))
    for s0 in range(0, n, step):
        k = min(step, n - s0)
        z = torch.randn((k, E, Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
        x[s0:s0 + k] = (centre + 0.01 * z).reshape(k, E * Wp, ndim)
    return x


class Calls:
    """The calls on one chain, outputs and workspaces allocated once."""

    def __init__(self, x, E, Wp, ndim, workspace_gib):
        import torch
        from bisip_amd import _hip
        self.hip, self.x, self.E, self.Wp, self.ndim = _hip, x, E, Wp, ndim
        self.n = n = int(x.shape[0])
        self.ptr, self.stride = x.data_ptr(), E * Wp * ndim
        self.st = torch.cuda.current_stream().cuda_stream
        dev = x.device
        self.pct = torch.empty((len(P), n, E, ndim), dtype=torch.float64, device=dev)
        self.avg = torch.empty((n, E, ndim), dtype=torch.float64, device=dev)
        self.trace_bytes = _hip.chain_trace_workspace(n, E, Wp, ndim, len(P))
        self.trace_work = torch.empty((max(1, self.trace_bytes),), dtype=torch.uint8, device=dev)
        self.mean = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.std = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.mwork = torch.empty((max(1, _hip.chain_moments_workspace(n, E, ndim)),), dtype=torch.float64, device=dev)
        # the composition: groups = (sample, ensemble); as many samples per slab as the workspace budget and the 2^31
        # values of one call allow
        budget = int(workspace_gib * (1 << 30))
        s = n
        while s > 1 and not 0 < _hip.grouped_percentiles_workspace(s * E, Wp, ndim, len(P)) <= budget:
            s = (s + 1) // 2
        self.slab = s
        self.gbytes = _hip.grouped_percentiles_workspace(s * E, Wp, ndim, len(P))
        if self.gbytes <= 0:
            raise SystemExit('one sample does not fit one grouped_percentiles call')
        self.gwork = torch.empty((self.gbytes,), dtype=torch.uint8, device=dev)
        self.copy = torch.empty((s, E * Wp, ndim), dtype=torch.float64, device=dev)
        self.gout = torch.empty((len(P), s * E, ndim), dtype=torch.float64, device=dev)
        self.composed_pct = torch.empty((len(P), n, E, ndim), dtype=torch.float64, device=dev)

    def trace(self):
        self.hip.chain_trace_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, P, self.pct.data_ptr(),
                                 self.avg.data_ptr(), self.trace_work.data_ptr(), self.trace_bytes, self.st)

    def trace_mean_only(self):
        self.hip.chain_trace_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, None, 0, self.avg.data_ptr(),
                                 self.trace_work.data_ptr(), self.trace_bytes, self.st)

    def moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                                   self.std.data_ptr(), self.mwork.data_ptr(), self.st)

    def composed(self):
        for s0 in range(0, self.n, self.slab):
            k = min(self.slab, self.n - s0)
            self.copy[:k].copy_(self.x[s0:s0 + k])
            self.hip.grouped_percentiles_dev(self.copy.data_ptr(), k * self.E, self.Wp, self.ndim, P, self.gout.data_ptr(),
                                             self.gwork.data_ptr(), self.gbytes, self.st)
            # (k groups of a short last slab lie at the front of gout's (len(P), k * E, ndim) layout)
            got = self.gout.reshape(-1)[:len(P) * k * self.E * self.ndim].reshape(len(P), k, self.E, self.ndim)
            self.composed_pct[:, s0:s0 + k].copy_(got)


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


def host_path(c, host_subset):
    """np.percentile / np.mean over the walkers on a host copy of a subset of the chain, extrapolated by its share."""
    E, Wp, ndim, n = c.E, c.Wp, c.ndim, c.n
    if E > 1:
        k = min(E, host_subset)
        part, scale = c.x[:, :k * Wp], E / k
    else:
        k, m = 1, max(1, n // 16)
        part, scale = c.x[:m], n / m
    t0 = time.perf_counter()
    sub = part.cpu().numpy().reshape(part.shape[0], k, Wp, ndim)
    copy_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    pct = np.percentile(sub, P, axis=2)
    mean = np.mean(sub, axis=2)
    host_s = time.perf_counter() - t0
    got = c.pct[:, :sub.shape[0], :k].cpu().numpy()
    assert np.array_equal(got, pct), 'device percentiles differ from np.percentile'
    assert np.allclose(c.avg[:sub.shape[0], :k].cpu().numpy(), mean, rtol=1e-13, atol=0)
    return dict(host_subset_values=int(sub.size), host_copy_subset_s=copy_s, host_trace_subset_s=host_s,
                host_trace_extrapolated_s=host_s * scale, host_copy_extrapolated_s=copy_s * scale,
                host_note='extrapolated linearly from the subset, not measured on the whole chain')


def run(name, reps, host_subset, workspace_gib):
    import torch
    E, Wp, ndim, n = SHAPES[name]
    x = make_chain(E, Wp, ndim, n)
    c = Calls(x, E, Wp, ndim, workspace_gib)
    chain_bytes = 8 * n * E * Wp * ndim
    res = dict(shape=name, E=E, Wp=Wp, ndim=ndim, samples=n, percentiles=P, chain_bytes=chain_bytes, reps=reps,
               lds_walkers=c.hip.chain_trace_lds_walkers(ndim), path='lds' if c.trace_bytes == 0 else 'gather+select',
               trace_workspace_bytes=c.trace_bytes, composed_slab_samples=c.slab, composed_workspace_bytes=c.gbytes)
    for what in ('moments', 'trace', 'trace_mean_only', 'moments'):        # (the yardstick before and after: best of both)
        best, med = time_call(getattr(c, what), reps)
        if what + '_ms' in res:
            best, med = min(best, res[what + '_ms']), min(med, res[what + '_ms_median'])
        res[what + '_ms'], res[what + '_ms_median'] = best, med
    res['composed_ms'], res['composed_ms_median'] = time_call(c.composed, max(2, reps // 3))
    for what in ('moments', 'trace', 'trace_mean_only', 'composed'):
        rate = chain_bytes / (res[what + '_ms'] * 1e-3)
        res[what + '_chain_TBps'] = rate / 1e12
        res[what + '_frac_of_hbm_peak'] = rate / HBM_PEAK
    res['trace_over_moments'] = res['trace_ms'] / res['moments_ms']
    res['composed_over_trace'] = res['composed_ms'] / res['trace_ms']
    res['composed_equals_trace'] = bool(torch.equal(c.composed_pct, c.pct))
    res.update(host_path(c, host_subset))
    res['trace_speedup_vs_host_extrapolated'] = res['host_trace_extrapolated_s'] * 1e3 / res['trace_ms']
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
        for key in ('k_chain_trace_lds', 'k_trace_column_mean', 'k_gather_columns_tiled', 'k_segmented_select',
                    'k_moments_partial'):
            if key in row['Name']:
                per[key] = per.get(key, 0.0) + float(row['TotalDurationNs']) / int(row['Calls']) / 1e6
    return dict(kernel_ms=per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles the host path times')
    ap.add_argument('--workspace-gib', type=float, default=8.0, help='workspace budget of the composed path')
    ap.add_argument('--profile', action='store_true', help='also a rocprofv3 kernel trace of every shape')
    ap.add_argument('--out', help='directory for the JSON lines and the kernel-trace CSVs (default: stdout only)')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('trace_bench needs a GPU')
    if args.child:                   # under rocprofv3: the calls only
        E, Wp, ndim, n = SHAPES[args.child]
        c = Calls(make_chain(E, Wp, ndim, n), E, Wp, ndim, args.workspace_gib)
        for _ in range(args.reps):
            c.trace(); c.moments()
        torch.cuda.synchronize()
        return
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory(prefix='trace_bench_') as tmp:
        outdir = args.out or tmp
        os.makedirs(outdir, exist_ok=True)
        for name in args.shapes.split(','):
            r = run(name, args.reps, args.host_subset, args.workspace_gib)
            if args.profile:
                r.update(kernel_times(name, args.reps, outdir))
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(os.path.join(args.out, 'trace_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
