#!/usr/bin/env python3
"""Per-walker moments and split R-hat of device-resident chains (bisip_chain_rhat_dev).

The three shapes of trace_bench.py: the survey (512 spectra x 256 walkers x 500 samples x 7), the quickstart (one
ensemble of 32 walkers x 5000 x 7: cut into segments) and cfg4 (one ensemble of 32,768 walkers x 200 x 7).  The chain is
a Gaussian around a centre per ensemble, made on the device.  Per shape, device events around each call after warm-up
(outputs and workspace allocated once), best of --reps:
  * rhat_ms: R-hat alone (splits = 2); rhat_moments_ms: with the mean and variance of every chain stored;
  * the chain's bytes n * E * Wp * ndim * 8 over that time, and that as a fraction of the 8 TB/s HBM peak;
  * moments_ms: bisip_chain_moments_dev on the same chain in the same run (reads the chain twice), the yardstick;
  * the host path: bisip_amd.convergence.rhat (NumPy) on a host copy of a subset (8 ensembles, or 1/16 of the walkers of
    a lone ensemble), extrapolated linearly (labelled as such; the device-to-host copy is timed apart).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_bench import HBM_PEAK, SHAPES, make_chain, time_call      # noqa: E402


class Calls:
    """The calls on one chain, outputs and workspaces allocated once."""

    def __init__(self, x, E, Wp, ndim):
        import torch
        from bisip_amd import _hip
        self.hip, self.x, self.E, self.Wp, self.ndim = _hip, x, E, Wp, ndim
        self.n = n = int(x.shape[0])
        self.ptr, self.stride = x.data_ptr(), E * Wp * ndim
        self.st = torch.cuda.current_stream().cuda_stream
        dev = x.device
        self.rh = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.cmean = torch.empty((2, E, Wp, ndim), dtype=torch.float64, device=dev)
        self.cvar = torch.empty((2, E, Wp, ndim), dtype=torch.float64, device=dev)
        self.nbytes = _hip.chain_rhat_workspace(n, E, Wp, ndim, 2)
        self.work = torch.empty((max(1, self.nbytes),), dtype=torch.uint8, device=dev)
        self.mean = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.std = torch.empty((E, ndim), dtype=torch.float64, device=dev)
        self.mwork = torch.empty((max(1, _hip.chain_moments_workspace(n, E, ndim)),), dtype=torch.float64, device=dev)

    def rhat(self):
        self.hip.chain_rhat_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, 2, 0, 0, self.rh.data_ptr(),
                                self.work.data_ptr(), self.nbytes, self.st)

    def rhat_moments(self):
        self.hip.chain_rhat_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, 2, self.cmean.data_ptr(),
                                self.cvar.data_ptr(), self.rh.data_ptr(), self.work.data_ptr(), self.nbytes, self.st)

    def moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                                   self.std.data_ptr(), self.mwork.data_ptr(), self.st)


def host_path(c, host_subset):
    """convergence.rhat and walker_moments in NumPy on a host copy of a subset of the chain, extrapolated by its share."""
    from bisip_amd import convergence as cv
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
    t0 = time.perf_counter()
    r = np.stack([cv.rhat(sub[:, e * wk:(e + 1) * wk]) for e in range(k)])
    cv.walker_moments(sub)
    host_s = time.perf_counter() - t0
    if E > 1:               # (a subset of a lone ensemble's walkers has another R-hat)
        assert np.allclose(c.rh[:k].cpu().numpy(), r, rtol=1e-9, atol=0), 'device R-hat differs from the definition'
    return dict(host_subset_values=int(sub.size), host_copy_subset_s=copy_s, host_rhat_subset_s=host_s,
                host_rhat_extrapolated_s=host_s * scale, host_copy_extrapolated_s=copy_s * scale,
                host_note='extrapolated linearly from the subset, not measured on the whole chain')


def run(name, reps, host_subset):
    import torch
    from bisip_amd import convergence as cv
    E, Wp, ndim, n = SHAPES[name]
    x = make_chain(E, Wp, ndim, n)
    c = Calls(x, E, Wp, ndim)
    chain_bytes = 8 * n * E * Wp * ndim
    seg_len, nseg = cv.segment_plan(n // 2, E * Wp * ndim, 2)
    res = dict(shape=name, E=E, Wp=Wp, ndim=ndim, samples=n, chain_bytes=chain_bytes, reps=reps,
               workspace_bytes=c.nbytes, segments_per_half=nseg, segment_samples=seg_len,
               path='one kernel' if c.nbytes == 0 else 'accumulate + ' + ('merge + ' if nseg > 1 else '') + 'stage')
    for what in ('moments', 'rhat', 'rhat_moments', 'moments'):        # (the yardstick before and after: best of both)
        best, med = time_call(getattr(c, what), reps)
        if what + '_ms' in res:
            best, med = min(best, res[what + '_ms']), min(med, res[what + '_ms_median'])
        res[what + '_ms'], res[what + '_ms_median'] = best, med
    for what in ('moments', 'rhat', 'rhat_moments'):
        rate = chain_bytes / (res[what + '_ms'] * 1e-3)
        res[what + '_chain_TBps'] = rate / 1e12
        res[what + '_frac_of_hbm_peak'] = rate / HBM_PEAK
    res['rhat_over_moments'] = res['rhat_ms'] / res['moments_ms']
    res.update(host_path(c, host_subset))
    res['rhat_speedup_vs_host_extrapolated'] = res['host_rhat_extrapolated_s'] * 1e3 / res['rhat_ms']
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
        for key in ('k_rhat_fused', 'k_rhat_accumulate', 'k_rhat_merge', 'k_rhat_stage', 'k_moments_partial'):
            if key in row['Name']:
                per[key] = per.get(key, 0.0) + float(row['TotalDurationNs']) / int(row['Calls']) / 1e6
    return dict(kernel_ms=per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles the host path times')
    ap.add_argument('--profile', action='store_true', help='also a rocprofv3 kernel trace of every shape')
    ap.add_argument('--out', help='directory for the JSON lines and the kernel-trace CSVs (default: stdout only)')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('convergence_bench needs a GPU')
    if args.child:                   # under rocprofv3: the calls only
        E, Wp, ndim, n = SHAPES[args.child]
        c = Calls(make_chain(E, Wp, ndim, n), E, Wp, ndim)
        for _ in range(args.reps):
            c.rhat(); c.rhat_moments(); c.moments()
        torch.cuda.synchronize()
        return
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory(prefix='convergence_bench_') as tmp:
        outdir = args.out or tmp
        os.makedirs(outdir, exist_ok=True)
        for name in args.shapes.split(','):
            r = run(name, args.reps, args.host_subset)
            if args.profile:
                r.update(kernel_times(name, args.reps, outdir))
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(os.path.join(args.out, 'convergence_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
