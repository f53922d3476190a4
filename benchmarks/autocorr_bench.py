#!/usr/bin/env python3
"""Integrated autocorrelation time of device-resident chains (bisip_chain_autocorr_time_dev).

Three shapes: the cfg5 slice (512 spectra x 256 walkers x 7, 1000 stored, discard 500), one ensemble of
32 walkers x 5000 samples x 7, and one ensemble of 131,072 walkers x 200 x 7.  The chains are AR(1) series
generated on the device, rho of every (ensemble, parameter) drawn from [0.5, 0.95] (tau 3 ... 39, the range
of a stretch-move run's parameters).  Per shape:
  * call_ms: device events around a synchronised call (workspace allocated once), after warm-up;
  * kernel_ms: the library's kernels per call from a separate `rocprofv3 --kernel-trace --stats` run;
  * the FMAs the rounds evaluated (from the returned windows and the round size) over kernel time, as a
    fraction of the measured fp64 FMA ceiling (bisip_fp64_stream_probe_dev), and the chain's bytes over
    the HBM peak -- and which of the two bounds the call;
  * the host path (emcee's algorithm, bisip_amd.autocorr.integrated_time on a copy of the chain) timed on
    a subset of ensembles / walkers and extrapolated by the number of series (labelled as such).
Prints one JSON line per shape; with --out DIR also writes them and the rocprofv3 CSVs there."""
import argparse
import glob
import json
import os
import re
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
}
HBM_PEAK = 8.0e12          # bytes/s, MI355X spec
TILE, LAG_BLOCK, T_STAGE, TARGET_BLOCKS = 64, 64, 32, 512    # bisip_amd/csrc/chain_lags.h


def make_chain(E, Wp, ndim, n, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    rho = 0.5 + 0.45 * torch.rand((E, 1, ndim), generator=g, dtype=torch.float64, device='cuda')
    rho = rho.expand(E, Wp, ndim).reshape(E * Wp, ndim)
    x = torch.empty((n, E * Wp, ndim), dtype=torch.float64, device='cuda')
    x[0] = torch.randn((E * Wp, ndim), generator=g, dtype=torch.float64, device='cuda') / torch.sqrt(1 - rho * rho)
    for s in range(1, n):
        x[s] = rho * x[s - 1] + torch.randn((E * Wp, ndim), generator=g, dtype=torch.float64, device='cuda')
    return x


def round_lags(n_t, M):
    tiles = -(-M // TILE)
    nb = max(1, min(-(-TARGET_BLOCKS // tiles), -(-n_t // LAG_BLOCK), 65535))
    return nb * LAG_BLOCK


def evaluated_fmas(win, n_t, E, Wp, ndim):
    """FMAs the lag kernel issues: per tile of 64 series, every round up to the last one any of its
    (ensemble, parameter) pairs needs; per lag workgroup 64 series x 64 lags x the staged samples."""
    M = E * Wp * ndim
    L = round_lags(n_t, M)
    need = win.reshape(E, 1, ndim).repeat(Wp, axis=1).reshape(-1)      # window of every series
    tiles = -(-M // TILE)
    pad = np.full(tiles * TILE, -1, dtype=np.int64)
    pad[:M] = need
    last_round = pad.reshape(tiles, TILE).max(axis=1) // L             # rounds 0 ... last_round run
    per_round = []                                                     # FMAs of one tile in round r
    for k0 in range(0, n_t, L):
        f = 0
        for kb in range(k0, min(k0 + L, n_t), LAG_BLOCK):
            f += TILE * LAG_BLOCK * (-(-(n_t - kb) // T_STAGE)) * T_STAGE
        per_round.append(f)
    cum = np.cumsum(per_round)
    return int(cum[np.minimum(last_round, len(cum) - 1)].sum()), L


def fp64_ceiling():
    """Independent fp64 FMAs per second (bisip_fp64_stream_probe_dev), best of five after a warm-up."""
    import torch
    from bisip_amd import _hip
    out = torch.empty(_hip.fp64_stream_probe_lanes(), dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream()
    _hip.fp64_stream_probe_dev(out.data_ptr(), 4096, st.cuda_stream)
    best = 0.0
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        n = _hip.fp64_stream_probe_dev(out.data_ptr(), 4096, st.cuda_stream)
        b.record()
        b.synchronize()
        best = max(best, n * 64 / (a.elapsed_time(b) * 1e-3))
    return best


def run_shape(name, reps, host_subset):
    import torch
    from bisip_amd import _hip
    from bisip_amd.autocorr import integrated_time
    E, Wp, ndim, stored, discard = SHAPES[name]
    W, n = E * Wp, stored - discard
    x = make_chain(E, Wp, ndim, stored)
    nbytes = _hip.chain_autocorr_time_workspace(n, E, Wp, ndim)
    work = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    tau = torch.empty((E, ndim), dtype=torch.float64, device='cuda')
    win = torch.empty((E, ndim), dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream()

    def call():
        _hip.chain_autocorr_time_dev(x.data_ptr() + 8 * discard * W * ndim, n, W * ndim, E, Wp, ndim, 5.0,
                                     tau.data_ptr(), win.data_ptr(), work.data_ptr(), st.cuda_stream)
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    t_dev, w_dev = tau.cpu().numpy(), win.cpu().numpy()
    res = dict(shape=name, E=E, Wp=Wp, ndim=ndim, samples=n, discard=discard, workspace_MB=nbytes / 2 ** 20,
               call_ms=float(np.min(times)), call_ms_median=float(np.median(times)), reps=reps,
               tau_range=[float(np.nanmin(t_dev)), float(np.nanmax(t_dev))],
               window_range=[int(w_dev.min()), int(w_dev.max())])
    fmas, L = evaluated_fmas(w_dev, n, E, Wp, ndim)
    res.update(round_lags=L, rounds_needed=int(w_dev.max() // L + 1), fmas_evaluated=fmas,
               fmas_all_lags=int(E * Wp * ndim * n * (n + 1) // 2), chain_bytes=int(8 * n * W * ndim))
    # host path on a subset, extrapolated by the number of series
    if E > 1:
        k = min(E, host_subset)
        sub = x[discard:, :k * Wp].cpu().numpy()
        t0 = time.perf_counter()
        for e in range(k):
            integrated_time(sub[:, e * Wp:(e + 1) * Wp], tol=0)
        host_s = time.perf_counter() - t0
        scale = E / k
    else:
        k = min(Wp, max(2, host_subset * 32))
        sub = x[discard:, :k].cpu().numpy()
        t0 = time.perf_counter()
        integrated_time(sub, tol=0)
        host_s = time.perf_counter() - t0
        scale = Wp / k
    res.update(host_subset_series=int(sub.shape[1] * ndim), host_subset_s=host_s,
               host_extrapolated_s=host_s * scale, host_note='extrapolated linearly from the subset, not measured '
               'on the whole chain; excludes the device-to-host copy of the chain')
    del x, work
    torch.cuda.empty_cache()
    return res


def kernel_times(names, reps, outdir):
    """Per-call time of the library's kernels from a separate rocprofv3 run of this script."""
    out = {}
    for name in names:
        d = os.path.join(outdir, f'rocprof_{name}')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', name, '--',
               sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(reps)]
        try:
            rc = subprocess.run(cmd, timeout=600, capture_output=True, text=True).returncode
        except (OSError, subprocess.TimeoutExpired) as e:
            out[name] = dict(error=str(e))
            break
        if rc != 0:
            out[name] = dict(error=f'rocprofv3 exit {rc}')
            break
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not files:
            out[name] = dict(error='no kernel_stats.csv')
            continue
        import csv
        per = {}
        for row in csv.DictReader(open(files[0])):
            m = re.search(r'\bk_ac_\w+', row['Name'])
            if m:
                per[m.group(0)] = (int(row['Calls']), float(row['TotalDurationNs']))
        calls = reps + 2
        out[name] = dict(kernel_ms=sum(v[1] for v in per.values()) / calls / 1e6,
                         per_kernel_ms={k: v[1] / calls / 1e6 for k, v in per.items()},
                         launches_per_call={k: v[0] / calls for k, v in per.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles (or 32 x walkers) the host path times')
    ap.add_argument('--out', help='directory for the JSON lines and the kernel-trace CSVs (default: stdout only)')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('autocorr_bench needs a GPU')
    if args.child:                   # under rocprofv3: the calls only
        E, Wp, ndim, stored, discard = SHAPES[args.child]
        from bisip_amd.autocorr import device_integrated_time
        from bisip_amd.chainview import ChainView
        x = make_chain(E, Wp, ndim, stored)
        W, n = E * Wp, stored - discard
        view = ChainView(x, n, E, Wp, ndim, offset=discard * W * ndim, stride=W * ndim)
        for _ in range(args.reps + 2):
            device_integrated_time(view, 5.0)
        return
    import tempfile
    with tempfile.TemporaryDirectory(prefix='autocorr_bench_') as tmp:
        outdir = args.out or tmp                 # traces are kept only when --out is given
        os.makedirs(outdir, exist_ok=True)
        ceiling = fp64_ceiling()
        names = args.shapes.split(',')
        results = [run_shape(nm, args.reps, args.host_subset) for nm in names]
        prof = {} if args.no_profile else kernel_times(names, args.reps, outdir)
    lines = []
    for r in results:
        r['fp64_fma_ceiling_per_s'] = ceiling
        p = prof.get(r['shape'], {})
        r.update(p)
        t = p.get('kernel_ms') or r['call_ms']
        r['timed_on'] = 'kernel_ms' if p.get('kernel_ms') else 'call_ms (no kernel trace)'
        r['fma_bound_ms'] = r['fmas_evaluated'] / ceiling * 1e3
        r['hbm_bound_ms'] = r['chain_bytes'] / HBM_PEAK * 1e3
        r['frac_of_fma_ceiling'] = r['fma_bound_ms'] / t
        r['frac_of_hbm_peak'] = r['hbm_bound_ms'] / t
        r['bound'] = 'fp64 FMA' if r['fma_bound_ms'] >= r['hbm_bound_ms'] else 'HBM'
        r['speedup_vs_host_extrapolated'] = r['host_extrapolated_s'] * 1e3 / r['call_ms']
        lines.append(json.dumps(r))
        print(lines[-1])
    if args.out:
        with open(os.path.join(args.out, 'autocorr_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')

if __name__ == '__main__':
    main()
