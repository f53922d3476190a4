#!/usr/bin/env python3
"""PolynomialDecomposition's integrating parameters, RTD bands and relaxation descriptors of device-resident chains
(bisip_rtd_integrals_dev, bisip_rtd_columns_dev, bisip_rtd_descriptors_dev + the chain summaries).

Three shapes: the cfg5 slice (512 spectra x 256 walkers, P = 5, 1000 stored, discard 500), one ensemble of
32 walkers x 5000 samples, and one ensemble of 131,072 walkers x 200 samples.  The chains are rows drawn
uniformly from the prior box on the device; log_tau is the 64-point grid of a 32-frequency spectrum.  Per shape:
  * call_ms: device events around the synchronised calls, after warm-up -- integrating mean + std + percentiles as
    the public get_integrating_mean, get_integrating_std and get_integrating_percentile make them (each call
    builds the derived chain again: three integrals launches, two moment passes, one percentile selection), and
    get_rtd_percentile;
  * descriptors_ms, integrals_ms, columns_ms: the three C entry points alone on the same chain -- the relaxation
    descriptors (peak, tau_10, tau_50, tau_90), the integrating parameters, and every m_l in passes under
    decomposition.RTD_PASS_BYTES (no percentile taken) -- medians of 5 with the calls alternating, and the descriptors'
    time as a ratio to the other two;
  * kernel_ms: the library's kernels per call from a separate `rocprofv3 --kernel-trace --stats` run;
  * the integrals kernel's chain bytes over its kernel time, as a fraction of the 8 TB/s HBM peak, and the columns
    kernel's write rate beside the recorded rate of the forward columns kernel (5.3 TB/s, README);
  * the host path (the chain copied with get_chain's device-to-host copy, then the NumPy definitions and
    np.mean / np.std / np.percentile) timed on a subset of ensembles / walkers and extrapolated (labelled so).
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

SHAPES = {   # name: (E, Wp, P, stored, discard)
    'cfg5_slice': (512, 256, 5, 1000, 500),
    'lone_32x5000': (1, 32, 5, 5000, 0),
    'big_131072x200': (1, 131072, 5, 200, 0),
}
HBM_PEAK = 8.0e12              # bytes/s, MI355X spec
FORWARD_COLUMNS_TBS = 5.3      # README: bisip_forward_columns_dev write rate
LOG_TAU = np.linspace(-7.0, 3.0, 64)
P_BAND = [2.5, 50, 97.5]


def make_chain(E, Wp, P, n, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.rand((n, E * Wp, P + 2), generator=g, dtype=torch.float64, device='cuda') * 2.0 - 1.0
    x[..., 0] = 1.0 + 0.1 * x[..., 0]
    return x


def norm_factors(E):
    return np.random.default_rng(0).uniform(0.5, 2.0, E)


def device_calls(x, E, Wp, P, n, discard):
    from bisip_amd import decomposition as dc
    from bisip_amd.chainview import ChainView, device_moments, device_percentiles
    W, ndim = E * Wp, P + 2
    nf = norm_factors(E)

    def view():
        return ChainView(x, n, E, Wp, ndim, offset=discard * W * ndim, stride=W * ndim)

    def derived():
        v = view()
        return v.derived(dc.device_integrating_chain(v, LOG_TAU, nf))

    def integrating():           # get_integrating_mean, get_integrating_std, get_integrating_percentile
        device_moments(derived())
        device_moments(derived())
        device_percentiles(derived(), P_BAND)

    def band():
        dc.device_rtd_percentiles(view(), P_BAND, LOG_TAU)
    return integrating, band


def entry_points(x, E, Wp, P, n, discard):
    """The three C entry points alone on the used samples: (descriptors, integrals, columns), outputs allocated once."""
    import torch
    from bisip_amd import _hip
    from bisip_amd import decomposition as dc
    from bisip_amd.chainview import ChainView
    W, ndim, L = E * Wp, P + 2, LOG_TAU.size
    v = ChainView(x, n, E, Wp, ndim, offset=discard * W * ndim, stride=W * ndim)
    q = np.asarray(dc.DEFAULT_FRACTIONS)
    d_lt, d_q = v.upload(LOG_TAU), v.upload(q)
    d_S, d_nf = v.upload(dc.power_sums(LOG_TAU, ndim)), v.upload(norm_factors(E))
    G = int(min(E, max(1, dc.RTD_PASS_BYTES // (n * Wp * L * 8))))
    out_d = v.empty((n, W, 2 + q.size), torch.float64)
    out_i = v.empty((n, W, 3), torch.float64)
    cols = v.empty((G * L, n * Wp), torch.float64)

    def descriptors():
        _hip.rtd_descriptors_dev(v.ptr, n, v.stride, E, Wp, ndim, d_lt.data_ptr(), L, d_q.data_ptr(), q.size,
                                 out_d.data_ptr(), v.stream)

    def integrals():
        _hip.rtd_integrals_dev(v.ptr, n, v.stride, E, Wp, ndim, d_S.data_ptr(), d_nf.data_ptr(), out_i.data_ptr(), v.stream)

    def columns():
        for g0 in range(0, E, G):
            _hip.rtd_columns_dev(v.ptr, n, v.stride, E, Wp, ndim, g0, min(E, g0 + G) - g0, d_lt.data_ptr(), L,
                                 cols.data_ptr(), v.stream)
    return descriptors, integrals, columns


def timed_alternating(fs, reps=5):
    """Median device time (ms) of each call of ``fs``, taken in turn ``reps`` times after one warm-up round."""
    import torch
    for f in fs:
        f()
    torch.cuda.synchronize()
    times = [[] for _ in fs]
    for _ in range(reps):
        for f, ts in zip(fs, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return [float(np.median(ts)) for ts in times]


def timed(f, reps):
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


def host_path(x, E, Wp, P, discard, subset):
    """get_chain's copy of a subset plus the NumPy definitions and summaries, timed; scale to the whole chain."""
    from bisip_amd.decomposition import integrating_params, rtd
    nf = norm_factors(E)
    if E > 1:
        k = min(E, subset)
        part, scale = x[discard:, :k * Wp], E / k
        nf_rows = np.repeat(nf[:k], Wp)
    else:
        k = min(Wp, max(32, subset * 1024))
        part, scale = x[discard:, :k], Wp / k
        nf_rows = np.full(k, nf[0])
    t0 = time.perf_counter()
    ch = part.cpu().numpy()
    t1 = time.perf_counter()
    n, w = ch.shape[:2]
    groups = max(1, w // Wp)
    ip = integrating_params(ch, LOG_TAU, nf_rows)                       # (n, w, 3)
    ipg = ip.reshape(n, groups, -1, 3).transpose(1, 0, 2, 3).reshape(groups, -1, 3)
    ipg.mean(axis=1), ipg.std(axis=1), np.percentile(ipg, P_BAND, axis=1)
    t2 = time.perf_counter()
    m = rtd(ch, LOG_TAU)                                                # (n, w, L)
    mg = m.reshape(n, groups, -1, LOG_TAU.size).transpose(1, 0, 2, 3).reshape(groups, -1, LOG_TAU.size)
    np.percentile(mg, P_BAND, axis=1)
    t3 = time.perf_counter()
    return dict(host_subset_rows=int(n * w), host_copy_s=(t1 - t0) * scale,
                host_integrating_extrapolated_s=(t2 - t0) * scale,
                host_rtd_band_extrapolated_s=((t1 - t0) + (t3 - t2)) * scale,
                host_note='extrapolated linearly from the subset (copy included), not measured on the whole chain')


def run_shape(name, reps, subset):
    import torch
    E, Wp, P, stored, discard = SHAPES[name]
    W, n, ndim, L = E * Wp, stored - discard, P + 2, LOG_TAU.size
    x = make_chain(E, Wp, P, stored)
    integrating, band = device_calls(x, E, Wp, P, n, discard)
    ims, ims_med = timed(integrating, reps)
    bms, bms_med = timed(band, reps)
    res = dict(shape=name, E=E, Wp=Wp, P=P, L=L, samples=n, discard=discard, reps=reps,
               integrating_call_ms=ims, integrating_call_ms_median=ims_med,
               rtd_band_call_ms=bms, rtd_band_call_ms_median=bms_med,
               chain_bytes=int(8 * n * W * ndim), derived_bytes=int(8 * n * W * 3), columns_bytes=int(8 * n * W * L))
    dms, ims3, cms = timed_alternating(entry_points(x, E, Wp, P, n, discard))
    res.update(descriptors_ms=dms, integrals_ms=ims3, columns_ms=cms, descriptors_over_integrals=dms / ims3,
               descriptors_over_columns=dms / cms, descriptor_bytes=int(8 * n * W * 5))
    torch.cuda.empty_cache()
    res.update(host_path(x, E, Wp, P, discard, subset))
    del x
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
            m = re.search(r'\bk_(rtd_integrals|rtd_columns|rtd_descriptors|moments_\w+|gather_columns\w*|segmented_select|percentile_lerp)'
                          r'|DeviceSegmentedRadixSort|segmented_sort', row['Name'])
            if m:
                key = m.group(0)
                c, t = per.get(key, (0, 0.0))
                per[key] = (c + int(row['Calls']), t + float(row['TotalDurationNs']))
        calls = reps + 2
        out[name] = dict(kernel_ms_per_call={k: v[1] / calls / 1e6 for k, v in per.items()},
                         launches_per_call={k: v[0] / calls for k, v in per.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles (or 1024 x walkers) the host path times')
    ap.add_argument('--out', help='directory for the JSON lines and the kernel-trace CSVs (default: stdout only)')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('decomposition_bench needs a GPU')
    if args.child:                   # under rocprofv3: the calls only (each call = integrating + band)
        E, Wp, P, stored, discard = SHAPES[args.child]
        x = make_chain(E, Wp, P, stored)
        integrating, band = device_calls(x, E, Wp, P, stored - discard, discard)
        descriptors = entry_points(x, E, Wp, P, stored - discard, discard)[0]
        for _ in range(args.reps + 2):
            integrating()
            band()
            descriptors()
        torch.cuda.synchronize()
        return
    import tempfile
    with tempfile.TemporaryDirectory(prefix='decomposition_bench_') as tmp:
        outdir = args.out or tmp
        os.makedirs(outdir, exist_ok=True)
        names = args.shapes.split(',')
        results = [run_shape(nm, args.reps, args.host_subset) for nm in names]
        prof = {} if args.no_profile else kernel_times(names, args.reps, outdir)
    lines = []
    for r in results:
        p = prof.get(r['shape'], {})
        r.update(p)
        k = p.get('kernel_ms_per_call', {})
        if 'k_rtd_integrals' in k:       # per launch (three per call)
            r['integrals_kernel_ms'] = k['k_rtd_integrals'] / p['launches_per_call']['k_rtd_integrals']
            r['integrals_chain_TBps'] = r['chain_bytes'] / (r['integrals_kernel_ms'] * 1e-3) / 1e12
            r['integrals_frac_of_hbm_peak'] = r['chain_bytes'] / (r['integrals_kernel_ms'] * 1e-3) / HBM_PEAK
        if 'k_rtd_descriptors' in k:
            r['descriptors_kernel_ms'] = k['k_rtd_descriptors']
        if 'k_rtd_columns' in k:         # all passes of one call
            r['columns_kernel_ms'] = k['k_rtd_columns']
            r['columns_write_TBps'] = r['columns_bytes'] / (k['k_rtd_columns'] * 1e-3) / 1e12
            r['forward_columns_write_TBps_recorded'] = FORWARD_COLUMNS_TBS
        r['integrating_speedup_vs_host_extrapolated'] = r['host_integrating_extrapolated_s'] * 1e3 / r['integrating_call_ms']
        r['rtd_band_speedup_vs_host_extrapolated'] = r['host_rtd_band_extrapolated_s'] * 1e3 / r['rtd_band_call_ms']
        lines.append(json.dumps(r))
        print(lines[-1])
    if args.out:
        with open(os.path.join(args.out, 'decomposition_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
