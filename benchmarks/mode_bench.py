#!/usr/bin/env python3
"""The ordering of Cole-Cole modes and the per-mode descriptors of device-resident chains (bisip_mode_order_dev).

Three shapes: the cfg5 slice (512 spectra x 256 walkers, 500 used of 1000 stored samples) with K = 2 and with K = 5 modes, and
one model's 32 walkers x 5000 samples with K = 2.  The chains are rows drawn uniformly from the default prior box on the
device.  Per shape, medians of 5 device-event times with the calls alternating, and the spread (min, max) of the five:
  * desc_ms: bisip_mode_order_dev asked for the descriptors alone;
  * all_ms: asked for the ordered rows, the descriptors and ``moved``;
  * integrals_ms: bisip_rtd_integrals_dev on the same chain read as a PolynomialDecomposition chain of equal ndim -- the same
    grid and the same row reads, three doubles written per row.
Both kernels should be bound by the bytes they move, so the expected ratio of their times is the ratio of bytes per row:
(8 ndim + 8 (1 + 2K)) / (8 ndim + 24) for the descriptors alone and (16 ndim + 8 (1 + 2K) + 1) / (8 ndim + 24) for all three
outputs (K = 2: 96 / 80 = 1.2 and 153 / 80 = 1.9).  The measured ratios stand beside the expected ones.
The host path -- order_modes and mode_descriptors in NumPy on a get_chain-style copy -- is timed on 8 spectra (or the whole
lone chain) and extrapolated linearly to the shape (labelled so).
Prints one JSON line per shape; with --out DIR also writes them to DIR/mode_bench.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # name: (E, Wp, K, stored, discard)
    'cfg5_slice_K2': (512, 256, 2, 1000, 500),
    'cfg5_slice_K5': (512, 256, 5, 1000, 500),
    'lone_32x5000_K2': (1, 32, 2, 5000, 0),
}
HBM_PEAK = 8.0e12              # bytes/s, MI355X spec
LOG_TAU = np.linspace(-7.0, 3.0, 64)


def make_chain(E, Wp, K, n, seed=0):
    """(n, E * Wp, 1 + 3K) rows uniform in the default box of PeltonColeCole, on the device."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.rand((n, E * Wp, 1 + 3 * K), generator=g, dtype=torch.float64, device='cuda')
    x[..., 0] = 0.9 + 0.2 * x[..., 0]
    x[..., 1 + K:1 + 2 * K] = -15.0 + 20.0 * x[..., 1 + K:1 + 2 * K]
    return x


def entry_points(x, E, Wp, K, n, discard):
    """(descriptors alone, all three outputs, the integrals of a PolynomialDecomposition chain of equal ndim), outputs
    allocated once."""
    import torch
    from bisip_amd import _hip
    from bisip_amd import decomposition as dc
    from bisip_amd.chainview import ChainView
    W, ndim = E * Wp, 1 + 3 * K
    v = ChainView(x, n, E, Wp, ndim, offset=discard * W * ndim, stride=W * ndim)
    d_S, d_nf = v.upload(dc.power_sums(LOG_TAU, ndim)), v.upload(np.ones(E))
    out_o = v.empty((n, W, ndim), torch.float64)
    out_d = v.empty((n, W, 1 + 2 * K), torch.float64)
    out_m = v.empty((n, W), torch.uint8)
    out_i = v.empty((n, W, 3), torch.float64)

    def descriptors():
        _hip.mode_order_dev(v.ptr, n, v.stride, E, Wp, K, 1, 0, out_d.data_ptr(), 0, v.stream)

    def everything():
        _hip.mode_order_dev(v.ptr, n, v.stride, E, Wp, K, 1, out_o.data_ptr(), out_d.data_ptr(), out_m.data_ptr(), v.stream)

    def integrals():
        _hip.rtd_integrals_dev(v.ptr, n, v.stride, E, Wp, ndim, d_S.data_ptr(), d_nf.data_ptr(), out_i.data_ptr(), v.stream)
    return descriptors, everything, integrals


def timed_alternating(fs, reps=5):
    """The device times (ms) of each call of ``fs``, taken in turn ``reps`` times after one warm-up round: a list per call."""
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
    return times


def host_path(x, E, Wp, K, discard, subset):
    """A copy of ``subset`` spectra's used samples, then the NumPy definitions; scaled to the whole chain."""
    from bisip_amd.modes import mode_descriptors, order_modes
    k = min(E, subset)
    part, scale = x[discard:, :k * Wp], E / k
    t0 = time.perf_counter()
    ch = part.cpu().numpy()
    t1 = time.perf_counter()
    order_modes(ch, K)
    t2 = time.perf_counter()
    mode_descriptors(ch, K)
    t3 = time.perf_counter()
    return dict(host_subset_rows=int(ch.shape[0] * ch.shape[1]), host_copy_extrapolated_s=(t1 - t0) * scale,
                host_order_extrapolated_s=(t2 - t1) * scale, host_descriptors_extrapolated_s=(t3 - t2) * scale,
                host_note='extrapolated linearly from the subset, not measured on the whole chain')


def run_shape(name, subset):
    import torch
    E, Wp, K, stored, discard = SHAPES[name]
    W, n, ndim = E * Wp, stored - discard, 1 + 3 * K
    x = make_chain(E, Wp, K, stored)
    td, ta, ti = timed_alternating(entry_points(x, E, Wp, K, n, discard))
    med = lambda ts: float(np.median(ts))
    spread = lambda ts: [float(min(ts)), float(max(ts))]
    rows = n * W
    bytes_d, bytes_a, bytes_i = rows * (8 * ndim + 8 * (1 + 2 * K)), rows * (16 * ndim + 8 * (1 + 2 * K) + 1), rows * (8 * ndim + 24)
    res = dict(shape=name, E=E, Wp=Wp, K=K, ndim=ndim, samples=n, discard=discard, reps=5,
               desc_ms=med(td), desc_ms_spread=spread(td), all_ms=med(ta), all_ms_spread=spread(ta),
               integrals_ms=med(ti), integrals_ms_spread=spread(ti),
               desc_over_integrals=med(td) / med(ti), desc_over_integrals_expected=bytes_d / bytes_i,
               all_over_integrals=med(ta) / med(ti), all_over_integrals_expected=bytes_a / bytes_i,
               desc_TBps=bytes_d / (med(td) * 1e-3) / 1e12, all_TBps=bytes_a / (med(ta) * 1e-3) / 1e12,
               integrals_TBps=bytes_i / (med(ti) * 1e-3) / 1e12, hbm_peak_TBps=HBM_PEAK / 1e12)
    torch.cuda.empty_cache()
    res.update(host_path(x, E, Wp, K, discard, subset))
    res['desc_speedup_vs_host_extrapolated'] = (res['host_copy_extrapolated_s'] + res['host_descriptors_extrapolated_s']) * 1e3 / res['desc_ms']
    del x
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--host-subset', type=int, default=8, help='spectra the host path times')
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mode_bench needs a GPU')
    lines = []
    for name in args.shapes.split(','):
        lines.append(json.dumps(run_shape(name, args.host_subset)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'mode_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
