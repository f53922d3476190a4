#!/usr/bin/env python3
"""Highest-density intervals of device-resident chains (bisip_chain_hdi_dev): its two paths against each other and
against what the library had before.

Shapes: the README's survey slice (512 spectra x 256 walkers, 500 used of 1000 stored samples: thin = 2, ndim 7) and one
model's chain (32 walkers x 5000 samples x 7: seven columns of 160,000 values).  The chain is a Gaussian around a centre per
ensemble, made on the device.  Per shape, in one process, device events around each call after two warm-up calls (outputs
and workspaces allocated once), medians (and the best) of --reps, the two paths ALTERNATING call by call so that both see
the same clocks:
  * hdi_full_ms / hdi_tails_ms for mass 0.95 and for (0.5, 0.9, 0.95) in one call, forced with BISIP_HDI_PATH; hdi_rule_ms
    with the variable unset, and the path interval.plan gives;
  * sort_ms: bisip_chain_percentiles_dev of [2.5, 97.5] on the same chain forced through its segmented sort
    (BISIP_PERCENTILE_SORT=1) -- "gather + sort everything", what an HDI would have cost with the kernels the library
    had; select_ms: the same call through the selection kernel, the equal-tailed interval as it is shipped;
  * moments_ms: bisip_chain_moments_dev, two passes over the chain -- the bandwidth floor the other benches quote;
  * the host path: interval.hdi in NumPy on a host copy of 8 spectra, extrapolated linearly (labelled as such; the
    device-to-host copy is timed apart).
The engine clocks are not read: a ratio of two alternating calls does not need them, an absolute time is the box's.
Prints one JSON line per shape; with --out DIR also writes them there."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_bench import HBM_PEAK, make_chain      # noqa: E402

SHAPES = {   # name: (E, Wp, ndim, used samples, discard, thin)
    'survey_512x256x500': (512, 256, 7, 500, 0, 2),
    'one_model_32x5000': (1, 32, 7, 5000, 0, 1),
}
MASS_SETS = {'mass95': (0.95,), 'mass50_90_95': (0.5, 0.9, 0.95)}


class Calls:
    """The calls on the used samples of one stored chain, outputs and workspaces allocated once (the workspace of the
    larger path serves both)."""

    def __init__(self, x, E, Wp, ndim, n, discard, thin):
        import torch
        from bisip_amd import _hip, interval
        self.hip, self.x, self.E, self.Wp, self.ndim, self.n = _hip, x, E, Wp, ndim, n
        row, first = E * Wp * ndim, discard + thin - 1
        self.ptr, self.stride = x.data_ptr() + 8 * first * row, thin * row
        self.st = torch.cuda.current_stream().cuda_stream
        dev = x.device

        def empty(shape, dtype=torch.float64):
            return torch.empty(shape, dtype=dtype, device=dev)

        self.K = {name: interval.windows(m, n * Wp) for name, m in MASS_SETS.items()}
        self.out = empty((3, 2, E, ndim))
        self.index = empty((3, E, ndim), torch.int64)
        self.hbytes = {}
        for name, K in self.K.items():
            for path in ('full', 'tails', None):
                self.set_path(path)
                self.hbytes[name, path] = _hip.chain_hdi_workspace(n, E, Wp, ndim, K)
        self.set_path(None)
        self.hwork = empty((max(self.hbytes.values()),), torch.uint8)
        self.pct = empty((2, E, ndim))
        self.pbytes = _hip.chain_percentiles_workspace(n, E, Wp, ndim, 2)
        self.pwork = empty((self.pbytes,), torch.uint8)
        self.mean, self.std = empty((E, ndim)), empty((E, ndim))
        self.mwork = empty((max(1, _hip.chain_moments_workspace(n, E, ndim)),))

    @staticmethod
    def set_path(path):
        if path is None:
            os.environ.pop('BISIP_HDI_PATH', None)
        else:
            os.environ['BISIP_HDI_PATH'] = path

    def hdi(self, name, path):
        self.set_path(path)
        self.hip.chain_hdi_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.K[name], self.out.data_ptr(),
                               self.index.data_ptr(), self.hwork.data_ptr(), self.hbytes[name, path], self.st)

    def percentiles(self, sort):
        os.environ['BISIP_PERCENTILE_SORT'] = '1' if sort else '0'
        self.hip.chain_percentiles_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, np.array([2.5, 97.5]),
                                       self.pct.data_ptr(), self.pwork.data_ptr(), self.pbytes, self.st)

    def moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                                   self.std.data_ptr(), self.mwork.data_ptr(), self.st)


def time_alternating(calls, reps):
    """{name: (best, median) ms} of several calls timed in turn, rep by rep, after two warm-up rounds."""
    import torch
    for _ in range(2):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (float(np.min(v)), float(np.median(v))) for k, v in times.items()}


def host_path(c, used, host_subset):
    """interval.hdi in NumPy on a host copy of a subset of the ensembles, extrapolated by its share."""
    from bisip_amd import interval
    k = min(c.E, host_subset)
    part = used[:, :k * c.Wp]
    t0 = time.perf_counter()
    sub = part.cpu().numpy()
    copy_s = time.perf_counter() - t0
    res = dict(host_subset_ensembles=k, host_subset_values=int(sub.size), host_copy_subset_s=copy_s,
               host_copy_extrapolated_s=copy_s * c.E / k,
               host_note='extrapolated linearly from the subset, not measured on the whole chain')
    for name, masses in MASS_SETS.items():
        t0 = time.perf_counter()
        want, widx = interval.hdi(sub, masses, k, index=True)
        host_s = time.perf_counter() - t0
        for path in ('full', 'tails'):                    # the device's answer is the definition's, on either path
            c.hdi(name, path)
            got, gidx = c.out[:len(masses), :, :k].cpu().numpy(), c.index[:len(masses), :k].cpu().numpy()
            assert (got == want).all() and (gidx == widx).all(), f'device HDI ({path}) differs from interval.hdi'
        res[f'host_hdi_{name}_subset_s'] = host_s
        res[f'host_hdi_{name}_extrapolated_s'] = host_s * c.E / k
    return res


def run(name, reps, host_subset):
    import torch
    from bisip_amd import interval
    E, Wp, ndim, n, discard, thin = SHAPES[name]
    x = make_chain(E, Wp, ndim, discard + thin * n)
    c = Calls(x, E, Wp, ndim, n, discard, thin)
    chain_bytes = 8 * n * E * Wp * ndim
    res = dict(shape=name, E=E, Wp=Wp, ndim=ndim, samples=n, stored=discard + thin * n, discard=discard, thin=thin,
               column_values=n * Wp, columns=E * ndim, chain_bytes=chain_bytes, reps=reps, clocks='not read',
               timing='device events, medians of reps, the calls of a group alternating rep by rep')
    for mname in MASS_SETS:
        res[f'rule_{mname}'] = interval.plan(n, E, Wp, ndim, c.K[mname])
        res[f'workspace_bytes_{mname}'] = {str(p): c.hbytes[mname, p] for p in ('full', 'tails')}
        t = time_alternating({'full': lambda: c.hdi(mname, 'full'), 'tails': lambda: c.hdi(mname, 'tails'),
                              'rule': lambda: c.hdi(mname, None)}, reps)
        for path, (best, med) in t.items():
            res[f'hdi_{path}_{mname}_ms'], res[f'hdi_{path}_{mname}_ms_best'] = med, best
        res[f'tails_over_full_{mname}'] = t['tails'][1] / t['full'][1]
    t = time_alternating({'sort': lambda: c.percentiles(True), 'select': lambda: c.percentiles(False), 'moments': c.moments,
                          'full': lambda: c.hdi('mass95', 'full'), 'tails': lambda: c.hdi('mass95', 'tails')}, reps)
    os.environ.pop('BISIP_PERCENTILE_SORT', None)
    for key in ('sort', 'select', 'moments'):
        res[f'{key}_ms'], res[f'{key}_ms_best'] = t[key][1], t[key][0]
    res['hdi_full_mass95_over_sort'] = t['full'][1] / t['sort'][1]
    res['hdi_tails_mass95_over_sort'] = t['tails'][1] / t['sort'][1]
    res['hdi_tails_mass95_over_moments'] = t['tails'][1] / t['moments'][1]
    res['hdi_tails_mass95_over_select'] = t['tails'][1] / t['select'][1]
    res['moments_frac_of_hbm_peak'] = 2 * chain_bytes / (t['moments'][1] * 1e-3) / HBM_PEAK      # (it reads the chain twice)
    first = discard + thin - 1
    res.update(host_path(c, x[first::thin], host_subset))
    best_dev = min(res['hdi_full_mass95_ms'], res['hdi_tails_mass95_ms'])
    res['speedup_vs_host_extrapolated_mass95'] = res['host_hdi_mass95_extrapolated_s'] * 1e3 / best_dev
    Calls.set_path(None)
    del x, c
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles the host path times')
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('interval_bench needs a GPU')
    lines = []
    for name in args.shapes.split(','):
        lines.append(json.dumps(run(name, args.reps, args.host_subset)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'interval_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
