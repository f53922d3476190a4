#!/usr/bin/env python3
"""Posterior covariance and best sample of device-resident chains (bisip_chain_cov_dev, bisip_chain_best_sample_dev).

Shapes: the README's survey slice (512 spectra x 256 walkers x 500 used samples x 7, read through discard = 10 and thin = 2
of 1010 stored samples), half of it (256 spectra, the fewest that take the one-kernel path: one workgroup per CU), the same
walkers at ndim 16 (250 used samples), one big ensemble (32,768 walkers x 200 x 7) and the quickstart (32 walkers x 5000 x
7: cut into segments).  The chain is a Gaussian around a centre per ensemble, made on the
device; the log-probability is a standard normal.  Per shape, in one process, device events around each call after two
warm-up calls (outputs and workspaces allocated once), best and median of --reps:
  * cov_ms, best_ms: the two new entry points;
  * rhat_ms: bisip_chain_rhat_dev (splits = 2, R-hat alone), ONE coalesced pass over the chain, and moments_ms:
    bisip_chain_moments_dev, TWO passes -- existing code on the same chain, the yardsticks, timed before and after;
  * the used chain's bytes n * E * Wp * ndim * 8 over each time and that as a fraction of the 8 TB/s HBM peak (the best
    sample reads the log-probability, 1 / ndim of it, and one row per ensemble);
  * cov_over_moments and cov_over_rhat;
  * the host path: np.cov and np.argmax per ensemble on a host copy of a subset (8 ensembles, or 1/16 of the walkers of a
    lone ensemble), extrapolated linearly (labelled as such; the device-to-host copy is timed apart).
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

from trace_bench import HBM_PEAK, make_chain, time_call      # noqa: E402

SHAPES = {   # name: (E, Wp, ndim, used samples, discard, thin)
    'survey_512x256x500': (512, 256, 7, 500, 10, 2),
    'survey_256x256x500': (256, 256, 7, 500, 10, 2),      # the fewest ensembles that take one workgroup each: one per CU
    'survey_ndim16_512x256x250': (512, 256, 16, 250, 10, 2),
    'one_ensemble_32768x200': (1, 32768, 7, 200, 0, 1),
    'quickstart_32x5000': (1, 32, 7, 5000, 0, 1),
}


class Calls:
    """The calls on the used samples of one stored chain, outputs and workspaces allocated once."""

    def __init__(self, x, lp, E, Wp, ndim, n, discard, thin):
        import torch
        from bisip_amd import _hip
        self.hip, self.x, self.lp, self.E, self.Wp, self.ndim, self.n = _hip, x, lp, E, Wp, ndim, n
        row, first = E * Wp * ndim, discard + thin - 1
        self.ptr, self.stride = x.data_ptr() + 8 * first * row, thin * row
        self.lptr, self.lstride = lp.data_ptr() + 8 * first * E * Wp, thin * E * Wp
        self.st = torch.cuda.current_stream().cuda_stream
        dev = x.device

        def empty(shape, dtype=torch.float64):
            return torch.empty(shape, dtype=dtype, device=dev)

        self.cov, self.mean, self.std = empty((E, ndim, ndim)), empty((E, ndim)), empty((E, ndim))
        self.theta, self.best, self.index = empty((E, ndim)), empty((E,)), empty((E,), torch.int64)
        self.rh = empty((E, ndim))
        self.cbytes = _hip.chain_cov_workspace(n, E, Wp, ndim)
        self.bbytes = _hip.chain_best_sample_workspace(n, E, Wp)
        self.rbytes = _hip.chain_rhat_workspace(n, E, Wp, ndim, 2)
        self.cwork = empty((max(1, self.cbytes),), torch.uint8)
        self.bwork = empty((max(1, self.bbytes),), torch.uint8)
        self.rwork = empty((max(1, self.rbytes),), torch.uint8)
        self.mwork = empty((max(1, _hip.chain_moments_workspace(n, E, ndim)),))

    def cov_(self):
        self.hip.chain_cov_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                               self.cov.data_ptr(), self.cwork.data_ptr(), self.cbytes, self.st)

    def best_(self):
        self.hip.chain_best_sample_dev(self.ptr, self.stride, self.lptr, self.lstride, self.n, self.E, self.Wp, self.ndim,
                                       self.theta.data_ptr(), self.best.data_ptr(), self.index.data_ptr(),
                                       self.bwork.data_ptr(), self.bbytes, self.st)

    def rhat(self):
        self.hip.chain_rhat_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, 2, 0, 0, self.rh.data_ptr(),
                                self.rwork.data_ptr(), self.rbytes, self.st)

    def moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.mean.data_ptr(),
                                   self.std.data_ptr(), self.mwork.data_ptr(), self.st)


def host_path(c, used, used_lp, host_subset):
    """np.cov and np.argmax per ensemble on a host copy of a subset of the used samples, extrapolated by its share."""
    E, Wp, ndim = c.E, c.Wp, c.ndim
    if E > 1:
        k = min(E, host_subset)
        part, lpart, scale, wk = used[:, :k * Wp], used_lp[:, :k * Wp], E / k, Wp
    else:
        k, wk = 1, max(2, Wp // 16)
        part, lpart, scale = used[:, :wk], used_lp[:, :wk], Wp / wk
    t0 = time.perf_counter()
    sub, lsub = part.cpu().numpy(), lpart.cpu().numpy()
    copy_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    covs = np.stack([np.cov(sub[:, e * wk:(e + 1) * wk].reshape(-1, ndim).T) for e in range(k)])
    idx = np.array([np.argmax(lsub[:, e * wk:(e + 1) * wk].reshape(-1)) for e in range(k)])
    host_s = time.perf_counter() - t0
    if E > 1:               # (a subset of a lone ensemble's walkers has another covariance)
        assert np.allclose(c.cov[:k].cpu().numpy(), covs, rtol=1e-9, atol=0), 'device covariance differs from np.cov'
        assert (c.index[:k].cpu().numpy() == idx).all(), 'device best sample differs from np.argmax'
    return dict(host_subset_values=int(sub.size), host_copy_subset_s=copy_s, host_cov_argmax_subset_s=host_s,
                host_cov_argmax_extrapolated_s=host_s * scale, host_copy_extrapolated_s=copy_s * scale,
                host_note='extrapolated linearly from the subset, not measured on the whole chain')


def run(name, reps, host_subset):
    import torch
    from bisip_amd import covariance as cv
    E, Wp, ndim, n, discard, thin = SHAPES[name]
    stored = discard + thin * n
    x = make_chain(E, Wp, ndim, stored)
    lp = torch.randn((stored, E * Wp), dtype=torch.float64, device='cuda',
                     generator=torch.Generator(device='cuda').manual_seed(1))
    c = Calls(x, lp, E, Wp, ndim, n, discard, thin)
    chain_bytes = 8 * n * E * Wp * ndim
    seg_rows, nseg, slots = cv.plan(n, E, Wp, ndim)
    res = dict(shape=name, E=E, Wp=Wp, ndim=ndim, samples=n, discard=discard, thin=thin, chain_bytes=chain_bytes, reps=reps,
               cov_workspace_bytes=c.cbytes, cov_segments=nseg, cov_segment_rows=seg_rows, cov_row_slots=slots,
               best_segments=cv.best_plan(n, E, Wp)[1])
    for what in ('moments', 'rhat', 'cov_', 'best_', 'rhat', 'moments'):        # (the yardsticks before and after: best of both)
        key = what.rstrip('_')
        best, med = time_call(getattr(c, what), reps)
        if key + '_ms' in res:
            best, med = min(best, res[key + '_ms']), min(med, res[key + '_ms_median'])
        res[key + '_ms'], res[key + '_ms_median'] = best, med
    for key in ('moments', 'rhat', 'cov', 'best'):
        rate = chain_bytes / (res[key + '_ms'] * 1e-3)
        if key == 'best':
            rate /= ndim                                            # it reads the log-probability only
        res[key + '_TBps'] = rate / 1e12
        res[key + '_frac_of_hbm_peak'] = rate / HBM_PEAK
    res['cov_over_moments'] = res['cov_ms'] / res['moments_ms']
    res['cov_over_rhat'] = res['cov_ms'] / res['rhat_ms']
    first = discard + thin - 1
    res.update(host_path(c, x[first::thin], lp[first::thin], host_subset))
    res['speedup_vs_host_extrapolated'] = res['host_cov_argmax_extrapolated_s'] * 1e3 / (res['cov_ms'] + res['best_ms'])
    del x, lp, c
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-subset', type=int, default=8, help='ensembles the host path times')
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('covariance_bench needs a GPU')
    lines = []
    for name in args.shapes.split(','):
        lines.append(json.dumps(run(name, args.reps, args.host_subset)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'covariance_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
