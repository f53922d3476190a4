#!/usr/bin/env python3
"""Per-point fit quality of device-resident chains (bisip_fit_quality_dev): mean and variance of q = (y - Z)^2 / sigma^2 and
log mean exp(-q / 2) per data point, what WAIC and the per-point misfit are made of.

Shape: the README's survey slice as response_bench.py -- 512 spectra x 256 walkers x 500 used samples of 1000 stored
(discard = 0, thin = 2), N = 32 synthetic frequencies, for the double Cole-Cole model and PolynomialDecomposition (degree
5); --quick: 16 spectra x 64 walkers x 50 of 100, for a machine that is shared.  The chain is response_bench's.  In one
process, device events around each whole call, two warm-up calls each, then --repeats (default 5) rounds in which the
three calls alternate; the medians are reported, the repeats kept:
  * fit_ms: the fused kernel, all spectra in one launch, the three outputs; chain bytes over the time and model
    evaluations (rows x N) per second;
  * moments_ri_ms: bisip_response_moments_dev kind 'ri' on the same chain -- the same evaluation with two running sums per
    point instead of four and no exp; fit_over_moments_ri is what the two more states and the exp cost;
  * unfused_ms: what Python allows without the kernel -- per pass (spectra under decomposition.RTD_PASS_BYTES) the copy of
    the rows, forward_columns_dev into Re / Im columns, torch elementwise ops for q in place, torch.mean, torch.var
    and torch.logsumexp over the columns; unfused_over_fit.
Prints one JSON line per model; with --out DIR also writes them to DIR/fit_quality_bench.jsonl."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from response_bench import MODELS, N_FREQ, SHAPES, make_chain      # noqa: E402
from trace_bench import HBM_PEAK                                    # noqa: E402


class Calls:
    def __init__(self, batch, x, E, Wp, n, discard, thin):
        import torch
        from bisip_amd import decomposition, fitquality
        self.ctx, self.torch = batch.ctx, torch
        self.E, self.Wp, self.n, self.ndim, self.N = E, Wp, n, batch.ndim, batch.N
        first, row = discard + thin - 1, E * Wp * batch.ndim
        self.ptr, self.stride = x.data_ptr() + 8 * first * row, thin * row
        self.grid = x[first::thin][:n].reshape(n, E, Wp, batch.ndim)
        self.st = torch.cuda.current_stream().cuda_stream
        self.rows_per, cols = n * Wp, 2 * batch.N
        self.G = G = int(min(E, max(1, decomposition.RTD_PASS_BYTES // (self.rows_per * cols * 8))))

        def empty(*shape):
            return torch.empty(shape, dtype=torch.float64, device=x.device)

        self.rows, self.cols = empty(G, n, Wp, batch.ndim), empty(G, cols, self.rows_per)
        self.y = torch.from_numpy(batch.zn.reshape(E, cols, 1)).to(x.device)
        self.iv = torch.from_numpy(fitquality.inverse_variance(batch.zn_err).reshape(E, cols, 1)).to(x.device)
        self.out = empty(3, E, 2, batch.N)                         # the fused kernel's mean_q, var_q, lmeh
        self.un = empty(3, E, cols)                                # the unfused route's
        self.mean, self.std = empty(E, 2, batch.N), empty(E, 2, batch.N)
        self.fbytes = self.ctx.fit_quality_workspace(n, E, Wp)
        self.mbytes = self.ctx.response_moments_workspace(n, E, Wp)
        self.work = torch.empty((max(1, self.fbytes, self.mbytes),), dtype=torch.uint8, device=x.device)

    def fit(self):
        self.ctx.fit_quality_dev(0, self.E, self.ptr, self.n, self.stride, self.Wp, self.out[0].data_ptr(),
                                 self.out[1].data_ptr(), self.out[2].data_ptr(), self.work.data_ptr(), self.fbytes, self.st)

    def moments_ri(self):
        self.ctx.response_moments_dev(0, self.E, self.ptr, self.n, self.stride, self.Wp, 'ri', self.mean.data_ptr(),
                                      self.std.data_ptr(), self.work.data_ptr(), self.mbytes, self.st)

    def unfused(self):
        torch = self.torch
        for g0 in range(0, self.E, self.G):
            k = min(self.E, g0 + self.G) - g0
            self.rows[:k].copy_(self.grid[:, g0:g0 + k].permute(1, 0, 2, 3))        # spectrum-major, as the summaries do
            self.ctx.forward_columns_dev(g0, k, self.rows.data_ptr(), k * self.rows_per, self.cols.data_ptr(), self.st)
            q = self.cols[:k]
            torch.sub(self.y[g0:g0 + k], q, out=q)
            q.mul_(q).mul_(self.iv[g0:g0 + k])
            torch.mean(q, dim=-1, out=self.un[0, g0:g0 + k])
            torch.var(q, dim=-1, correction=1, out=self.un[1, g0:g0 + k])
            q.mul_(-0.5)
            torch.logsumexp(q, dim=-1, out=self.un[2, g0:g0 + k])
        self.un[2].sub_(math.log(self.rows_per))


def timed(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(model, shape, repeats):
    import torch
    import bisip_amd
    from bisip_amd import response as rs
    from bisip_amd.synthetic import synthetic_columns
    E, Wp, n, discard, thin = SHAPES[shape]
    batch = bisip_amd.SpectraBatch(model, [synthetic_columns(N_FREQ, i) for i in range(E)], nwalkers=Wp, nsteps=8, **MODELS[model])
    stored = discard + thin * n
    x = make_chain(model, *batch.param_bounds, stored, E * Wp)
    c = Calls(batch, x, E, Wp, n, discard, thin)
    chain_bytes = 8 * n * E * Wp * batch.ndim
    seg_rows, nseg, _ = rs.plan(n, E, Wp)
    res = dict(model=model, options=MODELS[model], shape=shape, E=E, Wp=Wp, N=N_FREQ, ndim=batch.ndim, samples=n, stored=stored,
               discard=discard, thin=thin, chain_bytes=chain_bytes, column_bytes=8 * n * E * Wp * 2 * N_FREQ, passes=-(-E // c.G),
               spectra_per_pass=c.G, segments=nseg, segment_rows=seg_rows, fit_workspace_bytes=c.fbytes, repeats=repeats)
    calls = dict(fit=c.fit, moments_ri=c.moments_ri, unfused=c.unfused)
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(repeats):                                         # alternating on one box
        for k, f in calls.items():
            times[k].append(timed(f))
    for k, v in times.items():
        res[k + '_ms'], res[k + '_ms_repeats'] = float(np.median(v)), v
    res['spread'] = float((max(times['moments_ri']) - min(times['moments_ri'])) / np.median(times['moments_ri']))
    s = res['fit_ms'] * 1e-3
    res['fit_chain_TBps'] = chain_bytes / s / 1e12
    res['fit_frac_of_hbm_peak'] = chain_bytes / s / HBM_PEAK
    res['fit_evaluations_per_s'] = n * E * Wp * N_FREQ / s
    res['fit_over_moments_ri'] = res['fit_ms'] / res['moments_ri_ms']
    res['unfused_over_fit'] = res['unfused_ms'] / res['fit_ms']
    # the same numbers from both routes (torch's are another order of summation; q is far from 0 on this chain)
    torch.cuda.synchronize()
    fused, un = c.out.reshape(3, E, -1), c.un
    res['fused_vs_unfused_max_rel'] = [float(((fused[i] - un[i]).abs() / un[i].abs()).max()) for i in range(3)]
    batch.close()
    del x, c
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default=','.join(MODELS))
    ap.add_argument('--quick', action='store_true', help='the small shape')
    ap.add_argument('--repeats', type=int, default=5, help='rounds of the alternating calls (median)')
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fit_quality_bench needs a GPU')
    lines = []
    for model in args.models.split(','):
        lines.append(json.dumps(run(model, 'quick' if args.quick else 'full', args.repeats)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'fit_quality_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
