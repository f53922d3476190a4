#!/usr/bin/env python3
"""Amplitude / phase bands and response moments of device-resident chains (bisip_forward_columns_kind_dev +
bisip_columns_percentiles_dev, bisip_response_moments_dev).

Shape: the README's survey slice, 512 spectra x 256 walkers x 500 used samples of 1000 stored (discard = 0, thin = 2),
N = 32 synthetic frequencies, for the double Cole-Cole model and PolynomialDecomposition (degree 5); --quick: 16 spectra x
64 walkers x 50 of 100, for a machine that is shared.  The chain is uniform in the part of the prior box where Re Z > 0,
made on the device.  Spectra go in passes under decomposition.RTD_PASS_BYTES as in summaries.device_model_percentiles;
every buffer is allocated once.  In one process, device events around each whole call after two warm-up calls:
  * pa_ms: the PA percentiles -- per pass the copy of the rows, ONE forward launch that writes amplitude / phase columns,
    the selection;
  * pa_baseline_ms: what the parent commit allows from Python -- forward_columns_dev into Re / Im columns, torch.atan2 /
    torch.hypot / torch.neg in place on the two halves (one half-size temporary), the same selection.  The two are timed
    alternately --repeats times (default 5); pa_spread is (max - min) / median of the baseline's repeats;
  * ri_ms: plain get_model_percentile's passes on the same chain, and pa_over_ri;
  * moments_ri_ms, moments_pa_ms: the fused kernel, all spectra in one launch; chain bytes n * E * Wp * ndim * 8 over the
    time, and model evaluations (rows x N) per second;
  * moments_columns_ms: forward_columns_dev + torch.mean / torch.std over the columns in the same passes (Re / Im);
  * chain_moments_ms: bisip_chain_moments_dev on the same chain, for context (it evaluates no model).
Where the fused kernel's time goes (evaluation or reduction) is read from a kernel trace and a counter run of this
script with --only moments, each in a run of its own.  Prints one JSON line per model; with --out DIR also writes them."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_bench import HBM_PEAK, time_call      # noqa: E402

P = np.array([2.5, 50.0, 97.5])
N_FREQ = 32
MODELS = {'PeltonColeCole': dict(n_modes=2), 'PolynomialDecomposition': dict(poly_deg=5)}
SHAPES = {'full': (512, 256, 500, 0, 2), 'quick': (16, 64, 50, 0, 2)}      # E, Wp, used samples, discard, thin


def sub_box(model, lo, hi):
    """The part of the prior box the chain is drawn from: Re Z > 0 everywhere in it."""
    a, b = lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)
    if model == 'PolynomialDecomposition':
        scale = 0.005 * 6.0 ** -np.arange(lo.size - 1)
        a[1:], b[1:] = np.maximum(a[1:], -scale), np.minimum(b[1:], scale)
    else:
        D = (lo.size - 1) // 3
        b[1:1 + D] = 0.9 / D
    return a, b


def make_chain(model, lo, hi, stored, W):
    import torch
    g = torch.Generator(device='cuda').manual_seed(3)
    a, b = (torch.from_numpy(v).cuda() for v in sub_box(model, lo.copy(), hi.copy()))
    x = torch.empty((stored, W, lo.size), dtype=torch.float64, device='cuda')
    step = max(1, (1 << 26) // (W * lo.size))
    for s0 in range(0, stored, step):
        k = min(step, stored - s0)
        x[s0:s0 + k] = a + (b - a) * torch.rand((k, W, lo.size), generator=g, dtype=torch.float64, device='cuda')
    return x


class Calls:
    def __init__(self, batch, x, E, Wp, n, discard, thin):
        import torch
        from bisip_amd import _hip, decomposition
        self.hip, self.ctx, self.torch = _hip, batch.ctx, torch
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
        self.tmp = empty(G, batch.N, self.rows_per)
        self.pct = empty(E // G + 1, len(P), G * cols)
        self.cm, self.cs = empty(E, cols), empty(E, cols)
        self.mean, self.std = empty(E, 2, batch.N), empty(E, 2, batch.N)
        self.pmean, self.pstd = empty(E, batch.ndim), empty(E, batch.ndim)
        self.wbytes = self.ctx.response_moments_workspace(n, E, Wp)
        self.work = torch.empty((max(1, self.wbytes),), dtype=torch.uint8, device=x.device)
        self.mwork = empty(max(1, _hip.chain_moments_workspace(n, E, batch.ndim)))

    def passes(self):
        for i, g0 in enumerate(range(0, self.E, self.G)):
            k = min(self.E, g0 + self.G) - g0
            self.rows[:k].copy_(self.grid[:, g0:g0 + k].permute(1, 0, 2, 3))        # spectrum-major, as the summaries do
            yield i, g0, k

    def select(self, i, k):
        self.hip.columns_percentiles_dev(self.cols.data_ptr(), k * 2 * self.N, self.rows_per, P, self.pct[i].data_ptr(), self.st)

    def pa(self):
        for i, g0, k in self.passes():
            self.ctx.forward_columns_kind_dev(g0, k, self.rows.data_ptr(), k * self.rows_per, self.cols.data_ptr(), 'pa', self.st)
            self.select(i, k)

    def pa_baseline(self):
        torch, N = self.torch, self.N
        for i, g0, k in self.passes():
            self.ctx.forward_columns_dev(g0, k, self.rows.data_ptr(), k * self.rows_per, self.cols.data_ptr(), self.st)
            c = self.cols[:k]
            re, im, tmp = c[:, :N], c[:, N:], self.tmp[:k]
            torch.atan2(im, re, out=tmp)
            torch.hypot(re, im, out=re)
            torch.neg(tmp, out=im)
            self.select(i, k)

    def ri(self):
        for i, g0, k in self.passes():
            self.ctx.forward_columns_dev(g0, k, self.rows.data_ptr(), k * self.rows_per, self.cols.data_ptr(), self.st)
            self.select(i, k)

    def moments_columns(self):
        torch = self.torch
        for i, g0, k in self.passes():
            self.ctx.forward_columns_dev(g0, k, self.rows.data_ptr(), k * self.rows_per, self.cols.data_ptr(), self.st)
            torch.mean(self.cols[:k], dim=-1, out=self.cm[g0:g0 + k])
            torch.std(self.cols[:k], dim=-1, correction=0, out=self.cs[g0:g0 + k])

    def moments(self, kind):
        self.ctx.response_moments_dev(0, self.E, self.ptr, self.n, self.stride, self.Wp, kind, self.mean.data_ptr(),
                                      self.std.data_ptr(), self.work.data_ptr(), self.wbytes, self.st)

    def moments_ri(self):
        self.moments('ri')

    def moments_pa(self):
        self.moments('pa')

    def chain_moments(self):
        self.hip.chain_moments_dev(self.ptr, self.n, self.stride, self.E, self.Wp, self.ndim, self.pmean.data_ptr(),
                                   self.pstd.data_ptr(), self.mwork.data_ptr(), self.st)


def run(model, shape, reps, repeats, only):
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
               spectra_per_pass=c.G, moments_segments=nseg, moments_segment_rows=seg_rows, moments_workspace_bytes=c.wbytes,
               reps=reps, repeats=repeats)
    if only in ('all', 'percentiles'):
        a, b = [], []
        for _ in range(repeats):                                     # alternating A / B on one box
            a.append(time_call(c.pa, reps)[1])
            b.append(time_call(c.pa_baseline, reps)[1])
        res['pa_ms'], res['pa_baseline_ms'] = float(np.median(a)), float(np.median(b))
        res['pa_ms_repeats'], res['pa_baseline_ms_repeats'] = a, b
        res['pa_spread'] = float((max(b) - min(b)) / np.median(b))
        res['pa_over_baseline'] = res['pa_ms'] / res['pa_baseline_ms']
        res['ri_ms'] = time_call(c.ri, reps)[1]
        res['pa_over_ri'] = res['pa_ms'] / res['ri_ms']
    if only in ('all', 'moments'):
        for key in ('moments_ri', 'moments_pa', 'moments_columns', 'chain_moments'):
            best, med = time_call(getattr(c, key), reps)
            res[key + '_ms'], res[key + '_ms_best'] = med, best
        for key in ('moments_ri', 'moments_pa'):
            s = res[key + '_ms'] * 1e-3
            res[key + '_chain_TBps'] = chain_bytes / s / 1e12
            res[key + '_frac_of_hbm_peak'] = chain_bytes / s / HBM_PEAK
            res[key + '_evaluations_per_s'] = n * E * Wp * N_FREQ / s
        res['columns_over_fused_ri'] = res['moments_columns_ms'] / res['moments_ri_ms']
        # same numbers from both paths (the columns' moments are torch's: another order of summation)
        c.moments_ri()
        c.moments_columns()
        torch.cuda.synchronize()
        res['fused_vs_columns_max_rel'] = float(((c.mean.reshape(E, -1) - c.cm).abs() / c.cm.abs()).max())
    batch.close()
    del x, c
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default=','.join(MODELS))
    ap.add_argument('--quick', action='store_true', help='the small shape')
    ap.add_argument('--reps', type=int, default=5, help='timed calls per measurement (median)')
    ap.add_argument('--repeats', type=int, default=5, help='alternating repeats of the PA path and its baseline')
    ap.add_argument('--only', default='all', choices=('all', 'percentiles', 'moments'))
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('response_bench needs a GPU')
    lines = []
    for model in args.models.split(','):
        lines.append(json.dumps(run(model, 'quick' if args.quick else 'full', args.reps, args.repeats, args.only)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'response_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
