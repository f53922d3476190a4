#!/usr/bin/env python3
"""Posterior predictive checks of device-resident chains (bisip_predictive_check_dev): per data point the mean of
Phi((y - Z) / sigma), per spectrum the means of the chi-square T, of P(chi2_2N >= T) and of the probability of the largest
standardised residual, and the histogram of the residual's sign changes along the frequency axis.

Shape: the README's survey slice as fit_quality_bench.py -- 512 spectra x 256 walkers x 500 used samples of 1000 stored
(discard = 0, thin = 2), N = 32 synthetic frequencies, for the double Cole-Cole model and PolynomialDecomposition (degree
5); --quick: 16 spectra x 64 walkers x 50 of 100, for a machine that is shared.  The chain is response_bench's.  In one
process, device events around each whole call, two warm-up calls each, then --repeats (default 5) rounds in which the
calls alternate; the medians are reported, the repeats kept:
  * predictive_ms: the new call, all spectra, the three outputs (the row pass and the point pass); chain bytes over the
    time and model evaluations (2 x rows x N: either pass evaluates the model) per second; predictive_rows_ms and
    predictive_pit_ms: the same call asked for the row outputs alone (one pass) and for pit alone (both);
  * fit_ms: bisip_fit_quality_dev on the same chain -- one exp per row and point and four states where the point pass has
    one erfc and one state; predictive_over_fit;
  * unfused_ms: what Python allows without the kernel -- per pass (spectra under decomposition.RTD_PASS_BYTES) the copy of
    the rows, forward_columns_dev into Re / Im columns, torch elementwise ops, torch.special.erfc and torch.mean for pit,
    and the per-row sums, torch.special.gammaincc and the histogram in torch; unfused_over_predictive.
spread: (max - min) / median of the five repeats of each call.  Prints one JSON line per model; with --out DIR also writes
them to DIR/predictive_bench.jsonl."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fit_quality_bench import timed                                 # noqa: E402
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
        # two buffers of columns (the residuals and what is made of them) under the cap of one pass
        self.G = G = int(min(E, max(1, decomposition.RTD_PASS_BYTES // (2 * self.rows_per * cols * 8))))

        def empty(*shape, dtype=torch.float64):
            return torch.empty(shape, dtype=dtype, device=x.device)

        self.rows, self.cols, self.tmp = empty(G, n, Wp, batch.ndim), empty(G, cols, self.rows_per), empty(G, cols, self.rows_per)
        iv = fitquality.inverse_variance(batch.zn_err).reshape(E, cols, 1)
        self.y = torch.from_numpy(batch.zn.reshape(E, cols, 1)).to(x.device)
        self.iv = torch.from_numpy(iv).to(x.device)
        self.h = torch.from_numpy(np.sqrt(0.5 * iv)).to(x.device)
        self.pit, self.row, self.hist = empty(E, 2, batch.N), empty(E, 3), empty(E, cols - 1, dtype=torch.int64)
        self.un_pit, self.un_row, self.un_hist = empty(E, cols), empty(E, 3), empty(E, cols - 1, dtype=torch.int64)
        self.fit_out = empty(3, E, 2, batch.N)
        self.pbytes = self.ctx.predictive_check_workspace(n, E, Wp)
        self.fbytes = self.ctx.fit_quality_workspace(n, E, Wp)
        self.work = torch.empty((max(1, self.pbytes, self.fbytes),), dtype=torch.uint8, device=x.device)
        self.bin0 = (torch.arange(G, device=x.device) * (cols - 1)).reshape(G, 1)

    def _predictive(self, pit, row, hist):
        self.ctx.predictive_check_dev(0, self.E, self.ptr, self.n, self.stride, self.Wp, pit, row, hist, self.work.data_ptr(),
                                      self.pbytes, self.st)

    def predictive(self):
        self._predictive(self.pit.data_ptr(), self.row.data_ptr(), self.hist.data_ptr())

    def predictive_rows(self):
        self._predictive(0, self.row.data_ptr(), self.hist.data_ptr())

    def predictive_pit(self):
        self._predictive(self.pit.data_ptr(), 0, 0)

    def fit(self):
        self.ctx.fit_quality_dev(0, self.E, self.ptr, self.n, self.stride, self.Wp, self.fit_out[0].data_ptr(),
                                 self.fit_out[1].data_ptr(), self.fit_out[2].data_ptr(), self.work.data_ptr(), self.fbytes, self.st)

    def unfused(self):
        torch, N = self.torch, self.N
        for g0 in range(0, self.E, self.G):
            k = min(self.E, g0 + self.G) - g0
            self.rows[:k].copy_(self.grid[:, g0:g0 + k].permute(1, 0, 2, 3))        # spectrum-major, as the summaries do
            self.ctx.forward_columns_dev(g0, k, self.rows.data_ptr(), k * self.rows_per, self.cols.data_ptr(), self.st)
            d, t = self.cols[:k], self.tmp[:k]
            torch.sub(self.y[g0:g0 + k], d, out=d)
            torch.mul(d, self.h[g0:g0 + k], out=t)
            torch.special.erfc(t.neg_(), out=t)
            torch.mean(t, dim=-1, out=self.un_pit[g0:g0 + k])
            neg = (d < 0).reshape(k, 2, N, self.rows_per)
            C = (neg[:, :, 1:] != neg[:, :, :-1]).sum(dim=(1, 2))                   # (k, rows)
            bins = torch.bincount((C + self.bin0[:k]).reshape(-1), minlength=k * (2 * N - 1))
            self.un_hist[g0:g0 + k] = bins.reshape(k, 2 * N - 1)
            d.mul_(d).mul_(self.iv[g0:g0 + k])                                      # q
            T, qmax = d.sum(dim=1), d.amax(dim=1)
            self.un_row[g0:g0 + k, 0] = T.mean(dim=-1)
            self.un_row[g0:g0 + k, 1] = torch.special.gammaincc(torch.full_like(T, float(N)), T.mul_(0.5)).mean(dim=-1)
            e = torch.special.erfc(qmax.mul_(0.5).sqrt_())
            self.un_row[g0:g0 + k, 2] = torch.expm1(torch.log1p(e.neg_()).mul_(2.0 * N)).neg_().mean(dim=-1)
        self.un_pit.mul_(0.5)


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
               spectra_per_pass=c.G, segments=nseg, segment_rows=seg_rows, predictive_workspace_bytes=c.pbytes, repeats=repeats)
    calls = dict(predictive=c.predictive, fit=c.fit, unfused=c.unfused, predictive_rows=c.predictive_rows,
                 predictive_pit=c.predictive_pit)
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
        res[k + '_spread'] = float((max(v) - min(v)) / np.median(v))
    s = res['predictive_ms'] * 1e-3
    res['predictive_chain_TBps'] = 2 * chain_bytes / s / 1e12
    res['predictive_frac_of_hbm_peak'] = 2 * chain_bytes / s / HBM_PEAK
    res['predictive_evaluations_per_s'] = 2 * n * E * Wp * N_FREQ / s
    res['predictive_over_fit'] = res['predictive_ms'] / res['fit_ms']
    res['unfused_over_predictive'] = res['unfused_ms'] / res['predictive_ms']
    # faster than the unfused route by more than the spread of the repeats: the slowest fused call against the fastest unfused
    res['faster_than_unfused_beyond_spread'] = bool(max(times['predictive']) < min(times['unfused']))
    # the same numbers from both routes (torch's are another order of summation and other functions)
    c.predictive()
    c.unfused()
    torch.cuda.synchronize()
    res['fused_vs_unfused_pit_max_abs'] = float((c.pit.reshape(E, -1) - c.un_pit).abs().max())
    res['fused_vs_unfused_row_max_abs'] = [float((c.row[:, i] - c.un_row[:, i]).abs().max()) for i in range(3)]
    res['fused_vs_unfused_chi2_mean_max_rel'] = float(((c.row[:, 0] - c.un_row[:, 0]).abs() / c.un_row[:, 0].abs()).max())
    res['histograms_equal'] = bool((c.hist == c.un_hist).all())
    res['rows_counted'] = int(c.hist.sum())
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
        raise SystemExit('predictive_bench needs a GPU')
    lines = []
    for model in args.models.split(','):
        lines.append(json.dumps(run(model, 'quick' if args.quick else 'full', args.repeats)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'predictive_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
