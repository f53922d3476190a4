#!/usr/bin/env python3
"""PSIS-LOO of device-resident chains (bisip_q_columns_dev + bisip_loo_columns_dev behind bisip_amd.loo.device_loo): the
Pareto-smoothed leave-one-out sum and the Pareto k of every data point of every spectrum.

Shape: the README's survey slice as response_bench.py and fit_quality_bench.py -- 512 spectra x 256 walkers x 500 used
samples of 1000 stored (discard = 0, thin = 2), N = 32 synthetic frequencies, for the double Cole-Cole model and
PolynomialDecomposition (degree 5); --quick: 16 spectra x 64 walkers x 50 of 100, for a machine that is shared.  The chain is
response_bench's.  In one process, wall time around each whole call with a device synchronisation before and after (the
calls copy their results to the host), two warm-up calls each, then --repeats (default 5) rounds in which the calls
alternate; the medians are reported, the repeats kept:
  * loo_ms: device_loo, spectra in passes under decomposition.RTD_PASS_BYTES -- per pass the copy of the rows,
    bisip_forward_columns_dev, bisip_q_columns_dev, bisip_loo_columns_dev; 2N columns of 128,000 values per spectrum;
  * model_percentile_ms: summaries.device_model_percentiles (2.5, 50, 97.5) on the same chain -- the same passes, copy and
    forward launch, then ONE selection per column where PSIS-LOO selects, compacts, sorts the tails and fits them;
  * hdi_ms: interval.device_hdi at mass 0.95 (bisip_chain_hdi_dev, the tails path) of the same chain's ndim parameter
    columns per spectrum: the nearest sibling of the compaction and the segmented sort, on 2N / ndim times fewer columns;
  * stages_ms: one pass of device_loo taken apart with device events: rows, forward, q, columns (the column pass whole).
--only NAME runs one call alone (for a kernel trace, where the share of k_loo_tail in the column pass is read).
Prints one JSON line per model; with --out DIR also writes them to DIR/loo_bench.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from response_bench import MODELS, N_FREQ, SHAPES, make_chain      # noqa: E402

P_BAND = (2.5, 50.0, 97.5)


def wall(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def stages(view, ctx):
    """One pass of device_loo (its first spectra), the four steps between device events: milliseconds each."""
    import torch
    from bisip_amd import _hip, decomposition, loo
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    rows_per, cols = n * Wp, 2 * ctx.N
    M = loo.tail_length(rows_per)
    k = int(min(E, max(1, decomposition.RTD_PASS_BYTES // (rows_per * cols * 8))))
    nbytes = _hip.loo_columns_workspace(rows_per, k * cols, M)
    work, qc = view.empty((nbytes,), torch.uint8), view.empty((k, cols, rows_per), torch.float64)
    res, cnt = view.empty((2, k * cols), torch.float64), view.empty((k * cols,), torch.int64)
    grid = view.samples().reshape(n, E, Wp, ndim)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    out = None
    for _ in range(2):                                                  # the second round is reported
        ev[0].record()
        rows = grid[:, :k].permute(1, 0, 2, 3).reshape(k, rows_per, ndim).contiguous()
        ev[1].record()
        ctx.forward_columns_dev(0, k, rows.data_ptr(), k * rows_per, qc.data_ptr(), view.stream)
        ev[2].record()
        ctx.q_columns_dev(0, k, qc.data_ptr(), rows_per, view.stream)
        ev[3].record()
        _hip.loo_columns_dev(qc.data_ptr(), rows_per, k * cols, M, res[0].data_ptr(), res[1].data_ptr(), 0, cnt.data_ptr(),
                             work.data_ptr(), nbytes, view.stream)
        ev[4].record()
        ev[4].synchronize()
        out = dict(zip(('rows', 'forward', 'q', 'columns'), (ev[i].elapsed_time(ev[i + 1]) for i in range(4))))
    out.update(spectra=k, tail_len=M, workspace_bytes=nbytes)
    return out


def run(model, shape, repeats, only=None):
    import torch
    import bisip_amd
    from bisip_amd import decomposition, interval, loo, summaries
    from bisip_amd.chainview import ChainView
    from bisip_amd.synthetic import synthetic_columns
    E, Wp, n, discard, thin = SHAPES[shape]
    batch = bisip_amd.SpectraBatch(model, [synthetic_columns(N_FREQ, i) for i in range(E)], nwalkers=Wp, nsteps=8, **MODELS[model])
    stored = discard + thin * n
    x = make_chain(model, *batch.param_bounds, stored, E * Wp)
    row = E * Wp * batch.ndim
    view = ChainView(x, n, E, Wp, batch.ndim, (discard + thin - 1) * row, thin * row)
    ctx = batch.ctx
    rows_per, cols = n * Wp, 2 * N_FREQ
    G = int(min(E, max(1, decomposition.RTD_PASS_BYTES // (rows_per * cols * 8))))
    res = dict(model=model, options=MODELS[model], shape=shape, E=E, Wp=Wp, N=N_FREQ, ndim=batch.ndim, samples=n, stored=stored,
               discard=discard, thin=thin, rows_per_spectrum=rows_per, columns=E * cols, column_bytes=8 * rows_per * E * cols,
               tail_len=loo.tail_length(rows_per), passes=-(-E // G), spectra_per_pass=G, repeats=repeats,
               hdi_path=interval.plan(n, E, Wp, batch.ndim, interval.windows(0.95, rows_per)))
    kept = {}
    calls = dict(loo=lambda: kept.__setitem__('loo', loo.device_loo(view, ctx)),
                 model_percentile=lambda: summaries.device_model_percentiles(view, ctx, P_BAND),
                 hdi=lambda: interval.device_hdi(view, 0.95))
    if only:
        calls = {only: calls[only]}
    for f in calls.values():
        f()
        f()
    times = {k: [] for k in calls}
    for _ in range(repeats):                                         # alternating on one box
        for k, f in calls.items():
            times[k].append(wall(f))
    for k, v in times.items():
        res[k + '_ms'], res[k + '_ms_repeats'] = float(np.median(v)), v
    if not only:
        res['loo_over_model_percentile'] = res['loo_ms'] / res['model_percentile_ms']
        res['loo_over_hdi'] = res['loo_ms'] / res['hdi_ms']
        res['stages_ms'] = stages(view, ctx)
    if 'loo' in kept:
        _, khat, n_tail = kept['loo']
        fin = np.isfinite(khat)
        res.update(smoothed_points=int(fin.sum()), points=int(khat.size), khat_median=float(np.median(khat[fin])) if fin.any() else None,
                   n_tail_min=int(n_tail.min()), n_tail_max=int(n_tail.max()))
    batch.close()
    del x, view
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default=','.join(MODELS))
    ap.add_argument('--quick', action='store_true', help='the small shape')
    ap.add_argument('--repeats', type=int, default=5, help='rounds of the alternating calls (median)')
    ap.add_argument('--only', choices=('loo', 'model_percentile', 'hdi'), help='one call alone')
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('loo_bench needs a GPU')
    lines = []
    for model in args.models.split(','):
        lines.append(json.dumps(run(model, 'quick' if args.quick else 'full', args.repeats, args.only)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'loo_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
