#!/usr/bin/env python3
"""The log marginal likelihood of device-resident chains by bridge sampling (bisip_bridge_logg_dev, _draw_dev, _scale_dev,
_iterate_dev and bisip_logprob_dev behind bisip_amd.evidence.device_evidence).

Shapes: the README's survey slice as loo_bench.py -- 512 spectra x 256 walkers x 500 used samples of 1000 stored (discard = 0,
thin = 2), N = 32 synthetic frequencies, for the double Cole-Cole model and PolynomialDecomposition (degree 5), N2 = N1 = 250
x 256 draws per spectrum -- and one model's 32 walkers x 5000 samples (double Cole-Cole, ndim 7); --quick: 16 spectra x 64
walkers x 50 of 100.  The chain is response_bench's (uniform in a part of the box: the times depend on the shape and on the
number of passes of the iteration, which is reported), its log-probability bisip_logprob_dev's.  In one process, wall time
around each whole call with a device synchronisation before and after, two warm-up calls each, then --repeats (default 5)
rounds in which the calls alternate; the medians are reported, the repeats kept:
  * evidence_ms: device_evidence end to end (neff = None: no ESS pass), the covariance of the first half and the host's
    Cholesky factors included;
  * logg_ms against cov_ms: bisip_bridge_logg_dev and bisip_chain_cov_dev on the same second half -- both read the chain once;
  * logprob_draws_ms against logprob_chain_ms: bisip_logprob_dev on the N2 draws per spectrum and on N2 rows per spectrum
    copied from the chain -- a share of the draws returns early outside the box (frac_outside);
  * draw_ms, scale_ms, median_ms (bisip_columns_percentiles_dev of l1), tau_ms (the copy and bisip_chain_autocorr_time_dev);
  * iterate_ms, iterations (the most passes of any spectrum: the workgroups run side by side) and iterate_ms_per_iteration;
  * fitted_evidence_ms: get_evidence (neff = None) of a chain the batch sampled itself in the same run -- FIT_BURN steps of
    burn-in from uniform starts, then the same used / stored samples -- with fitted_iterations, fitted_not_finite (spectra whose
    estimate is NaN), fitted_se_median and fitted_frac_outside: what the call costs where a normal proposal bridges the
    posterior, and whether it does.
Clocks are not read.  Prints one JSON line per model and shape; with --out DIR also appends them to DIR/evidence_bench.jsonl."""
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

ONE_MODEL = (1, 32, 5000, 0, 1)                                      # E, Wp, used samples, discard, thin
FIT_BURN = 2000                                                      # steps the fitted chain leaves behind before it is stored


def wall(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def run(model, shape, repeats):
    import torch
    import bisip_amd
    from bisip_amd import _hip, evidence as ev
    from bisip_amd.autocorr import device_integrated_time
    from bisip_amd.chainview import ChainView
    from bisip_amd.covariance import device_cov
    from bisip_amd.synthetic import synthetic_columns
    E, Wp, n, discard, thin = ONE_MODEL if shape == 'one_model' else SHAPES[shape]
    batch = bisip_amd.SpectraBatch(model, [synthetic_columns(N_FREQ, i) for i in range(E)], nwalkers=Wp, nsteps=8, **MODELS[model])
    ndim, ctx = batch.ndim, batch.ctx
    stored = discard + thin * n
    x = make_chain(model, *batch.param_bounds, stored, E * Wp)
    lp = torch.empty((stored, E * Wp), dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    for s in range(stored):                                          # (a sample is the batch row layout: rows e * Wp + w)
        ctx.logprob_dev(x[s].data_ptr(), E * Wp, lp[s].data_ptr(), st)
    torch.cuda.synchronize()
    row = E * Wp * ndim
    view = ChainView(x, n, E, Wp, ndim, (discard + thin - 1) * row, thin * row)
    lview = ChainView(lp, n, E, Wp, 1, (discard + thin - 1) * E * Wp, thin * E * Wp)
    n0, n1 = ev.halves(n, Wp, ndim)
    v1, lv1 = ev._tail_view(view, n0, n1), ev._tail_view(lview, n0, n1)
    N1 = N2 = n1 * Wp
    mean, cov = device_cov(ev._tail_view(view, 0, n0), mean=True)
    mu, L, c = ev.proposal_factor(mean, cov)
    d_mu, d_L, d_c = view.upload(mu), view.upload(L), view.upload(c)
    f64 = torch.float64
    l1, a1, a2, f2 = (view.empty((E, k), f64) for k in (N1, N2, N1, N1))
    logp2, logg2, lchain = view.empty((E, N2), f64), view.empty((E, N2), f64), view.empty((E, N2), f64)
    theta = view.empty((E * N2, ndim), f64)
    rows = view.samples()[n0:].reshape(n1, E, Wp, ndim).permute(1, 0, 2, 3).reshape(E * N1, ndim).contiguous()
    lstar, d_s1 = view.empty((1, E), f64), view.upload(np.full(E, 0.5))
    r, its, mom = view.empty((E,), f64), view.empty((E,), torch.int64), view.empty((E, 4), f64)
    covw = _hip.chain_cov_workspace(n1, E, Wp, ndim)
    cwork, dcov = view.empty((max(covw, 1),), torch.uint8), view.empty((E, ndim, ndim), f64)
    kept = {}

    def tau():
        series = f2.view(E, n1, Wp).permute(1, 0, 2).contiguous()
        device_integrated_time(ChainView(series, n1, E, Wp, 1), 5)

    calls = dict(
        evidence=lambda: kept.__setitem__('res', ev.device_evidence(view, lview, ctx, neff=None)),
        logg=lambda: _hip.bridge_logg_dev(v1.ptr, n1, v1.stride, E, Wp, ndim, lv1.ptr, lv1.stride, d_mu.data_ptr(), d_L.data_ptr(),
                                          d_c.data_ptr(), l1.data_ptr(), st),
        cov=lambda: _hip.chain_cov_dev(v1.ptr, n1, v1.stride, E, Wp, ndim, 0, dcov.data_ptr(), cwork.data_ptr() if covw else 0,
                                       covw, st),
        draw=lambda: _hip.bridge_draw_dev(d_mu.data_ptr(), d_L.data_ptr(), d_c.data_ptr(), E, ndim, N2, 0, 0, 0, theta.data_ptr(),
                                          logg2.data_ptr(), st),
        logprob_draws=lambda: ctx.logprob_dev(theta.data_ptr(), E * N2, logp2.data_ptr(), st),
        logprob_chain=lambda: ctx.logprob_dev(rows.data_ptr(), E * N1, lchain.data_ptr(), st),
        median=lambda: _hip.columns_percentiles_dev(l1.data_ptr(), E, N1, (50.0,), lstar.data_ptr(), st),
        scale=lambda: _hip.bridge_scale_dev(l1.data_ptr(), N1, logp2.data_ptr(), logg2.data_ptr(), N2, E, lstar.data_ptr(), 0,
                                            a1.data_ptr(), a2.data_ptr(), st),
        iterate=lambda: _hip.bridge_iterate_dev(a1.data_ptr(), N2, a2.data_ptr(), N1, E, d_s1.data_ptr(), ev.TOL, ev.MAXITER,
                                                r.data_ptr(), its.data_ptr(), mom.data_ptr(), f2.data_ptr(), st),
        tau=tau)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                # (a uniform chain: the iteration may stop at maxiter)
        for f in calls.values():                                       # (in this order: each stage has its inputs)
            f()
            f()
        times = {k: [] for k in calls}
        for _ in range(repeats):                                       # alternating on one box
            for k, f in calls.items():
                times[k].append(wall(f))
    res = dict(model=model, options=MODELS[model], shape=shape, E=E, Wp=Wp, N=N_FREQ, ndim=ndim, samples=n, stored=stored,
               discard=discard, thin=thin, n1=N1, n2=N2, chain_bytes_second_half=8 * E * N1 * ndim, repeats=repeats)
    for k, v in times.items():
        res[k + '_ms'], res[k + '_ms_repeats'] = float(np.median(v)), v
    it = its.cpu().numpy()
    res.update(logg_over_cov=res['logg_ms'] / res['cov_ms'], logprob_draws_over_chain=res['logprob_draws_ms'] / res['logprob_chain_ms'],
               iterations=int(it.max()), iterations_median=float(np.median(it)),
               iterate_ms_per_iteration=res['iterate_ms'] / (int(it.max()) + 2),     # (+ the two passes of the moments)
               frac_outside=float(torch.isneginf(logp2).double().mean()),
               evidence_iterations=int(np.max(kept['res']['iterations'])), clocks_read=False)
    del x, lp, view, lview, v1, lv1, rows, theta, l1, a1, a2, f2, logp2, logg2, lchain
    torch.cuda.empty_cache()
    # the same shape of a chain the batch sampled itself: FIT_BURN steps of burn-in, then `stored` steps of which n are used
    batch.nsteps = FIT_BURN + stored
    np.random.seed(7)
    batch.fit(seed=7, chain='device')
    fitted = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        get = lambda: fitted.__setitem__('res', batch.get_evidence(discard=FIT_BURN + discard, thin=thin, neff=None))
        get()
        get()
        t = [wall(get) for _ in range(repeats)]
    fit_it = fitted['res']['iterations']
    res.update(fitted_burn=FIT_BURN, fitted_evidence_ms=float(np.median(t)), fitted_evidence_ms_repeats=t,
               fitted_iterations=int(fit_it.max()), fitted_iterations_median=float(np.median(fit_it)),
               fitted_not_finite=int((~np.isfinite(fitted['res']['log_ml'])).sum()),
               fitted_se_median=float(np.nanmedian(fitted['res']['se'])),
               fitted_frac_outside=float(np.mean(fitted['res']['frac_outside'])))
    batch.close()
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
        raise SystemExit('evidence_bench needs a GPU')
    lines = []
    for model in args.models.split(','):
        lines.append(json.dumps(run(model, 'quick' if args.quick else 'full', args.repeats)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(run('PeltonColeCole', 'one_model', args.repeats)))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'evidence_bench.jsonl'), 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
