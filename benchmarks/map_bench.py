#!/usr/bin/env python3
"""The multi-start Levenberg-Marquardt MAP fit on the device (bisip_map_fit_dev) beside the same loop driven from the host,
and what it buys: the burn-in a fit saves when it starts from the optimum, and the Laplace evidence beside bridge sampling.

Speed.  512 synthetic spectra (bisip_amd.synthetic) x 32 uniform starts, N = 32, a double Cole-Cole model and a
PolynomialDecomposition of degree 5; medians of 5 with the calls alternating, and the spread (min, max) of the five:
  * fused_ms: bisip_map_fit_dev, every spectrum and start in one launch (device-event time), max_iter = 60, pred_tol = 1e-8;
  * unfused_s_per_spectrum: mapfit.lm_fit around a single-spectrum context's forward -- one forward launch per stencil and
    per round of candidates, the dense steps in NumPy -- on the first ``--host-subset`` spectra (wall time), and the ratio
    of the two per spectrum;
  * evals_per_s: model evaluations of bisip_map_fit_dev per second -- a start makes (iterations + 1) stencil passes of
    2 ndim + 1 evaluations and one candidate pass of 12 evaluations per iteration (one more when it stalled) -- beside
    logprob_rows_per_s, bisip_logprob_dev on as many rows.
    Expectation, written down before the measurement: with one start per wave only 2 ndim + 1 (stencil pass) or 12
    (candidate pass) of 64 lanes evaluate the model, so the rate should be about (2 ndim + 1) / 64 of the bulk rate (0.23 for
    ndim = 7) if the model evaluations were all a wave did; the dense step in single lanes, the cross-lane exchange and the
    sums of A (ndim products per lane and frequency) come on top.  The measured ratio stands beside the expected one.

Burn-in.  The step at which the per-step median log-probability over the walkers (get_log_prob_trace) first comes within
ndim of its final plateau (the median of the trace's last quarter), for p0=None against p0='map': on the bundled two-mode
Cole-Cole fit (SIP-K389174, 32 walkers) and on a survey of synthetic spectra (SpectraBatch, median over the spectra).

Evidence.  log_evidence_laplace of fit_map beside get_evidence (bridge sampling) on the PolynomialDecomposition fit of
SIP-K389175.

Prints one JSON line per result; with --out DIR also writes them to DIR/map_bench.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {'double_cole_cole': ('PeltonColeCole', dict(n_modes=2)), 'polydecomp_deg5': ('PolynomialDecomposition', dict(poly_deg=5))}
CANDIDATES = 12


def survey(model, kw, E, n_freq, nwalkers=32, nsteps=8):
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    return bisip_amd.SpectraBatch(model, [synthetic_columns(n_freq, i) for i in range(E)], nwalkers=nwalkers, nsteps=nsteps, **kw)


def single_context(b, e):
    from bisip_amd import _hip
    from bisip_amd.batch import _MODELS
    kw = {}
    if b.model == 'PolynomialDecomposition':
        kw = dict(poly_deg=b.poly_deg, c_exp=b.c_exp, taus=b.taus, log_taus=b.log_taus)
    if b.model == 'PeltonColeCole':
        kw = dict(n_modes=b.n_modes)
    return _hip.HipContext(_MODELS[b.model], b.w[e], b.zn[e], b.zn_err[e], b.param_bounds, **kw)


def speed(name, E, S, n_freq, subset, reps=5):
    import torch
    from bisip_amd import mapfit as mf
    from bisip_amd.fitquality import inverse_variance
    model, kw = MODELS[name]
    b = survey(model, kw, E, n_freq)
    n = b.ndim
    starts = mf.uniform_starts(b.param_bounds, (E, S), seed=7)
    d_starts = torch.from_numpy(starts).cuda()
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device='cuda')
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device='cuda')
    out = dict(theta=f64(E, S, n), chi2=f64(E, S), logp=f64(E, S), pred=f64(E, S), A=f64(E, S, n, n), it=i64(E, S), st=i64(E, S))
    stream = torch.cuda.current_stream().cuda_stream

    def fused():
        b.ctx.map_fit_dev(0, E, d_starts.data_ptr(), S, 60, 1e-8, *[out[k].data_ptr() for k in ('theta', 'chi2', 'logp', 'pred', 'A', 'it', 'st')],
                          stream)

    fused()
    torch.cuda.synchronize()
    it, st = out['it'].cpu().numpy(), out['st'].cpu().numpy()
    stencil_evals = int(((it + 1) * (2 * n + 1)).sum())
    candidate_evals = int(((it + (st == 1)) * CANDIDATES).sum())
    evals = stencil_evals + candidate_evals
    # bisip_logprob_dev on as many rows (a multiple of E), uniform in the box
    rows = -(-evals // E) * E
    d_rows = torch.from_numpy(mf.uniform_starts(b.param_bounds, (rows,), seed=8)).cuda()
    d_lp = f64(rows)

    def logprob():
        b.ctx.logprob_dev(d_rows.data_ptr(), rows, d_lp.data_ptr(), stream)

    def device_ms(f):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        z.record()
        z.synchronize()
        return a.elapsed_time(z)

    k = min(E, subset)
    ctxs = [single_context(b, e) for e in range(k)]
    ivs = [inverse_variance(b.zn_err[e]) for e in range(k)]

    def unfused():
        t0 = time.perf_counter()
        res = [mf.lm_fit(ctxs[e].forward, b.zn[e], ivs[e], b.param_bounds, starts[e], 60, 1e-8) for e in range(k)]
        return (time.perf_counter() - t0) / k, res

    logprob()
    _, host = unfused()
    torch.cuda.synchronize()
    t_f, t_l, t_u = [], [], []
    for _ in range(reps):
        t_f.append(device_ms(fused))
        t_l.append(device_ms(logprob))
        t_u.append(unfused()[0])
    med = lambda ts: float(np.median(ts))
    spread = lambda ts: [float(min(ts)), float(max(ts))]
    chi2 = out['chi2'].cpu().numpy()
    best_dev = chi2[:k].min(axis=1)
    best_host = np.array([r['chi2'].min() for r in host])
    rate, bulk = evals / (med(t_f) * 1e-3), rows / (med(t_l) * 1e-3)
    res = dict(bench='speed', model=name, E=E, S=S, N=n_freq, ndim=n, reps=reps, max_iter=60, pred_tol=1e-8,
               fused_ms=med(t_f), fused_ms_spread=spread(t_f), fused_us_per_spectrum=med(t_f) * 1e3 / E,
               unfused_s_per_spectrum=med(t_u), unfused_s_per_spectrum_spread=spread(t_u), unfused_spectra=k,
               fused_over_unfused_per_spectrum=med(t_u) / (med(t_f) * 1e-3 / E),
               best_chi2_max_abs_difference_on_subset=float(np.max(np.abs(best_dev - best_host))),
               median_iterations=float(np.median(it)), status_counts=[int((st == s).sum()) for s in (0, 1, 2)],
               starts_agreeing_median=float(np.median((chi2 <= chi2.min(axis=1, keepdims=True) + 1e-6).sum(axis=1))),
               model_evaluations=evals, stencil_evaluations=stencil_evals, candidate_evaluations=candidate_evals,
               evals_per_s=rate, logprob_rows=rows, logprob_ms=med(t_l), logprob_ms_spread=spread(t_l), logprob_rows_per_s=bulk,
               rate_ratio=rate / bulk, rate_ratio_expected=(2 * n + 1) / 64)
    for c in ctxs:
        c.close()
    b.close()
    return res


def burn_in_step(trace, ndim):
    """The first step whose median log-probability is within ndim of the plateau (the median of the trace's last quarter);
    trace (n,) or (n, E) -> int or (E,)."""
    trace = np.asarray(trace)
    plateau = np.median(trace[-max(1, trace.shape[0] // 4):], axis=0)
    ok = trace >= plateau - ndim
    return np.argmax(ok, axis=0)


def burn_in_lone(nsteps):
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389174']
    res = dict(bench='burn_in', fit='PeltonColeCole n_modes=2 on SIP-K389174', nwalkers=32, nsteps=nsteps)
    for p0 in (None, 'map'):
        m = bisip_amd.PeltonColeCole(path, n_modes=2, nwalkers=32, nsteps=nsteps)
        np.random.seed(1)
        t0 = time.perf_counter()
        m.fit(p0=p0, chain='device')
        res[f'fit_s_{p0}'] = time.perf_counter() - t0
        trace = m.get_log_prob_trace(50.0)
        res[f'burn_in_step_{p0}'] = int(burn_in_step(trace, m.ndim))
        res[f'plateau_{p0}'] = float(np.median(trace[-nsteps // 4:]))
        if p0 == 'map':
            res['logp_map'] = m.get_map()['logp']
            res['n_agree'] = m.get_map()['n_agree']
    return res


def burn_in_survey(E, nsteps, n_freq=32):
    res = dict(bench='burn_in', fit=f'SpectraBatch of {E} synthetic double Cole-Cole spectra', nwalkers=64, nsteps=nsteps)
    for p0 in (None, 'map'):
        b = survey('PeltonColeCole', dict(n_modes=2), E, n_freq, nwalkers=64, nsteps=nsteps)
        np.random.seed(1)
        t0 = time.perf_counter()
        b.fit(p0=p0, seed=3, chain='device')
        res[f'fit_s_{p0}'] = time.perf_counter() - t0
        steps = burn_in_step(b.get_log_prob_trace(50.0), b.ndim)
        res[f'burn_in_step_median_{p0}'] = float(np.median(steps))
        res[f'burn_in_step_max_{p0}'] = int(steps.max())
        b.close()
    return res


def evidence(nsteps=4000, discard=1000):
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389175']
    m = bisip_amd.PolynomialDecomposition(path, nwalkers=32, nsteps=nsteps)
    np.random.seed(2)
    m.fit(p0='map', chain='device')
    best = m.get_map()
    ev = m.get_evidence(discard=discard)
    return dict(bench='evidence', fit='PolynomialDecomposition degree 5 on SIP-K389175', nsteps=nsteps, discard=discard,
                log_evidence_laplace=best['log_evidence_laplace'], log_evidence_bridge=float(ev['log_evidence']),
                bridge_se=float(ev['se']), difference=best['log_evidence_laplace'] - float(ev['log_evidence']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spectra', type=int, default=512)
    ap.add_argument('--starts', type=int, default=32)
    ap.add_argument('--n-freq', type=int, default=32)
    ap.add_argument('--host-subset', type=int, default=8, help='spectra the unfused loop times')
    ap.add_argument('--survey-spectra', type=int, default=64)
    ap.add_argument('--nsteps', type=int, default=2000)
    ap.add_argument('--only', default='speed,burn_in,evidence')
    ap.add_argument('--out', help='directory for the JSON lines (default: stdout only)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('map_bench needs a GPU')
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    only = args.only.split(',')
    if 'speed' in only:
        for name in MODELS:
            emit(speed(name, args.spectra, args.starts, args.n_freq, args.host_subset))
    if 'burn_in' in only:
        emit(burn_in_lone(args.nsteps))
        emit(burn_in_survey(args.survey_spectra, args.nsteps))
    if 'evidence' in only:
        emit(evidence())
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'map_bench.jsonl'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
