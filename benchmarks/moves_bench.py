#!/usr/bin/env python3
"""The differential-evolution and snooker moves of the device sampler (bisip_move_run_dev) beside the stretch move.

Speed, on the launch-per-half-step path, at the survey (512 spectra x 256 walkers, double Cole-Cole, 32 frequencies) and
at one ensemble of 4,096 walkers (single Cole-Cole): microseconds per half-step of ``run_mcmc(None, n)`` -- draw kernels,
enqueue and the half-step launches of a warm sampler, samples kept on the device -- under 'de', 'snooker' and the
0.8 / 0.2 mixture, against the stretch move (``moves=None, persistent=False``) in the same run; medians of --reps (5)
with the calls alternating, and each ratio to the stretch move.

Mixing, on the two-mode label-switching fit of tests/test_gpu_modes.py (20 frequencies, 32 walkers started near the truth,
the odd ones with the two modes exchanged): the integrated autocorrelation time of ``log_tau_1`` (emcee's estimate,
quiet) and the mode switch rate under the stretch move and under the mixture.  A finding to record, not a claim.

Prints one JSON line per measurement and writes them to profiles/moves_bench.jsonl (--out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXTURE = [('de', 0.8), ('snooker', 0.2)]
CONFIGS = (('stretch', None), ('de', 'de'), ('snooker', 'snooker'), ('mixture', MIXTURE))
TRUTH = np.array([1.0, 0.15, 0.5, -1.5, -12.0, 0.45, 0.6])       # of bisip_amd.synthetic, two modes
SWAP = [0, 2, 1, 4, 3, 6, 5]


def speed(label, ctx, Wp, E, ndim, bounds, steps, warm, reps):
    from bisip_amd.sampler import DeviceEnsembleSampler
    lo, hi = bounds
    p0 = np.random.RandomState(1).uniform(lo + 0.3 * (hi - lo), hi - 0.3 * (hi - lo), (E * Wp, ndim))
    samplers = {}
    for name, moves in CONFIGS:
        s = DeviceEnsembleSampler(Wp, ndim, ctx, rng='philox', seed=7, n_ensembles=E, persistent=False, moves=moves,
                                  chain_on_device=True)
        s.run_mcmc(p0, warm)
        assert s.last_path == 'launch-per-half-step', s.last_path
        samplers[name] = s
    times = {name: [] for name in samplers}
    for _ in range(reps):
        for name, s in samplers.items():             # alternating: a drift of the clocks lands on every configuration
            s.reset()
            t0 = time.perf_counter()
            s.run_mcmc(None, steps)
            times[name].append((time.perf_counter() - t0) / (2 * steps) * 1e6)
    out = dict(bench='moves_speed', shape=label, spectra=E, walkers=Wp, ndim=ndim, steps=steps, reps=reps)
    for name in samplers:
        out[f'{name}_us_per_half_step'] = float(np.median(times[name]))
        out[f'{name}_spread_us'] = float(np.max(times[name]) - np.min(times[name]))
        out[f'{name}_acceptance'] = float(samplers[name].acceptance_fraction.mean())
    for name in ('de', 'snooker', 'mixture'):
        out[f'{name}_over_stretch'] = out[f'{name}_us_per_half_step'] / out['stretch_us_per_half_step']
    return out


def mixing(nsteps, discard):
    import bisip_amd
    from bisip_amd.synthetic import write_spectrum_file
    out = dict(bench='moves_mixing', walkers=32, nsteps=nsteps, discard=discard)
    with tempfile.TemporaryDirectory(prefix='bisip_moves_') as d:
        path = write_spectrum_file(os.path.join(d, 'two_modes.csv'), 20, 0)
        for name, moves in (('stretch', None), ('mixture', MIXTURE)):
            m = bisip_amd.PeltonColeCole(path, n_modes=2, nwalkers=32, nsteps=nsteps)
            p0 = TRUTH + 1e-3 * np.random.default_rng(4).standard_normal((32, 7))
            p0[1::2] = p0[1::2][:, SWAP]
            np.random.seed(31)
            m.fit(p0=p0, rng='philox', persistent=False, chain='device', moves=moves)
            tau = m.sampler.get_autocorr_time(discard=discard, quiet=True)
            out[f'{name}_tau_log_tau_1'] = float(tau[3])
            out[f'{name}_switch_rate'] = float(np.mean(m.get_mode_switch_rate(discard=discard)))
            out[f'{name}_acceptance'] = float(m.sampler.acceptance_fraction.mean())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--mixing-steps', type=int, default=4000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moves_bench.jsonl'))
    args = ap.parse_args()
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns, write_spectrum_file
    lines = []
    batch = bisip_amd.SpectraBatch('PeltonColeCole', [synthetic_columns(32, i) for i in range(512)], nwalkers=256, nsteps=1,
                                   n_modes=2)
    lines.append(speed('survey-512x256-cc2', batch.ctx, 256, 512, batch.ndim, batch.param_bounds, args.steps, args.warmup,
                       args.reps))
    batch.close()
    print(json.dumps(lines[-1]), flush=True)
    with tempfile.TemporaryDirectory(prefix='bisip_moves_') as d:
        m = bisip_amd.PeltonColeCole(write_spectrum_file(os.path.join(d, 'one.csv'), 32, 0), n_modes=1, nwalkers=4096, nsteps=1)
        ctx = m._context()
        ctx.set_bounds(m.param_bounds)
        lines.append(speed('ensemble-4096-cc1', ctx, 4096, 1, m.param_bounds.shape[1], m.param_bounds, args.steps, args.warmup,
                           args.reps))
    print(json.dumps(lines[-1]), flush=True)
    lines.append(mixing(args.mixing_steps, args.mixing_steps // 4))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
