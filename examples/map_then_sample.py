#!/usr/bin/env python3
"""Find the optimum first, then sample around it.

fit_map() runs a multi-start Levenberg-Marquardt fit of the misfit inside the prior box on the GPU (every start in one
kernel launch) and returns the least-squares Cole-Cole parameters, their Laplace covariance and a Laplace evidence before any
chain exists; fit(p0='map') starts the walkers in a ball of that covariance around the optimum instead of uniformly in the
box, so that no burn-in has to be discarded."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bisip_amd  # noqa: E402

path = bisip_amd.DataFiles()['SIP-K389175']
model = bisip_amd.PolynomialDecomposition(path, nwalkers=32, nsteps=1000)

# the point estimate: milliseconds
best = model.fit_map(n_starts=32, seed=0)
print('parameters          ', model.param_names)
print('least-squares optimum', np.round(best['theta'], 4))
print('Laplace std          ', np.round(np.sqrt(np.diag(best['cov'])), 4))
print(f"chi2 {best['chi2']:.3f}, log-probability {best['logp']:.3f}, status {best['status']}, "
      f"{best['n_agree']} of {len(best['all_logp'])} starts reach it, {int(best['at_bound'].sum())} parameters on a bound")
print(f"Laplace log-evidence {best['log_evidence_laplace']:.3f}")

# the chain, started where it will stay
np.random.seed(0)
model.fit(p0='map', chain='device')
trace = model.get_log_prob_trace(50.0)
print(f'median log-probability of the walkers: step 1 {trace[0]:.2f}, step 1000 {trace[-1]:.2f} (optimum {best["logp"]:.2f})')
print('posterior mean       ', np.round(model.get_param_mean(discard=0), 4))
print('posterior std        ', np.round(model.get_param_std(discard=0), 4))
ev = model.get_evidence(discard=0)
print(f"bridge-sampling log-evidence {ev['log_evidence']:.3f} +- {ev['se']:.3f}")

# a survey's first look: every spectrum's optimum in one call
files = bisip_amd.DataFiles()
batch = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in sorted(files)], nwalkers=64, nsteps=500, n_modes=1)
quick = batch.fit_map(n_starts=32, seed=0)
for k, theta, chi2, n in zip(sorted(files), quick['theta'], quick['chi2'], quick['n_agree']):
    print(f'{k}: chi2 {chi2:9.2f}  theta {np.round(theta, 3)}  ({n} of 32 starts agree)')
batch.fit(p0='map', seed=0, chain='device')
print('acceptance', round(float(batch.acceptance_fraction.mean()), 3))
batch.close()
