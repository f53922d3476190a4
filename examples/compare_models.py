#!/usr/bin/env python3
"""Which model does the spectrum support: Pelton Cole-Cole with one mode and with two, fitted to the same spectrum and
ranked by WAIC, by PSIS-LOO and by their marginal likelihood (bridge sampling), whether each fits the spectrum within its
errors at all (posterior predictive checks), and where the better one still misses the data.  The chains stay on the GPU;
the sums over them (bisip_fit_quality_dev, bisip_predictive_check_dev), the Pareto-smoothed tails of every data point
(bisip_loo_columns_dev) and the bridge-sampling iteration (bisip_bridge_*_dev) are taken there."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout

import numpy as np

from bisip_amd import DataFiles, PeltonColeCole
from bisip_amd.evidence import compare_evidence
from bisip_amd.fitquality import compare_waic
from bisip_amd.loo import compare_loo

filepath = DataFiles()['SIP-K389174']                         # two bumps in its imaginary part (docs/tutorials/pelton.ipynb)
results, loos, evidences, checks, models = {}, {}, {}, {}, {}
for n_modes in (1, 2):
    np.random.seed(42)
    model = PeltonColeCole(filepath, nwalkers=64, nsteps=2000, n_modes=n_modes)
    if n_modes == 2:      # the modes are interchangeable: boxes that do not overlap, as the reference's Pelton tutorial does
        model.params.update(log_tau1=[-5, 5], log_tau2=[-15, -10])
    model.fit(chain='device')
    name = f'{n_modes} mode' + 's' * (n_modes > 1)
    results[name], loos[name], models[name] = model.get_waic(discard=1000), model.get_loo(discard=1000), model
    evidences[name] = model.get_evidence(discard=1000)          # the log marginal likelihood by bridge sampling
    checks[name] = model.get_predictive_check(discard=1000)     # does the model reproduce the data within their errors
    dic = model.get_dic(discard=1000)
    print(f'{name}: DIC {dic["dic"]:.1f}, p_D {dic["p_d"]:.1f}; {results[name]["n_high"]} points with p_waic > 0.4')

# the double Cole-Cole model once more with the SAME box for both modes: the chain may now hold both labellings of the modes
# (here it does: it starts from the ensemble above with the modes of every other walker exchanged), so the evidence is taken
# over one of them -- the samples with their modes in order of log_tau, log(2!) added (bisip_amd.modes).  Its prior box is 8
# times the volume of the two boxes above and holds the posterior twice: log_evidence should come out log(8 / 2) = 1.39 lower
np.random.seed(42)
model = PeltonColeCole(filepath, nwalkers=64, nsteps=2000, n_modes=2)
p0 = models['2 modes'].get_chain()[-1].copy()
p0[1::2] = p0[1::2][:, [0, 2, 1, 4, 3, 6, 5]]
model.fit(p0=p0, chain='device')
evidences['2 modes, one box'] = model.get_evidence(discard=1000, order_modes='log_tau')
rate = model.get_mode_switch_rate(discard=1000)
print(f'2 modes, one box: {np.mean((rate > 0) & (rate < 1)):.0%} of the walkers switch labels, {np.mean(rate == 1):.0%} keep the other one; '
      f'ordered log_tau {model.get_ordered_mean(discard=1000)[3:5].round(2)} +- {model.get_ordered_std(discard=1000)[3:5].round(2)}, '
      f'phase-peak log_tau {model.get_mode_mean(discard=1000)[3:5].round(2)}')

print('model      elpd_waic  p_waic   d_elpd    d_se')
for row in compare_waic(results):                             # the best model first
    print(f'{row["name"]:<10} {row["elpd_waic"]:9.1f} {row["p_waic"]:7.1f} {row["d_elpd"]:8.1f} {row["d_se"]:7.1f}')

# where n_high > 0 WAIC is unreliable: PSIS-LOO is the estimate to turn to, and pareto_k shows which points make it fragile
print('model       elpd_loo   p_loo   d_elpd    d_se  n_bad')
for row in compare_loo(loos):
    print(f'{row["name"]:<10} {row["elpd_loo"]:9.1f} {row["p_loo"]:7.1f} {row["d_elpd"]:8.1f} {row["d_se"]:7.1f} {row["n_bad"]:6d}')

# the evidence itself: Bayes factors against the best model and posterior model probabilities under equal prior odds
print('model      log_evidence   log_bf    prob      se')
for row in compare_evidence(evidences):
    print(f'{row["name"]:<10} {row["log_evidence"]:12.2f} {row["log_bf"]:8.2f} {row["prob"]:7.3f} {row["se"]:7.2f}')

# the criteria above are relative; the predictive checks are not: chi2_reduced near 1 and no probability near 0 is a fit.  A
# small p_runs: the residuals run in bands along the frequency axis, the model misses the spectrum's shape
print('model      chi2_reduced   p_chi2   p_runs    p_max  n_extreme')
for name, c in checks.items():
    print(f'{name:<10} {c["chi2_reduced"]:12.2f} {c["p_chi2"]:8.3g} {c["p_runs"]:8.3g} {c["p_max"]:8.3g} {c["n_extreme"]:10d}')

best = compare_waic(results)[0]['name']
misfit = models[best].get_pointwise_misfit(discard=1000)      # (2, N): near 1, the point is fitted to its error bar
worst = np.unravel_index(np.argmax(misfit), misfit.shape)
print(f'{best}: misfit at most {misfit.max():.1f}, at the {("real", "imaginary")[worst[0]]} part of frequency {worst[1]}')
k = loos[best]['pareto_k']
print(f'{best}: Pareto k at most {k.max():.2f} (threshold {loos[best]["k_threshold"]:.2f}), at the '
      f'{("real", "imaginary")[np.unravel_index(np.argmax(k), k.shape)[0]]} part of frequency {np.unravel_index(np.argmax(k), k.shape)[1]}')
