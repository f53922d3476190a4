#!/usr/bin/env python3
"""Which model does the spectrum support: Pelton Cole-Cole with one mode and with two, fitted to the same spectrum and
ranked by WAIC, and where the better one still misses the data.  The chains stay on the GPU; the sums over them are taken
there (bisip_fit_quality_dev)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout

import numpy as np

from bisip_amd import DataFiles, PeltonColeCole
from bisip_amd.fitquality import compare_waic

filepath = DataFiles()['SIP-K389174']                         # two bumps in its imaginary part (docs/tutorials/pelton.ipynb)
results, models = {}, {}
for n_modes in (1, 2):
    np.random.seed(42)
    model = PeltonColeCole(filepath, nwalkers=64, nsteps=2000, n_modes=n_modes)
    if n_modes == 2:      # the modes are interchangeable: boxes that do not overlap, as the reference's Pelton tutorial does
        model.params.update(log_tau1=[-5, 5], log_tau2=[-15, -10])
    model.fit(chain='device')
    name = f'{n_modes} mode' + 's' * (n_modes > 1)
    results[name], models[name] = model.get_waic(discard=1000), model
    dic = model.get_dic(discard=1000)
    print(f'{name}: DIC {dic["dic"]:.1f}, p_D {dic["p_d"]:.1f}; {results[name]["n_high"]} points with p_waic > 0.4')

print('model      elpd_waic  p_waic   d_elpd    d_se')
for row in compare_waic(results):                             # the best model first
    print(f'{row["name"]:<10} {row["elpd_waic"]:9.1f} {row["p_waic"]:7.1f} {row["d_elpd"]:8.1f} {row["d_se"]:7.1f}')

best = compare_waic(results)[0]['name']
misfit = models[best].get_pointwise_misfit(discard=1000)      # (2, N): near 1, the point is fitted to its error bar
worst = np.unravel_index(np.argmax(misfit), misfit.shape)
print(f'{best}: misfit at most {misfit.max():.1f}, at the {("real", "imaginary")[worst[0]]} part of frequency {worst[1]}')
