"""The Cole-Cole, Dias and Shin kernels against the exact value of the reference's formula, frequency by frequency, within a
rounding bound counted from kernels.h (tests/model_bounds.py: its docstring derives the bound and the probe).

The log-probability kernel gives back ONE residual bit for bit when all but one sigma of the spectrum are large (the probe
spectrum), so the `residual` path that the samplers run -- folded constants, shared reciprocals, stepped exponentials,
pairs, block tails -- is read at every frequency and in both parts, not through a sum of 2 N squares with 1e-10 of room.
`forward()` (the `eval` path) is held to the same exact value within its own bound.

Shapes: the smallest at which the loops differ.  Grid + FAST (Cole-Cole with one to three modes, Shin): N = 33 -- two full
blocks of 16, every q = 0..15, four quarters, one unpaired frequency -- and N = 21, a block and a partial quarter.  FAST off
the grid (ln w jittered by 1e-3; also what Cole-Cole with four modes and Dias run): N = 5 and 2 for the paired models, 5 for
three and four modes (rcp_batch_n of 3 and 4).  Safe loop (the box widened until loop_flags == 0, the asserted rows inside
the default box): N = 5.  140,000 and 5,000 rows: one and four lanes per walker; 256 asserted rows lead both launches --
uniform rows and the edges built by model_bounds.rows.

Measured on the MI355X, printed again by every run (the table of DESIGN.md section 2): worst |error| / bound of the residual
path over rows, frequencies and parts; the worst error in ulp of the sum of the terms of that part (|C| + r0 with them in the
real part); forward() against its own bound.
  model          grid N = 33 / 21                       FAST off the grid, N = 5 / 2          safe, N = 5
  Cole-Cole 1    0.46 / 0.46, 14.3 / 13.9 ulp; 0.46     0.43 / 0.41, 10.1 / 10.7 ulp; 0.43    0.43, 10.2 ulp; 0.43
  Cole-Cole 2    0.40 / 0.39, 12.2 / 13.0 ulp; 0.40     0.30 / 0.21, 7.7 / 7.7 ulp; 0.30      0.30, 7.3 ulp; 0.30
  Cole-Cole 3    0.26 / 0.24, 11.8 / 14.2 ulp; 0.26     0.18, 6.4 ulp; 0.18                   0.18, 6.4 ulp; 0.18
  Cole-Cole 4    (no stepped loop)                      0.20, 7.2 ulp; 0.20                   0.20, 7.2 ulp; 0.20
  Dias           (no stepped loop)                      0.50 / 0.50, 4.8 / 4.4 ulp *; 0.50    0.50, 4.4 ulp *; 0.50
  Shin           0.17 / 0.17, 15.2 / 14.6 ulp; 0.18     0.13 / 0.11, 11.4 / 11.4 ulp; 0.16    0.15, 11.4 ulp; 0.15
  * on the rows with delta < 0.9; 421 ulp at delta = 0.9998, where 1/delta - 1 loses 1/(1 - delta) = 5224 in any double
    evaluation (the reference's doubles: 419 ulp on the same row).
On the grid the worst error by q = f mod 16 stays at 5 .. 12 ulp up to q = 11 and reaches 12 .. 15 ulp at q = 12 .. 15 (the
direct loops: 6 .. 11): under the "<= 22 ulp on a term" that kernels.h states for quarter and step.
"""

import numpy as np
import pytest

import model_bounds as mb

pytestmark = pytest.mark.gpu

FLAGS = {'grid': 3, 'fast': 1, 'safe': 0}
ROWS_ONE_LANE, ROWS_FOUR_LANES = 140000, 5000
ROWSETS = [(model, D, loop, N) for model, D in mb.CASES for loop, N in mb.shapes(model, D)]


def _id(v):
    return '-'.join(str(x) for x in v)


@pytest.mark.parametrize('rs', ROWSETS, ids=_id)
def test_every_residual_and_forward_within_the_rounding_bound_of_the_exact_value(rs):
    from bisip_amd import _hip
    model, D, loop, N = rs
    mid = mb.MODELS[model]
    kw = dict(n_modes=D) if model == 'PeltonColeCole' else {}
    w = mb.frequencies(N, loop)
    assert (_hip.frequency_grid_step(w) is not None) == (loop == 'grid')
    box = mb.wide_box(model, D) if loop == 'safe' else mb.default_box(model, D)
    th = mb.rows(model, D, w)
    R = len(th)
    theta = np.concatenate([th, mb.filler(model, D, ROWS_ONE_LANE - R)])
    ex = mb.exact(model, th, w)
    unit = ex['unit'].astype(np.float64)[:, None, :]
    zmax = 2 * np.abs(ex['Z']).max(axis=(1, 2)).astype(np.float64)
    bounds = {path: mb.bound(ex, loop, path) for path in ('residual', 'eval')}
    for b in bounds.values():
        mb.assert_reference_is_sharp(ex, b)
        mb.assert_bound_is_worth_having(ex, b)

    got, du = np.empty((R, 2, N)), np.empty((R, 2, N))
    Z = None
    for part in (0, 1):
        for j in range(N):
            zn, zn_err = mb.probes(w, part, j)
            ctx = _hip.HipContext(mid, w, zn, zn_err, box, **kw)
            assert ctx.loop_flags == FLAGS[loop], (rs, ctx.loop_flags)
            one = ctx.logprob(theta)[:R]
            four = ctx.logprob(theta[:ROWS_FOUR_LANES])[:R]
            assert np.array_equal(one, four), (rs, part, j)
            got[:, part, j], du[:, part, j] = mb.recover(one, N, zmax)
            if Z is None:
                Z = ctx.forward(th)
            ctx.close()
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(Z))
    mb.assert_recovery_is_sharp(du, bounds['residual'], unit)

    res = mb.excess(got, ex, bounds['residual'], du)
    fwd = mb.signed_excess(Z, ex, bounds['eval'])
    # in ulp of the sum of the terms of that part (and |C| + r0 in the real part): what a reader of "x ulp on a term" expects
    scale = np.abs(ex['T']).sum(axis=1)
    scale[:, 0] += (ex['unit'] - ex['Tabs'].sum(axis=1))
    # (parts that are 2^-60 of the unit and less -- a clamped tau', m = 5e-324 -- say nothing in ulp: left out of this figure)
    seen = scale > 2.0 ** -60 * ex['unit'][:, None, :]
    err_ulp = np.where(seen, np.abs(got.astype(mb.LD) - np.abs(ex['Z'])) / np.where(seen, scale * mb.ULP, 1), 0).astype(np.float64)
    note = ''
    if model == 'Dias2000':
        # 1/delta - 1 loses 1/(1 - delta) in any double evaluation (the reference's too): the figure away from delta = 1
        note = f' ({err_ulp[th[:, 4] < 0.9].max():.2f} on the rows with delta < 0.9)'
    line = (f'{_id(rs)}: residual {res.max():.3f} of the bound, {err_ulp.max():.2f} ulp of the terms{note}; '
            f'forward {fwd.max():.3f} of its bound')
    if loop == 'grid':
        byq = [err_ulp[:, :, q::mb.GRID_BLOCK].max() for q in range(min(N, mb.GRID_BLOCK))]
        line += '; ulp by q: ' + ' '.join(f'{x:.2f}' for x in byq)
    print(line)
    i = np.unravel_index(np.argmax(res), res.shape)
    assert res.max() <= 1.0, (rs, 'residual', i, th[i[0]], got[i], float(np.abs(ex['Z'][i])), bounds['residual'][i])
    i = np.unravel_index(np.argmax(fwd), fwd.shape)
    assert fwd.max() <= 1.0, (rs, 'forward', i, th[i[0]], Z[i], float(ex['Z'][i]), bounds['eval'][i])
