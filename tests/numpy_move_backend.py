"""CPU stand-in for the move hooks of bisip_amd.sampler.HipStretchBackend (draw_moves, run_moves), used ONLY by tests:
NumpyStretchBackend plus the differential-evolution and snooker half-steps as bisip_amd/moves.py states them, around any
log-probability.  ``run_moves`` over arrays that a device drew is the replay the kernels are held to bit for bit
(tests/test_gpu_moves.py); over ``move_stream``'s own arrays it is what tests/test_moves.py holds to a posterior that is
drawn exactly.

``proposals`` replaces a move's proposal function (kind -> f(coords, arrays of the half-step, params) -> (q, factor)):
the mutants of tests/test_moves.py."""

import numpy as np
import torch

from bisip_amd import moves as mv
from numpy_stretch_backend import NumpyStretchBackend

MOVE_ARRAYS = ('active', 'p0', 'p1', 'p2', 'gamma', 'logu')


def propose(kind, coords, arr, params):
    """(q, factor) of the slots of one half-step: ``arr`` holds that half-step's move arrays, ``params`` the sampler's
    dict (gammas)."""
    s = coords[arr['active']]
    if kind == mv.MOVE_DE:
        return mv.de_proposal(s, coords[arr['p0']], coords[arr['p1']], arr['gamma'])
    if kind == mv.MOVE_SNOOKER:
        return mv.snooker_proposal(s, coords[arr['p0']], coords[arr['p1']], coords[arr['p2']], params['gammas'])
    raise ValueError(f'no proposal for move kind {kind}')


def move_half(coords, logp, arr, kind, logprob_fn, params, proposals=None):
    """One half-step of move ``kind`` in place on host arrays -> (idx, rows, lps, acc, any NaN)."""
    fn = (proposals or {}).get(kind)
    q, factor = fn(coords, arr, params) if fn is not None else propose(kind, coords, arr, params)
    idx = arr['active']
    s, old = coords[idx], logp[idx]
    new = logprob_fn(q)
    with np.errstate(invalid='ignore'):
        acc = (factor + new) - old > arr['logu']
    return idx, np.where(acc[:, None], q, s), np.where(acc, new, old), acc, bool(np.any(np.isnan(new)))


class NumpyMoveBackend(NumpyStretchBackend):
    def __init__(self, logprob_fn, n_ensembles=1, proposals=None, e0=0):
        super().__init__(logprob_fn, n_ensembles)
        self.proposals = proposals
        self.e0 = e0

    def draw_moves(self, st, W, seed, step0, n_steps, g0, sigma):
        arrs = mv.move_stream(W, seed, step0, st['perm'].numpy(), g0, sigma, E=self.n_ensembles, e0=self.e0)
        for name in MOVE_ARRAYS:
            st['mv_' + name][:] = torch.from_numpy(arrs[name])

    def run_moves(self, st, n_steps, moves):
        W = st['coords'].shape[0]
        coords, logp = st['coords'].numpy(), st['logp'].numpy()
        for k in range(n_steps):
            kind = int(st['kinds'][k])
            for h, n_slots in ((0, (W + 1) // 2), (1, W // 2)):
                if kind == mv.MOVE_STRETCH:
                    self.half(st, k, h, n_slots)
                    continue
                arr = {name: np.asarray(st['mv_' + name][k, h, :n_slots]) for name in MOVE_ARRAYS}
                idx, rows, lps, acc, nan = move_half(coords, logp, arr, kind, self.logprob_fn, moves, self.proposals)
                if nan:
                    st['status'][0] |= 1
                self._commit(st, k, idx, rows, lps, acc)
