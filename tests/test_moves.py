"""The differential-evolution and snooker moves as bisip_amd/moves.py states them: the draws of their stream against
their closed-form laws, the moves -- run by the device sampler's own driver around a NumPy backend
(tests/numpy_move_backend.py) on the Philox stream -- against a posterior that is drawn exactly, accepted and rejected
as soon as the snooker factor or the DE difference is changed, and the public surface.  No GPU."""

import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_posterior as ep
from conftest import ROOT

MIXTURE = [('de', 0.8), ('snooker', 0.2)]
# the tests of the stream: per W two chi-squares of pairs, two of triples, one KS and one correlation; two chi-squares
# of the schedule: one family at 1e-3, as test_draws_of_the_contract_follow_their_laws shares its level
P_FIT = 1e-3 / (5 * 6 + 2)


# ---------------------------------------------------------------------------------------------------------------
# the draws of the stream
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('W', [4, 6, 7, 32, 33])
def test_draws_of_the_move_stream_follow_their_laws(W):
    """>= 2^18 slots of move_stream, E = 64 ensembles: (i0, i1) is uniform over the Nc (Nc - 1) ordered pairs of
    distinct ranks of the OTHER half, (i0, i1, i2) over the ordered triples (chi-square per half), the normal deviate
    behind gamma is finite and N(0, 1) (KS), active and ln u are the stretch contract's own, and none of it touches
    what philox_stream gives."""
    from scipy import stats
    from bisip_amd.moves import move_stream
    from bisip_amd.sampler import affine_splits
    from numpy_stretch_backend import philox_stream
    E, seed, step0 = 64, 0x600d0000 + W, 5
    nh = (W + 1) // 2
    n = -(-(1 << 18) // (E * W)) + 1
    perm = affine_splits(seed, W, step0, n)
    before = philox_stream(W, 5, 2.0, seed, step0, perm, E)
    s = {k: v.reshape(n, 2, E, nh) for k, v in move_stream(W, seed, step0, perm, g0=1.0, sigma=1.0, E=E).items()}
    after = philox_stream(W, 5, 2.0, seed, step0, perm, E)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # the slot's walker and its ln u are the ones a stretch iteration would have used
    assert np.array_equal(s['active'].reshape(n, 2, -1), before['active'])
    assert np.array_equal(s['logu'].reshape(n, 2, -1), before['logu'])
    A, B = perm[:, 0].astype(np.int64)[:, None, None], perm[:, 2].astype(np.int64)[:, None, None]
    offset = (np.arange(E) * W)[None, :, None]
    normals = []
    for h in (0, 1):
        Ns = nh if h == 0 else W // 2
        Nc = W - Ns
        ranks = []
        for name in ('p0', 'p1', 'p2')[:3 if Nc >= 3 else 2]:
            local = s[name][:, h, :, :Ns] - offset
            assert local.min() >= 0 and local.max() < W                     # inside its own ensemble
            pi = (A * local + B) % W
            assert np.all(pi % 2 == 1 - h)                                    # every partner: the other half
            r = (pi - (1 - h)) // 2
            assert r.min() >= 0 and r.max() < Nc
            ranks.append(r.ravel())
        if Nc < 3:
            assert not s['p2'][:, h].any()
        assert np.all(ranks[0] != ranks[1])
        # ordered pairs of distinct ranks: cell (i0, position of i1 among the others)
        cell = ranks[0] * (Nc - 1) + ranks[1] - (ranks[1] > ranks[0])
        counts = np.bincount(cell, minlength=Nc * (Nc - 1))
        assert counts.size == Nc * (Nc - 1) and stats.chisquare(counts).pvalue >= P_FIT, (h, 'pairs')
        if Nc >= 3:
            assert np.all(ranks[2] != ranks[0]) and np.all(ranks[2] != ranks[1])
            third = ranks[2] - (ranks[2] > ranks[0]) - (ranks[2] > ranks[1])
            counts = np.bincount(cell * (Nc - 2) + third, minlength=Nc * (Nc - 1) * (Nc - 2))
            assert counts.size == Nc * (Nc - 1) * (Nc - 2) and counts.mean() >= 5
            assert stats.chisquare(counts).pvalue >= P_FIT, (h, 'triples')
        normals.append((s['gamma'][:, h, :, :Ns] - 1.0).ravel())             # g0 = sigma = 1: gamma = 1 + n
    normals = np.concatenate(normals)
    assert normals.size >= 1 << 18 and np.isfinite(normals).all()
    assert stats.kstest(normals, 'norm').pvalue >= P_FIT
    # the normal deviate shares nothing with the stretch factor of the same slot
    zz = before['zz'].reshape(n, 2, E, nh)[:, 0].ravel()
    g = (s['gamma'][:, 0] - 1.0).ravel()
    assert abs(np.corrcoef(zz, g)[0, 1]) * np.sqrt(zz.size) <= stats.norm.ppf(1.0 - P_FIT / 2.0)    # two-sided, its share
    # ensembles do not share a stream
    assert len({s['gamma'][:, 0, e].tobytes() for e in range(E)}) == E


def test_schedule_follows_the_weights_and_is_a_function_of_seed_and_step():
    from scipy import stats
    from bisip_amd.moves import move_schedule
    n = 1 << 16
    for weights in ([0.8, 0.2], [1.0, 2.0, 1.0]):
        w = np.array(weights)
        j = move_schedule(77, 0, n, w)
        assert j.dtype == np.int32 and j.min() == 0 and j.max() == len(w) - 1
        assert stats.chisquare(np.bincount(j, minlength=len(w)), n * w / w.sum()).pvalue >= P_FIT
        # chunks of a run draw what the run draws, and another seed another schedule
        assert np.array_equal(np.concatenate([move_schedule(77, 0, 1000, w), move_schedule(77, 1000, n - 1000, w)]), j)
        assert not np.array_equal(move_schedule(78, 0, n, w), j)
    assert not move_schedule(1, 0, 100, [1.0]).any()


# ---------------------------------------------------------------------------------------------------------------
# the moves are accepted, their mutants are rejected
# ---------------------------------------------------------------------------------------------------------------

def _snooker(coords, arr, params):
    from bisip_amd.moves import snooker_proposal
    return snooker_proposal(coords[arr['active']], coords[arr['p0']], coords[arr['p1']], coords[arr['p2']], params['gammas'])


def _snooker_without_factor(coords, arr, params):
    q, factor = _snooker(coords, arr, params)
    return q, np.where(np.isfinite(factor), 0.0, factor)


def _snooker_exponent_ndim(coords, arr, params):
    q, factor = _snooker(coords, arr, params)
    ndim = coords.shape[1]
    return q, factor * (ndim / (ndim - 1.0))


def _de_towards_a_walker(coords, arr, params):
    s = coords[arr['active']]
    return s + arr['gamma'][:, None] * (coords[arr['p0']] - s), np.zeros(s.shape[0])


def _exact_run(prob, moves, E, W, steps, thin, seed, proposals=None):
    from bisip_amd.sampler import DeviceEnsembleSampler
    from numpy_move_backend import NumpyMoveBackend
    p0, _ = prob.exact_draws(E * W, np.random.RandomState(11))
    s = DeviceEnsembleSampler(W, prob.ndim, backend=NumpyMoveBackend(prob.logp, E, proposals), rng='philox', seed=seed,
                              n_ensembles=E, moves=moves, chunk=100)
    s.run_mcmc(p0, steps // thin, thin_by=thin)
    assert s.last_path == 'launch-per-half-step' and s.last_stream == 'arrays'
    chain = s.get_chain().reshape(steps // thin, E, W, prob.ndim)
    assert np.isfinite(s.get_log_prob()).all()                # no sample ever leaves the open box
    return chain, s


def test_moves_are_accepted_and_their_mutants_are_rejected():
    """E = 64 ensembles of W = 16 walkers, every walker started at an exact draw of the truncated (8, 2) posterior, 400
    steps stored every 2, the Philox stream of seed 20241021.  DE, snooker and the 0.8 / 0.2 mixture keep every feature
    within t_limit(64, 17) = 4.31; snooker without its factor, snooker with exponent ndim for ndim - 1 and the DE
    mutant q = s + gamma (c_a - s) exceed it at least threefold.

    Measured on this stream: de 1.26, snooker 2.14, mixture 2.03; snooker with factor 0: 186; exponent ndim: 24.8;
    q = s + gamma (c_a - s): 720 (it accepts 99.9 % of its proposals and contracts the ensemble)."""
    from bisip_amd.moves import MOVE_DE, MOVE_SNOOKER
    prob = ep.truncated_problem()
    ref = ep.reference(prob)
    E, W, steps, thin, seed = 64, 16, 400, 2, 20241021
    limit = ep.t_limit(E, ref['mean'].size)
    assert abs(limit - 4.31) < 0.01
    got = {}
    for label, moves, proposals in (('de', 'de', None), ('snooker', 'snooker', None), ('mixture', MIXTURE, None),
                                    ('snooker-factor-0', 'snooker', {MOVE_SNOOKER: _snooker_without_factor}),
                                    ('snooker-exponent-ndim', 'snooker', {MOVE_SNOOKER: _snooker_exponent_ndim}),
                                    ('de-towards-a-walker', 'de', {MOVE_DE: _de_towards_a_walker})):
        chain, s = _exact_run(prob, moves, E, W, steps, thin, seed, proposals)
        got[label] = ep.worst(prob.t_statistics(chain, ref), ref['names'])
        print(f'{label}: max|T| = {got[label][0]:.2f} at {got[label][1]} (limit {limit:.2f}), '
              f'acceptance {s.acceptance_fraction.mean():.3f}')
    for label in ('de', 'snooker', 'mixture'):
        assert got[label][0] <= limit, got
    for label in ('snooker-factor-0', 'snooker-exponent-ndim', 'de-towards-a-walker'):
        assert got[label][0] >= 3 * limit, got


# ---------------------------------------------------------------------------------------------------------------
# the driver around the moves
# ---------------------------------------------------------------------------------------------------------------

def _driver_run(moves, W=12, E=1, chunk=None, thin=1, n=30, backend=None, **kw):
    from bisip_amd.sampler import DeviceEnsembleSampler
    from numpy_move_backend import NumpyMoveBackend
    prob = ep.problem(8, 0)
    p0, _ = prob.exact_draws(E * W, np.random.RandomState(3))
    be = backend(prob.logp, E) if backend is not None else NumpyMoveBackend(prob.logp, E)
    s = DeviceEnsembleSampler(W, prob.ndim, backend=be, rng='philox', seed=99, n_ensembles=E, moves=moves, chunk=chunk, **kw)
    s.run_mcmc(p0, n, thin_by=thin)
    return s


def test_chunks_thinning_and_continuation_do_not_change_the_chain():
    three = [('de', 1.0), ('snooker', 1.0), ('stretch', 1.0)]
    whole = _driver_run(three, W=13, n=30)
    assert 0.05 < whole.acceptance_fraction.mean() < 0.95
    chunked = _driver_run(three, W=13, n=30, chunk=7)
    assert np.array_equal(chunked.get_chain(), whole.get_chain())
    assert np.array_equal(chunked.get_log_prob(), whole.get_log_prob())
    assert np.array_equal(chunked.acceptance_fraction, whole.acceptance_fraction)
    cont = _driver_run(three, W=13, n=18, chunk=5)
    cont.run_mcmc(None, 12)
    assert np.array_equal(cont.get_chain(), whole.get_chain())
    thinned = _driver_run(three, W=13, n=10, thin=3, chunk=4)
    assert np.array_equal(thinned.get_chain(), whole.get_chain()[2::3])
    cont.reset()
    cont.run_mcmc(None, 4)
    assert cont.get_chain().shape[0] == 4 and cont.acceptance_fraction.max() <= 1.0


def test_a_mixture_that_is_all_stretch_is_the_stretch_sampler():
    from bisip_amd.moves import StretchMove
    from numpy_stretch_backend import NumpyStretchBackend
    plain = _driver_run(None, W=12, E=2, backend=NumpyStretchBackend, persistent=False)
    for moves in ('stretch', [StretchMove(), ('stretch', 3.0)]):
        mixed = _driver_run(moves, W=12, E=2)
        assert np.array_equal(mixed.get_chain(), plain.get_chain())
        assert np.array_equal(mixed.get_log_prob(), plain.get_log_prob())
        assert np.array_equal(mixed.acceptance_fraction, plain.acceptance_fraction)
    other = _driver_run(StretchMove(a=1.5), W=12, E=2)
    assert other.a == 1.5 and not np.array_equal(other.get_chain(), plain.get_chain())


# ---------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------

def test_parse_moves_forms_and_refusals():
    from bisip_amd.moves import (DEMove, DESnookerMove, StretchMove, is_native, parse_moves, MOVE_DE, MOVE_SNOOKER,
                                 MOVE_STRETCH)
    moves, w = parse_moves('de')
    assert [m.kind for m in moves] == [MOVE_DE] and w.tolist() == [1.0]
    assert moves[0].sigma == 1e-5 and moves[0].g0(8) == 2.38 / np.sqrt(16.0) and DEMove(gamma0=0.5).g0(8) == 0.5
    moves, w = parse_moves(DESnookerMove(gammas=1.2))
    assert moves[0].kind == MOVE_SNOOKER and moves[0].gammas == 1.2 and DESnookerMove().gammas == 1.7
    moves, w = parse_moves(['de', DESnookerMove(), 'stretch'])
    assert [m.kind for m in moves] == [MOVE_DE, MOVE_SNOOKER, MOVE_STRETCH] and w.tolist() == [1.0, 1.0, 1.0]
    moves, w = parse_moves([(DEMove(), 0.8), ('snooker', 0.2)])
    assert [m.kind for m in moves] == [MOVE_DE, MOVE_SNOOKER] and w.tolist() == [0.8, 0.2]
    assert StretchMove().a == 2.0
    for bad in ('walk', ['de', 'kde'], [('de', 0.0)], [('de', -1.0)], [('de', float('nan'))], [], [('de', 1.0, 2.0)],
                [DEMove(sigma=1e-5), DEMove(sigma=1e-3)], [('snooker', 1.0), (DESnookerMove(gammas=2.0), 1.0)]):
        with pytest.raises(ValueError):
            parse_moves(bad)
    with pytest.raises(TypeError):
        parse_moves([object()])
    with pytest.raises(ValueError):
        StretchMove(a=1.0)
    assert is_native('de') and is_native('walk') and is_native([('de', 0.8), (DESnookerMove(), 0.2)]) and is_native(DEMove())
    assert not is_native(object()) and not is_native([object()]) and not is_native([(object(), 1.0)])
    assert is_native([]) and is_native(())                    # nobody's moves: parse_moves refuses them (above)


def test_sampler_refuses_what_the_moves_do_not_serve():
    from bisip_amd.sampler import DeviceEnsembleSampler
    from numpy_move_backend import NumpyMoveBackend
    from numpy_stretch_backend import NumpyStretchBackend
    be = NumpyMoveBackend(lambda x: np.zeros(len(x)))
    for kw, text in ((dict(nwalkers=3, moves='de'), 'at least 4'), (dict(nwalkers=5, moves='snooker'), 'at least 6'),
                     (dict(nwalkers=4, moves=MIXTURE), 'at least 6'), (dict(moves='de', persistent=True), 'persistent'),
                     (dict(moves='de', rng='numpy'), 'philox'), (dict(moves='de', distributed=True), 'one rank'),
                     (dict(moves='de', force_sharded_path=True), 'one rank'),
                     (dict(moves='de', sharded_loop='simulate:2'), 'one rank'), (dict(moves='kde'), 'unknown move'),
                     (dict(moves='de', backend=NumpyStretchBackend(None)), 'hooks')):
        kw = dict(dict(nwalkers=8, ndim=2, backend=be, rng='philox'), **kw)
        with pytest.raises(ValueError, match=text):
            DeviceEnsembleSampler(kw.pop('nwalkers'), kw.pop('ndim'), **kw)
    # 4 walkers serve 'de', 6 'snooker'; persistent=None resolves to the launch path
    assert DeviceEnsembleSampler(4, 2, backend=be, rng='philox', moves='de').persistent is False
    assert DeviceEnsembleSampler(6, 2, backend=be, rng='philox', moves=MIXTURE).persistent is False


def test_abi_carries_the_three_symbols_and_stays_at_6():
    import __graft_entry__
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    for name in ('bisip_move_draw_dev', 'bisip_move_half_dev', 'bisip_move_run_dev'):
        assert re.search(r'\bint %s\(' % name, header) and name in exports and name in _hip.SYMBOLS
    assert __graft_entry__.header_abi_version() == 6
    assert [f[0] for f in _hip.MoveArgs._fields_] == ['stretch', 'active', 'p0', 'p1', 'p2', 'gamma', 'logu', 'snooker_gamma']
    assert _hip.MoveArgs._fields_[0][1] is _hip.StretchArgs


def test_fit_hands_any_other_moves_object_to_emcee(monkeypatch):
    """fit(moves=<not a native move>) takes the emcee branch as before: emcee.EnsembleSampler gets the object."""
    import bisip_amd
    calls = {}

    class FakeSampler:
        def __init__(self, nwalkers, ndim, log_prob_fn, moves=None, vectorize=False):
            calls['init'] = (nwalkers, ndim, moves, vectorize)

        def run_mcmc(self, p0, nsteps, progress=False):
            calls['run'] = (np.shape(p0), nsteps)

    class FakeContext:
        variant = 'collapsed'

        def set_bounds(self, bounds):
            pass

        def logprob(self, theta):
            return np.zeros(len(theta))

    model = bisip_amd.PeltonColeCole(bisip_amd.DataFiles()['SIP-K389175'], nwalkers=16, nsteps=3, n_modes=1)
    monkeypatch.setattr(model, '_context', lambda: FakeContext())
    theirs = object()
    monkeypatch.setitem(sys.modules, 'emcee', None)
    with pytest.raises(ImportError):          # without emcee the branch is reached and says so
        model.fit(moves=theirs)
    fake = types.ModuleType('emcee')
    fake.EnsembleSampler = FakeSampler
    monkeypatch.setitem(sys.modules, 'emcee', fake)
    model.fit(moves=theirs)
    assert calls['init'][2] is theirs and calls['init'][3] is True and calls['run'] == ((16, model.ndim), 3)
    with pytest.raises(ValueError, match='philox'):
        model.fit(moves='de', rng='numpy')
    with pytest.raises(ValueError, match='unknown move'):
        model.fit(moves='kde')
    with pytest.raises(ValueError, match='moves must be'):      # an empty list is not an emcee object
        model.fit(moves=[])
