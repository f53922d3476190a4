"""The exact-posterior helper against the oracle, the draws of the rng='philox' contract against their closed-form
laws, and the contract itself -- the stretch move in NumPy on ``philox_stream`` -- against a posterior that is drawn
exactly: accepted, and rejected as soon as its exponent or its z density is changed.  No GPU."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle
import exact_posterior as ep

SHAPES = [(8, 0), (8, 2), (20, 4), (20, 6)]
COND = {(8, 0): 4.5e2, (8, 2): 1.8e4, (20, 4): 6.2e7, (20, 6): 6.9e10}
RATE = {(8, 0): 0.86, (8, 2): 0.68, (20, 4): 0.58, (20, 6): 0.43}


def _normal_limit(n_tests, alpha=1e-3):
    """Two-sided normal quantile at level alpha, Bonferroni over n_tests."""
    from scipy.stats import norm
    return float(norm.ppf(1.0 - alpha / (2.0 * n_tests)))


# ---------------------------------------------------------------------------------------------------------------
# the helper against the oracle
# ---------------------------------------------------------------------------------------------------------------

def _problems():
    out = [ep.problem(nf, P) for nf, P in SHAPES]
    out.append(ep.problem(8, 2, c_exp=0.5))
    out.append(ep.truncated_problem())
    return out


@pytest.mark.parametrize('index', range(6))
def test_helper_logp_is_the_oracle_s(index):
    """logp at exact draws, at rows just inside every face and at rows on / just outside every face, against
    oracle.numpy_logprob: 1e-12 * max(1, |logp|), -inf exactly."""
    prob = _problems()[index]
    op = prob.oracle_problem()
    rng = np.random.RandomState(100 + index)
    draws, _ = prob.exact_draws(200, rng)
    inside, outside = ep.face_rows(prob, rng)
    assert inside.shape == outside.shape == (4 * prob.ndim, prob.ndim)
    for rows, finite in ((draws, True), (inside, True), (outside, False)):
        want = np.array([oracle.numpy_logprob(op, r) for r in rows])
        got = prob.logp(rows)
        if finite:
            assert np.isfinite(want).all() and np.isfinite(got).all()
            assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-12
        else:
            assert np.isneginf(want).all() and np.isneginf(got).all()


@pytest.mark.parametrize('n_freq,poly_deg', SHAPES)
def test_conditioning_and_acceptance_rates(n_freq, poly_deg):
    """cond(H) stays where float64 is accepted (cond * 2^-53 <= 1e-4; Problem refuses anything beyond), and the
    rejection accepts what it should: (lo_r0 / b0)^(P+1) at the posterior's b0, to two digits."""
    prob = ep.problem(n_freq, poly_deg)
    assert prob.cond * 2.0 ** -53 <= 1e-4
    assert abs(prob.cond / COND[(n_freq, poly_deg)] - 1) < 0.05
    assert np.allclose(prob.chol @ prob.chol.T, prob.H, rtol=1e-9, atol=0) and np.all(np.diag(prob.chol) > 0)
    assert abs(ep.reference(prob)['rate'] - RATE[(n_freq, poly_deg)]) < 0.01


@pytest.mark.parametrize('n_freq,poly_deg', SHAPES)
def test_gaussian_part_of_the_exact_sampler(n_freq, poly_deg):
    """Mean and covariance of 1e6 Gaussian draws in b-space (the box-accepted ones, without the Jacobian weight:
    the uncut box is 6+ sd away, it accepts them all) against b_hat and H^-1 -- both computed here a second way,
    by lstsq and by inverting the normal matrix, not through the helper's QR.  Every entry inside its band at a
    family-wise 1e-3."""
    prob = ep.problem(n_freq, poly_deg)
    n, nd = 1000000, prob.ndim
    b = prob.gaussian_b(n, np.random.RandomState(7))
    theta = np.concatenate([b[:, :1], b[:, 1:] / b[:, :1]], axis=1)
    assert np.all((theta > prob.lo) & (theta < prob.hi))
    A = prob.G / prob.sigma[:, None]
    b_hat = np.linalg.lstsq(A, prob.y / prob.sigma, rcond=None)[0]
    C = np.linalg.inv(A.T @ A)
    lim = _normal_limit(nd + nd * (nd + 1) // 2)
    sd = np.sqrt(np.diag(C))
    assert np.max(np.abs(b.mean(axis=0) - b_hat) / (sd / np.sqrt(n))) <= lim
    d = b - b_hat
    S = d.T @ d / n                                       # about the KNOWN mean: E[S] = C, var S_ij = (C_ii C_jj + C_ij^2) / n
    band = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / n)
    assert np.max(np.abs(S - C) / band) <= lim


def test_truncated_case_is_what_the_issue_describes():
    """Three faces cut the posterior of (8, 2): about 0.37 of the proposals survive and every coordinate's sd
    shrinks to 0.71 .. 0.89 of the uncut one."""
    cut, whole = ep.reference(ep.truncated_problem()), ep.reference(ep.problem(8, 2))
    assert abs(cut['rate'] - 0.37) < 0.01
    ratio = cut['sd'] / whole['sd']
    assert 0.70 < ratio.min() and ratio.max() < 0.90


# ---------------------------------------------------------------------------------------------------------------
# the draws of the contract
# ---------------------------------------------------------------------------------------------------------------

def _corr_T(x, y):
    """Sample correlation times sqrt(n): N(0, 1) for independent x, y."""
    x, y = np.ravel(x), np.ravel(y)
    return float(np.corrcoef(x, y)[0, 1] * np.sqrt(x.size))


@pytest.mark.parametrize('a', [2.0, 1.5])
@pytest.mark.parametrize('W', [4, 32, 33])
def test_draws_of_the_contract_follow_their_laws(W, a):
    """>= 2^18 draws of philox_stream (the device draw kernel is held to it bit for bit in
    test_philox_draw_kernel_matches_contract): zz has the CDF F(z) = (sqrt(a z) - 1) / (a - 1) on [1/a, a] -- the
    density 1/sqrt(z) of the stretch move --, -logu is Exp(1), the partner is uniform on the OTHER half and never
    in the walker's own, and zz is uncorrelated with logu, with the partner and with the next step's zz; ensembles of
    a batch do not share a stream.

    Levels: every correlation inside its own two-sided 1e-3 band.  The goodness-of-fit tests (two KS, two
    chi-square per case, six cases) share a family-wise 1e-3 as the features of a case do in t_limit: p >= 1e-3 / 24
    each.  A wrong law is nowhere near either level (z uniform on [1/a, a] gives a KS distance of 0.05 at a = 1.5
    and 0.08 at a = 2: p < 1e-250 at 2^18 draws).  Measured: the smallest p of the 24 is the KS of zz at W = 4,
    a = 2, 3.3e-4 (sqrt(n) D = 2.06); the same seed drawn eight times as long gives sqrt(n) D = 0.82, p = 0.51, and
    seven other seeds p = 0.07 .. 0.83 -- a deviation of the law would grow like sqrt(n) -- so that one is chance,
    and the family-wise level is what
    keeps 24 tests from failing by it."""
    from scipy import stats
    p_fit = 1e-3 / 24
    from bisip_amd.sampler import affine_splits
    from numpy_stretch_backend import philox_stream
    E, seed, step0 = 64, 0x5eed0000 + W, 3
    nh = (W + 1) // 2
    n = -(-(1 << 18) // (E * W)) + 1
    perm = affine_splits(seed, W, step0, n)
    s = {k: v.reshape(n, 2, E, nh) for k, v in philox_stream(W, 5, a, seed, step0, perm, E).items()}
    A, B = perm[:, 0].astype(np.int64), perm[:, 2].astype(np.int64)
    zz, logu, pos, zz_next = [], [], [], []
    for h in (0, 1):
        Ns, Nc = (nh, W // 2) if h == 0 else (W // 2, nh)
        act = s['active'][:, h, :, :Ns] - (np.arange(E) * W)[None, :, None]
        par = s['partner'][:, h, :, :Ns] - (np.arange(E) * W)[None, :, None]
        assert act.min() >= 0 and act.max() < W and par.min() >= 0 and par.max() < W      # inside its own ensemble
        # walker i belongs to half pi(i) & 1 with pi(i) = (A i + B) mod W (affine_splits)
        pi_act = (A[:, None, None] * act + B[:, None, None]) % W
        pi_par = (A[:, None, None] * par + B[:, None, None]) % W
        assert np.all(pi_act % 2 == h) and np.all(pi_par % 2 == 1 - h)                    # every partner: the other half
        assert np.array_equal(pi_act, np.broadcast_to(2 * np.arange(Ns) + h, pi_act.shape))
        r = (pi_par - (1 - h)) // 2
        assert r.min() >= 0 and r.max() < Nc
        counts = np.bincount(r.ravel(), minlength=Nc)
        assert stats.chisquare(counts).pvalue >= p_fit, (h, counts)
        z = s['zz'][:, h, :, :Ns]
        zz.append(z.ravel())
        logu.append(s['logu'][:, h, :, :Ns].ravel())
        pos.append((r.ravel() + 0.5) / Nc)
        zz_next.append((z[:-1].ravel(), z[1:].ravel()))
        assert np.array_equal(s['factor'][:, h, :, :Ns], (5 - 1.0) * np.log(z))
    zz, logu, pos = np.concatenate(zz), np.concatenate(logu), np.concatenate(pos)
    assert zz.size >= 1 << 18
    assert zz.min() >= 1 / a and zz.max() <= a
    assert stats.kstest(zz, lambda z: (np.sqrt(a * z) - 1) / (a - 1)).pvalue >= p_fit
    assert np.all(logu <= 0)
    assert stats.kstest(-logu, 'expon').pvalue >= p_fit
    lim = _normal_limit(1)
    fin = np.isfinite(logu)
    assert abs(_corr_T(zz[fin], logu[fin])) <= lim
    assert abs(_corr_T(zz, pos)) <= lim
    assert abs(_corr_T(np.concatenate([p[0] for p in zz_next]), np.concatenate([p[1] for p in zz_next]))) <= lim
    # ensembles: no two share a stream (and a batch of two is the first two of a batch of 64)
    z0 = s['zz'][:, 0, :, :nh]
    assert len({z0[:, e].tobytes() for e in range(E)}) == E
    assert abs(_corr_T(z0[:, 0], z0[:, 1])) <= lim
    two = philox_stream(W, 5, a, seed, step0, perm[:8], 2)['zz'].reshape(8, 2, 2, nh)
    assert np.array_equal(two, s['zz'][:8, :, :2]) and not np.array_equal(two[:, :, 0], two[:, :, 1])


# ---------------------------------------------------------------------------------------------------------------
# the contract is accepted, its mutants are rejected
# ---------------------------------------------------------------------------------------------------------------

def _whole_stream(W, ndim, a, seed, n_steps, E, chunk=50):
    from bisip_amd.sampler import affine_splits
    from numpy_stretch_backend import philox_stream
    parts = []
    for step0 in range(0, n_steps, chunk):
        n = min(chunk, n_steps - step0)
        parts.append(philox_stream(W, ndim, a, seed, step0, affine_splits(seed, W, step0, n), E))
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def contract_chain(prob, p0, stream, W, E, a, thin, mutant=None):
    """The stretch move of the contract (NumpyStretchBackend._slot / _commit) on ``stream``, all E ensembles at once,
    with the helper's logp.  ``mutant``: 'ndim' (factor = ndim log z), 'ndim-2' (factor = (ndim - 2) log z) or
    'uniform-z' (z uniform on [1/a, a], factor (ndim - 1) log z of that z).  Returns the chain (n / thin, E, W, ndim)."""
    ndim, nh = prob.ndim, (W + 1) // 2
    coords = np.array(p0, dtype=np.float64).reshape(E * W, ndim)
    lp = prob.logp(coords)
    n_steps = stream['zz'].shape[0]
    chain = np.empty((n_steps // thin, E * W, ndim))
    for k in range(n_steps):
        for h in (0, 1):
            Ns = nh if h == 0 else W // 2
            valid = (np.arange(E * nh) % nh) < Ns
            idx, par = stream['active'][k, h][valid], stream['partner'][k, h][valid]
            z, logu = stream['zz'][k, h][valid], stream['logu'][k, h][valid]
            if mutant == 'uniform-z':
                u = (np.sqrt(a * z) - 1.0) / (a - 1.0)
                z = 1.0 / a + u * (a - 1.0 / a)
            power = {None: ndim - 1.0, 'uniform-z': ndim - 1.0, 'ndim': float(ndim), 'ndim-2': ndim - 2.0}[mutant]
            factor = power * np.log(z)
            s, c = coords[idx], coords[par]
            q = c - (c - s) * z[:, None]
            new = prob.logp(q)
            acc = factor + new - lp[idx] > logu
            coords[idx[acc]] = q[acc]
            lp[idx[acc]] = new[acc]
        if (k + 1) % thin == 0:
            chain[k // thin] = coords
    return chain.reshape(-1, E, W, ndim)


def test_contract_is_accepted_and_its_mutants_are_rejected():
    """E = 64 ensembles of W = 16 walkers, every walker started at an exact draw of the truncated (8, 2) posterior,
    400 steps stored every 2, a = 2, one Philox stream for all four runs.  The contract keeps every feature within
    t_limit; a wrong exponent or a wrong z density exceeds it at least threefold.

    Measured (t_limit(64, 17) = 4.31, three times that 12.9): the contract max|T| = 1.67 (at a2); factor = ndim log z
    30.8; factor = (ndim - 2) log z 33.8; z uniform on [1/a, a] 28.2 -- each of the three at the indicator
    logp >= its 10 % quantile: a wrong exponent shows first in how far the ensemble spreads."""
    prob = ep.truncated_problem()
    ref = ep.reference(prob)
    E, W, n_steps, thin, a, seed = 64, 16, 400, 2, 2.0, 20240611
    p0, _ = prob.exact_draws(E * W, np.random.RandomState(11))
    stream = _whole_stream(W, prob.ndim, a, seed, n_steps, E)
    limit = ep.t_limit(E, ref['mean'].size)
    got = {}
    for mutant in (None, 'ndim', 'ndim-2', 'uniform-z'):
        chain = contract_chain(prob, p0, stream, W, E, a, thin, mutant)
        assert np.isfinite(prob.logp(chain)).all()                # no sample ever leaves the open box
        got[mutant] = ep.worst(prob.t_statistics(chain, ref), ref['names'])
        print(f'{mutant or "contract"}: max|T| = {got[mutant][0]:.2f} at {got[mutant][1]} (limit {limit:.2f})')
    assert got[None][0] <= limit, got
    for mutant in ('ndim', 'ndim-2', 'uniform-z'):
        assert got[mutant][0] >= 3 * limit, got
