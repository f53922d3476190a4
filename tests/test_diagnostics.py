"""The definitions of bisip_amd.diagnostics -- rank-normalised folded R-hat, the effective sample size and Monte-Carlo
error of the standard deviation, the posterior table -- without a GPU: against a second implementation written from the
formulas (tests/diagnostics_cases.py), on a known answer, on degenerate inputs, and the conditions that the inputs of
tests/test_gpu_diagnostics.py have to meet."""
import math
import os
import re

import numpy as np
import pytest

import diagnostics_cases as dc
import ess_cases as ec
import moments_bounds as mb
from bisip_amd import convergence as cv
from bisip_amd import diagnostics as dg
from bisip_amd import ess as es
from chain_harness import shape_id
from fitted import fitted_on_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bisip_chain_rank_normalize_folded_dev', 'bisip_chain_ess_squares_dev', 'bisip_chain_central_moments_dev')


# -- 1. an independent restatement --------------------------------------------------------------------------------------
# (n, W, rho): odd and even n, one walker (split: two chains), ties in parameter 1 (parameter 0 of a single one)
RESTATED = [(64, 6, (0.0, 0.5, 0.9)), (65, 6, (0.0, 0.5, 0.9)), (41, 1, (0.3, 0.7)), (40, 1, (0.6,)), (7, 31, (0.2, 0.8)),
            (200, 8, (0.0, 0.99))]


@pytest.mark.parametrize('n,W,rho', RESTATED, ids=lambda v: str(v).replace(' ', ''))
def test_against_a_second_implementation(n, W, rho):
    """z at Z_RTOL; R-hat at the tolerance diagnostics_cases derives from Z_RTOL and computes from the data; ess_sd at
    ESS_RTOL; mcse_sd at MCSE_RTOL while the difference of the two moments cancels fewer than three digits."""
    x = ec.ar1(np.random.default_rng(n * 31 + W), n, W, rho, ties=True)
    flat = x.reshape(-1, x.shape[2])
    if len(rho) > 1:
        assert np.unique(flat[:, 1]).size < flat.shape[0]                    # parameter 1 holds equal values
    for split in (True, False):
        if (2 if split else 1) * W >= 2:
            both, bulk, fold, z, zf = dc.second_rank_rhat(x, split)
            ec.assert_close(es.z_scale(x), z, ec.Z_RTOL, 'z')
            med = np.percentile(flat, 50, axis=0)
            ec.assert_close(es.z_scale(np.abs(x - med)), zf, ec.Z_RTOL, 'folded z')
            got = dg.rank_rhat(x, split, parts=True)
            tol_b, tol_f = dc.rhat_tolerance(z, 1, split)[0], dc.rhat_tolerance(zf, 1, split)[0]
            assert max(tol_b.max(), tol_f.max()) < 1e-9, 'the tolerance itself must stay small, else the inputs are wrong'
            dc.assert_rhat_close(got[1], bulk, tol_b, f'bulk split={split}')
            dc.assert_rhat_close(got[2], fold, tol_f, f'folded split={split}')
            dc.assert_rhat_close(got[0], both, np.maximum(tol_b, tol_f), f'rank_rhat split={split}')
            np.testing.assert_array_equal(dg.rank_rhat(x, split), got[0])
        else:
            with pytest.raises(ValueError, match='2 chains'):
                dg.rank_rhat(x, split)
        ec.assert_close(dg.ess_sd(x, split), dc.second_ess_sd(x, split), what=f'ess_sd split={split}')
        want, cancel = dc.second_mcse_sd(x, split)
        assert cancel.max() < 1e3
        ec.assert_close(dg.mcse_sd(x, split), want, dc.MCSE_RTOL, f'mcse_sd split={split}')
    np.testing.assert_array_equal(dg.ess_sd(x, center=flat.mean(axis=0)), dg.ess_sd(x))


# -- 2. known answer -----------------------------------------------------------------------------------------------------
def known_chain(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((200, 8, 3))
    x[:, 4:, 0] *= 3
    x[:, :, 1] = rng.standard_cauchy((200, 8))
    x[:, 0, 1] += 2
    return x


def test_known_answer():
    """Half the walkers three times as wide (parameter 0), a Cauchy posterior with one walker shifted by 2 (parameter 1),
    iid normal (parameter 2): the raw R-hat passes all three, the folded part catches the first and the bulk part the
    second.  The definitions give: raw <= 1.0002; folded 1.170 on parameter 0; bulk 1.0367 on parameter 1; 0.998 ... 0.999
    on parameter 2 (seeds 0 ... 2: raw <= 1.0015, folded 1.143 ... 1.170, bulk 1.0367 ... 1.0378, 0.997 ... 1.002)."""
    x = known_chain()
    raw = cv.rhat(x)
    both, bulk, fold = dg.rank_rhat(x, parts=True)
    print('raw', raw, 'rank', both, 'bulk', bulk, 'folded', fold)
    assert (raw < 1.01).all()
    assert both[0] > 1.1 and both[0] == fold[0] and fold[0] > bulk[0]
    assert both[1] > 1.02 and both[1] == bulk[1] and bulk[1] > fold[1]
    assert both[2] < 1.01
    N = x.shape[0] * x.shape[1]
    sd = np.std(x[:, :, 2], ddof=1)
    got = dg.mcse_sd(x)[2]
    print('mcse_sd', got, 'sd / sqrt(2 N)', sd / math.sqrt(2 * N))
    assert abs(got - sd / math.sqrt(2 * N)) <= 0.1 * sd / math.sqrt(2 * N)


def test_summary_and_its_table():
    x = known_chain(1)
    s = dg.summary(x, mass=0.9)
    assert tuple(s) == dg.SUMMARY_KEYS
    flat = x.reshape(-1, 3)
    np.testing.assert_array_equal(s['mean'], flat.mean(axis=0))
    np.testing.assert_array_equal(s['sd'], flat.std(axis=0, ddof=1))           # ddof = 1: not get_param_std's
    from bisip_amd.interval import hdi
    np.testing.assert_array_equal(np.stack([s['hdi_lo'], s['hdi_hi']]), hdi(flat, 0.9)[:, 0, :])
    np.testing.assert_array_equal(s['mcse_mean'], es.mcse_mean(x))
    np.testing.assert_array_equal(s['mcse_sd'], dg.mcse_sd(x))
    np.testing.assert_array_equal(s['ess_bulk'], es.ess(x, 'bulk'))
    np.testing.assert_array_equal(s['ess_tail'], es.ess(x, 'tail'))
    np.testing.assert_array_equal(s['r_hat'], dg.rank_rhat(x))
    text = dg.format_summary(s, names=['r0', 'm1', 'log_tau1'])
    lines = text.split('\n')
    assert len(lines) == 4 and lines[0].split() == list(dg.SUMMARY_KEYS)
    assert [ln.split()[0] for ln in lines[1:]] == ['r0', 'm1', 'log_tau1']
    assert all(len(ln.split()) == 1 + len(dg.SUMMARY_KEYS) for ln in lines[1:])
    assert len({len(ln) for ln in lines}) == 1                                  # fixed width
    assert lines[1].split()[1] == f'{s["mean"][0]:.3g}' and lines[3].split()[7] == f'{s["ess_bulk"][2]:.0f}'
    assert dg.format_summary(s, digits=5).split('\n')[2].split()[:2] == ['p1', f'{s["mean"][1]:.5g}']
    batch = {k: np.stack([v, 2 * v]) for k, v in s.items()}
    assert dg.format_summary(batch, spectrum=1).split('\n')[1].split()[1] == f'{2 * s["mean"][0]:.3g}'
    with pytest.raises(ValueError, match='spectrum'):
        dg.format_summary(batch)
    with pytest.raises(ValueError, match='spectrum'):
        dg.format_summary(s, spectrum=0)
    with pytest.raises(ValueError, match='names'):
        dg.format_summary(s, names=['a'])


# -- 3. conditions on the inputs of the GPU tests ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.COVER, ids=ec.cover_id)
def test_squares_of_the_cover_cases_sit_on_no_rounding_tie(case):
    for split in (True, False):
        _, gs, ge, lags = dc.cover_squares(case, split)
        print(case, split, 'smallest |even + odd|', np.nanmin(gs), 'smallest |even|', np.nanmin(ge), 'last lag', lags.max())
        ec.assert_margins(gs, ge, (case, split))


@pytest.mark.parametrize('case', [c for c in ec.COVER if dc.has_chains(c, True)], ids=ec.cover_id)
def test_both_parts_decide_in_the_cover_cases(case):
    """In every case with 16 or more (ensemble, parameter) pairs the folded part is the larger for some and the bulk part
    for others, so that a device that returned one of them only would not pass; the tolerance stays small everywhere."""
    E, ndim = case[0], case[2]
    for split in (True, False):
        if not dc.has_chains(case, split):
            continue
        both, bulk, fold, tol = dc.cover_rank_rhat(case, split)
        assert not np.isnan(both).any()
        n_fold = int((fold > bulk).sum())
        print(case, split, 'folded decides', n_fold, 'of', E * ndim, 'largest tolerance', tol.max())
        assert tol.max() < 1e-9
        if E * ndim >= 16:
            assert 0 < n_fold < E * ndim


# -- 4. degenerate inputs ----------------------------------------------------------------------------------------------------
def test_hand_built_chain():
    """NaN exactly where a parameter holds a value that is not finite, the middle sample of an odd n included (it is
    ranked; the squares' chains do not hold it); NaN for the constant parameter; a constant walker among moving ones
    gives a number."""
    x, nan_all, nan_ranked = ec.hand_built()
    E, ndim = nan_all.shape
    constant = np.zeros((E, ndim), dtype=bool)
    constant[E - 1, ndim - 1] = True
    for split in (True, False):
        both, bulk, fold = (np.stack(p) for p in zip(*[dg.rank_rhat(part, split, parts=True) for part in dc.ensembles(x, E)]))
        for got in (both, bulk, fold):
            np.testing.assert_array_equal(np.isnan(got), nan_ranked | constant)
        assert np.isfinite(both[0, 0])                                           # the constant walker among moving ones
        n_eff = dc.per_ensemble(dg.ess_sd, x, E, split)
        # the centre is the mean of ALL values: a NaN in the middle sample reaches every square
        np.testing.assert_array_equal(np.isnan(n_eff), nan_ranked)
        L = x.shape[0] // 2 if split else x.shape[0]
        assert n_eff[E - 1, ndim - 1] == L * (2 if split else 1) * (x.shape[1] // E)        # constant squares: S
        err = dc.per_ensemble(dg.mcse_sd, x, E, split)
        np.testing.assert_array_equal(np.isnan(err), nan_ranked | constant)
        s = dg.summary(dc.ensembles(x, E)[1], split=split)
        np.testing.assert_array_equal(np.isnan(s['r_hat']), nan_ranked[1])
    with pytest.raises(ValueError, match='center'):
        dg.ess_sd(x, center=np.zeros(ndim + 1))


def test_shapes_are_refused():
    for f in (dg.rank_rhat, dg.ess_sd, dg.mcse_sd, dg.summary):
        with pytest.raises(ValueError, match='unflattened'):
            f(np.zeros((40, 2)))
        with pytest.raises(ValueError, match='4 used samples'):
            f(np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match='2 chains'):
        dg.rank_rhat(np.zeros((8, 1, 2)), split=False)
    with pytest.raises(ValueError, match='2 per chain'):
        dg.ess_sd(np.zeros((1, 4, 2)), split=False)
    assert dg.ess_sd(np.random.default_rng(0).normal(size=(2, 1, 1)), split=False).shape == (1,)


@pytest.mark.parametrize('kw', [dict(discard=10), dict(discard=7, thin=3)], ids=str)
def test_inversion_methods_with_the_host_sampler(kw, capsys):
    m = fitted_on_host(60)
    chain, lp = m.get_chain(**kw), m._sampler.get_log_prob(**kw)
    for split in (True, False):
        np.testing.assert_array_equal(m.get_rank_rhat(split=split, **kw), dg.rank_rhat(chain, split))
        np.testing.assert_array_equal(m.get_ess_sd(split=split, **kw), dg.ess_sd(chain, split))
        np.testing.assert_array_equal(m.get_mcse_sd(split=split, **kw), dg.mcse_sd(chain, split))
        assert m.get_log_prob_rank_rhat(split=split, **kw) == dg.rank_rhat(lp[:, :, None], split)[0]
    got = m.get_rank_rhat(parts=True, **kw)
    assert len(got) == 3 and all(g.shape == (chain.shape[2],) for g in got)
    np.testing.assert_array_equal(m.get_rank_rhat(chain=chain), dg.rank_rhat(chain))
    s, want = m.get_summary(0.9, **kw), dg.summary(chain, 0.9)
    assert tuple(s) == dg.SUMMARY_KEYS
    for k in dg.SUMMARY_KEYS:
        np.testing.assert_array_equal(s[k], want[k], err_msg=k)
    N = chain[:, :, 0].size
    np.testing.assert_allclose(s['sd'], m.get_param_std(**kw) * np.sqrt(N / (N - 1.0)), rtol=1e-14)      # ddof = 1
    capsys.readouterr()
    m.print_summary(0.9, **kw)
    assert capsys.readouterr().out == dg.format_summary(want, m.param_names) + '\n'
    assert 'get_rank_rhat' in type(m).get_rhat.__doc__


def test_the_advice_about_discard_is_given_once():
    import warnings
    m = fitted_on_host(60)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        m.get_summary()
    assert len([w for w in caught if 'No samples were discarded' in str(w.message)]) == 1
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        m.get_summary(discard=10)
        m.get_summary(chain=m.get_chain())
    assert not [w for w in caught if 'No samples were discarded' in str(w.message)]


@pytest.mark.parametrize('method', ['get_rank_rhat', 'get_log_prob_rank_rhat', 'get_ess_sd', 'get_mcse_sd', 'get_summary'])
def test_inversion_refusals(method):
    m = fitted_on_host(60)
    f = getattr(m, method)
    with pytest.raises(ValueError, match='no samples'):
        f(discard=60)
    with pytest.raises(TypeError, match='flat'):
        f(flat=True)
    with pytest.raises(TypeError, match='unexpected keyword'):
        f(bins=3)
    with pytest.raises(ValueError, match='4 used samples'):
        f(discard=57)                                           # 3 used samples: halves of one
    if method != 'get_log_prob_rank_rhat':
        with pytest.raises(ValueError, match='unflattened'):
            f(chain=m.get_chain(flat=True))                     # a flat chain
        with pytest.raises(ValueError, match='Do not pass both'):
            f(chain=m.get_chain(), discard=5)                   # refuse_discard_of_a_chain


class _HostChainSampler:
    """What SpectraBatch asks of its sampler, answered from a host chain (n, E, Wp, ndim) by the definitions."""

    def __init__(self, chain, lp):
        self.chain, self.lp = chain, lp

    def _each(self, f, discard, thin, *args):
        c = self.chain[discard + thin - 1::thin]
        return [f(c[:, e], *args) for e in range(c.shape[1])]

    def param_rank_rhat(self, discard=0, thin=1, split=True, parts=False):
        got = self._each(dg.rank_rhat, discard, thin, split, parts)
        return tuple(np.stack(p) for p in zip(*got)) if parts else np.stack(got)

    def log_prob_rank_rhat(self, discard=0, thin=1, split=True):
        lp = self.lp[discard + thin - 1::thin]
        return np.stack([dg.rank_rhat(lp[:, e, :, None], split)[0] for e in range(lp.shape[1])])

    def param_ess_sd(self, discard=0, thin=1, split=True):
        return np.stack(self._each(dg.ess_sd, discard, thin, split))

    def param_mcse_sd(self, discard=0, thin=1, split=True):
        return np.stack(self._each(dg.mcse_sd, discard, thin, split))

    def param_summary(self, mass=0.95, discard=0, thin=1, split=True):
        rows = self._each(dg.summary, discard, thin, mass, split)
        return {k: np.stack([r[k] for r in rows]) for k in dg.SUMMARY_KEYS}


def test_spectra_batch_methods_on_a_host_chain(capsys):
    from bisip_amd.batch import SpectraBatch
    rng = np.random.default_rng(8)
    chain, lp = rng.normal(size=(30, 3, 6, 4)), rng.normal(size=(30, 3, 6))
    b = SpectraBatch.__new__(SpectraBatch)
    b._fitted = lambda: _HostChainSampler(chain, lp)
    b.params = {name: [0, 1] for name in 'abcd'}
    kw = dict(discard=4, thin=2)
    used = chain[5::2]
    assert b.get_rank_rhat(**kw).shape == (3, 4) and b.get_log_prob_rank_rhat(**kw).shape == (3,)
    assert len(b.get_rank_rhat(parts=True, **kw)) == 3
    np.testing.assert_array_equal(b.get_rank_rhat(split=False, **kw)[1], dg.rank_rhat(used[:, 1], split=False))
    np.testing.assert_array_equal(b.get_ess_sd(**kw)[2], dg.ess_sd(used[:, 2]))
    np.testing.assert_array_equal(b.get_mcse_sd(**kw)[0], dg.mcse_sd(used[:, 0]))
    s = b.get_summary(0.8, **kw)
    assert tuple(s) == dg.SUMMARY_KEYS and all(v.shape == (3, 4) for v in s.values())
    np.testing.assert_array_equal(s['r_hat'][2], dg.rank_rhat(used[:, 2]))
    capsys.readouterr()
    b.print_summary(2, 0.8, **kw)
    assert capsys.readouterr().out == dg.format_summary(s, list('abcd'), spectrum=2) + '\n'


# -- 5. the ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_exist(hip_lib):
    from __graft_entry__ import header_abi_version
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    for name in NAMES + ('bisip_chain_central_moments_workspace',):
        assert hasattr(hip_lib, name)
        assert re.search(r'\b%s\(' % name, header)
        assert re.search(r'\b%s;' % name, exports)
        assert callable(getattr(_hip, name[len('bisip_'):]))
    assert hip_lib.bisip_abi_version() == header_abi_version() == 6          # symbols were only added
    assert es.KINDS == ('bulk', 'tail', 'mean')
    with pytest.raises(ValueError, match='kind'):
        es.ess(np.zeros((8, 4, 2)), kind='median')


def test_entry_points_check_their_arguments():
    from bisip_amd import _hip
    from bisip_amd.chainview import moment_splits
    # the pointers are never dereferenced: every call below is refused on the host
    P = 4096

    def fold(chain=P, n=8, stride=24, E=1, Wp=8, ndim=3, center=P, z=P, work=P, nbytes=1 << 20):
        _hip.chain_rank_normalize_folded_dev(chain, n, stride, E, Wp, ndim, center, z, work, nbytes, 0)

    def squares(chain=P, n=8, stride=24, E=1, Wp=8, ndim=3, splits=2, center=P, out=P, work=P, nbytes=1 << 20):
        _hip.chain_ess_squares_dev(chain, n, stride, E, Wp, ndim, splits, center, out, work, nbytes, 0)

    def central(chain=P, n=8, stride=24, E=1, Wp=8, ndim=3, center=P, m2=P, m4=P, work=P):
        _hip.chain_central_moments_dev(chain, n, stride, E, Wp, ndim, center, m2, m4, work, 0)

    for call, pointers in ((fold, ('chain', 'center', 'z', 'work')), (squares, ('chain', 'center', 'out', 'work')),
                           (central, ('chain', 'center', 'm2', 'm4', 'work'))):
        for name in pointers:
            with pytest.raises(ValueError, match='null'):
                call(**{name: 0})
        with pytest.raises(ValueError, match='ndim'):
            call(ndim=17, stride=8 * 17)
        with pytest.raises(ValueError, match='bad chain shape'):
            call(Wp=0)
        with pytest.raises(ValueError, match='sample_stride'):
            call(stride=23)
    for splits in (0, 3):
        with pytest.raises(ValueError, match='splits'):
            squares(splits=splits)
    with pytest.raises(ValueError, match='2 samples'):
        squares(n=3)
    with pytest.raises(ValueError, match='2 samples'):
        squares(n=1, splits=1)
    with pytest.raises(ValueError, match='workspace'):
        squares(nbytes=_hip.chain_ess_workspace(8, 1, 8, 3, 2) - 1)
    with pytest.raises(ValueError, match='workspace'):
        fold(nbytes=_hip.chain_rank_normalize_workspace(8, 1, 8, 3) - 1)
    with pytest.raises(RuntimeError, match='2\\^31'):
        fold(n=1 << 20, E=1 << 10, stride=(1 << 10) * 8 * 3)
    for n, E, ndim in [(500, 8, 7), (3, 5000, 2), (1, 1, 1)]:
        assert _hip.chain_central_moments_workspace(n, E, ndim) == 2 * _hip.chain_moments_workspace(n, E, ndim) \
            == 2 * E * moment_splits(n, E) * ndim
    assert _hip.chain_central_moments_workspace(0, 1, 1) == 0


# -- 6. the order of the central moments ---------------------------------------------------------------------------------------
SMALL_MIRRORED = [s for s in mb.MIRRORED if s[0] * s[1] * s[2] * s[3] <= 20000]


@pytest.mark.parametrize('shape', SMALL_MIRRORED, ids=shape_id)
def test_ordered_central_moments_within_the_bound(shape):
    """The NumPy restatement of bisip_chain_central_moments_dev's order against the long-double evaluation: relative
    error at most (N + 3) u and (N + 7) u (tests/diagnostics_cases.py), NaN / inf as IEEE has them; and a column of plain
    values against math.fsum."""
    n, E, Wp, ndim = shape
    x, c = mb.case(*shape)['x'], dc.central_center(shape)
    m2, m4 = dc.central_ordered(shape)
    ref = dc.central_reference(x, c, E)
    worst = dc.assert_central_within_bounds(m2, m4, ref, str(shape))
    print(shape, 'checked', int(ref['checked'].sum()), 'of', ref['checked'].size, 'worst error / bound', worst)
    assert ref['checked'][0, 0] or n * Wp == 1           # parameter 0 of ensemble 0 is finite (one value: both moments 0)
    v = mb.per_ensemble(x, E)[0, :, 0]
    d = v - c[0, 0]                                       # (rounded once, as the kernel's: in the bound)
    N = v.size
    exact2, exact4 = math.fsum(d * d) / N, math.fsum((d * d) * (d * d)) / N
    assert abs(m2[0, 0] - exact2) <= (N + 3) * mb.U * exact2 and abs(m4[0, 0] - exact4) <= (N + 7) * mb.U * exact4
    bad = ~np.isfinite(mb.per_ensemble(x, E)).all(axis=1) | ~np.isfinite(c)
    assert not np.isfinite(m2[bad]).any() and not np.isfinite(m4[bad]).any()


def test_ordered_moments_keep_their_bits_after_sharing_the_sweep():
    """chainview.ordered_moments now runs on ordered_sweep: on a shape with left-over samples, several splits and fewer
    doubles than lanes it still gives what its stated order gives when written out sample by sample."""
    from bisip_amd.chainview import exact_fma, moment_splits, ordered_moments
    rng = np.random.default_rng(3)
    n, E, Wp, ndim = 11, 2, 3, 2
    x = rng.normal(size=(n, E * Wp, ndim)) * [1.0, 1e-3] + [0.0, 1e3]
    mean, std = ordered_moments(x, E)
    splits = moment_splits(n, E)
    assert splits == 2
    for e in range(E):
        for q in range(ndim):
            for second in (False, True):
                total = 0.0
                for sp in range(splits):
                    s0, s1 = n * sp // splits, n * (sp + 1) // splits
                    part = 0.0
                    for w in range(Wp):                                  # lane w * ndim + q holds walker w
                        acc = [0.0] * 4
                        for s in range(s0, s1):
                            j = (s - s0) % 4 if s - s0 < (s1 - s0) // 4 * 4 else 0
                            v = x[s, e * Wp + w, q]
                            acc[j] = exact_fma(v - mean[e, q], v - mean[e, q], acc[j]) if second else acc[j] + v
                        part = part + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
                    total = total + part
                got = math.sqrt(total / (float(n) * Wp)) if second else total / (float(n) * Wp)
                assert got == (std if second else mean)[e, q]
