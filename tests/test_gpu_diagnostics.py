"""Rank-normalised folded R-hat, the effective sample size and Monte-Carlo error of the standard deviation and the
posterior table on the device (bisip_chain_rank_normalize_folded_dev, bisip_chain_ess_squares_dev,
bisip_chain_central_moments_dev), from the C entry points up to the model and SpectraBatch methods.

The three transforms are applied where the chain is read, so each entry point is held BIT FOR BIT to its neighbour run on an
upload of NumPy's transformed chain (the same IEEE operations on both sides), the central moments to the NumPy restatement of
their order, and R-hat of z to ``convergence.ordered_rhat`` of the device's own z.  Against the definitions: ``Z_RTOL`` for z,
``ESS_RTOL`` for every effective sample size under the margins of tests/ess_cases.py, the tolerance that
tests/diagnostics_cases.py derives from ``Z_RTOL`` for R-hat, and its first-order bound for the central moments.
tests/test_diagnostics.py checks the conditions on the generated inputs without a GPU."""
import functools

import numpy as np
import pytest

import diagnostics_cases as dc
import ess_cases as ec
import fitted
import moments_bounds as mb
from bisip_amd import convergence as cv
from bisip_amd import diagnostics as dg
from bisip_amd import ess as es
from chain_harness import SENTINEL, GuardedCall, shape_id, store, used_window
from convergence_bounds import U

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, want, what=''):
    """The same bits everywhere: the finite values, the infinities and where NaN stands."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok], err_msg=what)


def on_device(case):
    """The stored chain of a COVER case on the device and how its used samples are read: ``(tensor, offset, stride)`` in
    doubles; what lies between the used samples, and after each, is NaN."""
    import torch
    E, Wp, ndim, n, discard, thin = case
    stored = ec.cover_case(*case)[0]
    offset, stride, used = used_window(stored.shape[0], stored.shape[1], discard, thin)
    assert used == n
    return torch.from_numpy(stored.copy()).cuda(), offset, stride


def upload(x):
    """A contiguous chain (n, W, ndim) on the device: ``(tensor, 0, W * ndim)``."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda(), 0, x.shape[1] * x.shape[2]


def run_rank(src, n, E, Wp, ndim, center=None):
    """One bisip_chain_rank_normalize_dev call, or with ``center (E, ndim)`` one of its folded sibling."""
    import torch
    from bisip_amd import _hip
    t, offset, stride = src
    nbytes = _hip.chain_rank_normalize_workspace(n, E, Wp, ndim)
    assert nbytes > 0
    call = GuardedCall()
    z = call.out('z', (n, E * Wp, ndim))
    if center is None:
        _hip.chain_rank_normalize_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, z, call.work(nbytes), nbytes,
                                      call.stream)
    else:
        c = torch.from_numpy(np.ascontiguousarray(center)).cuda()
        _hip.chain_rank_normalize_folded_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, c.data_ptr(), z,
                                             call.work(nbytes), nbytes, call.stream)
    res = call.finish()[0]
    assert not (res == SENTINEL).any()
    return res


def run_ess(src, n, E, Wp, ndim, splits, center=None):
    """One bisip_chain_ess_dev call without thresholds, or with ``center (E, ndim)`` one of bisip_chain_ess_squares_dev."""
    import torch
    from bisip_amd import _hip
    t, offset, stride = src
    nbytes = _hip.chain_ess_workspace(n, E, Wp, ndim, splits, 0)
    assert nbytes > 0
    call = GuardedCall()
    out = call.out('the effective sample sizes', (E, ndim))
    if center is None:
        _hip.chain_ess_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, splits, 0, 0, out, call.work(nbytes), nbytes,
                           call.stream)
    else:
        c = torch.from_numpy(np.ascontiguousarray(center)).cuda()
        _hip.chain_ess_squares_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, splits, c.data_ptr(), out,
                                   call.work(nbytes), nbytes, call.stream)
    res = call.finish()[0]
    assert not (res == SENTINEL).any()
    return res


def run_central(x, E, center, **storage):
    """One bisip_chain_central_moments_dev call on x (n, E * Wp, ndim) through store(x, **storage); the workspace holds
    exactly chain_central_moments_workspace() doubles."""
    import torch
    from bisip_amd import _hip
    n, W, ndim = x.shape
    stored, offset, stride = store(x, **storage)
    t = torch.from_numpy(stored).cuda()
    c = torch.from_numpy(np.ascontiguousarray(center)).cuda()
    call = GuardedCall()
    m2, m4 = call.out('the second moment', (E, ndim)), call.out('the fourth moment', (E, ndim))
    doubles = _hip.chain_central_moments_workspace(n, E, ndim)
    _hip.chain_central_moments_dev(t.data_ptr() + 8 * offset, n, stride, E, W // E, ndim, c.data_ptr(), m2, m4,
                                   call.work(8 * doubles), call.stream)
    m2, m4 = call.finish()
    assert not (m2 == SENTINEL).any() and not (m4 == SENTINEL).any()
    return m2, m4


# -- 1. the folded rank pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.COVER, ids=ec.cover_id)
def test_folded_rank_pass(case):
    """On the stored chain (offset, stride, NaN padding) about np.percentile's medians: the bits of the plain pass on an
    upload of NumPy's ``np.abs(x - c)``; the definition's z at Z_RTOL; the same bits on a second call."""
    E, Wp, ndim, n = case[:4]
    used = ec.cover_case(*case)[1]
    c = dc.medians(used, E)
    src = on_device(case)
    got = run_rank(src, n, E, Wp, ndim, c)
    assert_bits(got, run_rank(upload(dc.folded(used, E, c)), n, E, Wp, ndim), f'{case}: the plain pass on the folded chain')
    ec.assert_close(got, dc.cover_z(case)[1], ec.Z_RTOL, f'{case} folded z')
    assert_bits(run_rank(src, n, E, Wp, ndim, c), got, f'{case}: a second call')


def test_folded_rank_pass_on_the_hand_built_chain():
    """A NaN centre, an infinite centre and values that are not finite (the middle sample of an odd n among them) blank
    their own (ensemble, parameter) and no other."""
    x, _, nan_ranked = ec.hand_built()
    n, W, ndim = x.shape
    E = nan_ranked.shape[0]
    Wp = W // E
    c = dc.medians(x, E)
    np.testing.assert_array_equal(np.isnan(c), np.isnan(x).reshape(n, E, Wp, ndim).any(axis=(0, 2)))
    c[0, 3], c[2, 0] = np.nan, np.inf
    blank = nan_ranked.copy()
    blank[0, 3] = blank[2, 0] = True
    got = run_rank(upload(x), n, E, Wp, ndim, c)
    z = got.reshape(n, E, Wp, ndim)
    np.testing.assert_array_equal(np.isnan(z).any(axis=(0, 2)), blank)
    np.testing.assert_array_equal(np.isnan(z).all(axis=(0, 2)), blank)
    ec.assert_close(got, dc.z_of(dc.folded(x, E, c), E), ec.Z_RTOL, 'hand-built folded z')
    assert_bits(got, run_rank(upload(dc.folded(x, E, c)), n, E, Wp, ndim), 'hand-built: the plain pass on the folded chain')


# -- 2. the effective sample size of the squares ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.COVER, ids=ec.cover_id)
def test_squares_ess(case):
    """About np.mean's centres: the bits of bisip_chain_ess_dev on an upload of NumPy's ``(x - c) * (x - c)``, split and
    unsplit; ``ess_sd(x, center=c)`` at ESS_RTOL; a NaN centre gives NaN there and changes nothing else."""
    E, Wp, ndim, n = case[:4]
    used = ec.cover_case(*case)[1]
    c = dc.means(used, E)
    src, sq = on_device(case), upload(dc.squares(used, E, c))
    for split in (True, False):
        splits = 2 if split else 1
        want, gs, ge, lags = dc.cover_squares(case, split)
        ec.assert_margins(gs, ge, (case, split))
        got = run_ess(src, n, E, Wp, ndim, splits, c)
        assert_bits(got, run_ess(sq, n, E, Wp, ndim, splits), f'{case} split={split}: the plain call on the squares')
        ec.assert_close(got, want, what=f'{case} squares split={split} (last lag {int(lags.max())})')
        if E * Wp * ndim * n <= 50000:            # the definition as the issue names it, where that takes no time
            direct = np.stack([dg.ess_sd(p, split, center=c[e]) for e, p in enumerate(dc.ensembles(used, E))])
            np.testing.assert_array_equal(direct, want)
        planted = c.copy()
        planted[E - 1, ndim - 1] = np.nan
        again = run_ess(src, n, E, Wp, ndim, splits, planted)
        assert np.isnan(again[E - 1, ndim - 1])
        again[E - 1, ndim - 1] = got[E - 1, ndim - 1]
        assert_bits(again, got, f'{case} split={split}: beside the NaN centre')


# -- 3. the central moments -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', mb.SHAPES, ids=shape_id)
def test_central_moments(shape):
    """The bits of the NumPy restatement where the shape has one (MIRRORED), the first-order bound of the long-double
    evaluation on every shape, the same bits through other storage of the same used samples."""
    n, E, Wp, ndim = shape
    x, c = mb.case(*shape)['x'], dc.central_center(shape)
    m2, m4 = run_central(x, E, c)
    if shape in mb.MIRRORED:
        want2, want4 = dc.central_ordered(shape)
        mb.assert_same_bits(m2, want2, 'the second moment')
        mb.assert_same_bits(m4, want4, 'the fourth moment')
    ref = dc.central_reference(x, c, E)
    worst = dc.assert_central_within_bounds(m2, m4, ref, str(shape))
    varies = np.ptp(mb.per_ensemble(x, E)[:, :, 0], axis=1) > 0      # (one walker, and that one constant: both moments 0)
    assert ref['checked'][varies, 0].all()                           # parameter 0 stays finite: held to the bound
    print(f'shape {shape}: error at most {worst:.3f} of its bound; {int(ref["checked"].sum())} of {E * ndim} held to it')
    bad = ~np.isfinite(mb.per_ensemble(x, E)).all(axis=1) | ~np.isfinite(c)
    assert not np.isfinite(m2[bad]).any() and not np.isfinite(m4[bad]).any()
    for kw in ({}, dict(discard=0, thin=1, pad=0), dict(discard=3, thin=4, pad=11)):
        a2, a4 = run_central(x, E, c, **kw)
        assert_bits(a2, m2, str(kw))
        assert_bits(a4, m4, str(kw))


# -- 4. R-hat of the ranks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in ec.COVER if dc.has_chains(c, True)], ids=ec.cover_id)
def test_rank_rhat(case):
    """R-hat of the device's own z, plain and folded, has the bits of convergence.ordered_rhat of that z; device_rank_rhat
    returns them, the larger as the definition takes it; all three lie within the tolerance of the definition."""
    import torch
    from bisip_amd.chainview import ChainView, device_percentiles
    E, Wp, ndim, n = case[:4]
    t, offset, stride = on_device(case)
    view = ChainView(t.reshape(-1), n, E, Wp, ndim, offset=offset, stride=stride)
    med = device_percentiles(view, (50.0,))[0]
    np.testing.assert_array_equal(med, dc.medians(ec.cover_case(*case)[1], E))            # NumPy's own doubles
    for split in (True, False):
        if not dc.has_chains(case, split):
            with pytest.raises(ValueError, match='2 chains'):
                dg.device_rank_rhat(view, split)
            continue
        parts = []
        for center in (None, med):
            zv = es.device_rank_normalize(view, center=center)
            got = cv.device_rhat(zv, split=split)
            assert_bits(got, cv.ordered_rhat(zv.tensor.cpu().numpy(), split, n_ensembles=E)[2], f'{case} split={split}')
            parts.append(got)
            del zv
        both, bulk, fold = dg.device_rank_rhat(view, split, parts=True)
        assert_bits(bulk, parts[0], 'the bulk part')
        assert_bits(fold, parts[1], 'the folded part')
        assert_bits(both, np.maximum(bulk, fold), 'the larger')
        assert_bits(dg.device_rank_rhat(view, split), both, 'without parts')
        w_both, w_bulk, w_fold, tol = dc.cover_rank_rhat(case, split)
        dc.assert_rhat_close(bulk, w_bulk, tol, f'{case} bulk split={split}')
        dc.assert_rhat_close(fold, w_fold, tol, f'{case} folded split={split}')
        dc.assert_rhat_close(both, w_both, tol, f'{case} rank_rhat split={split}')
    del t, view
    torch.cuda.empty_cache()


def test_folded_pass_by_pass_of_ensembles(monkeypatch):
    """device_rank_normalize in passes of one ensemble each: every pass takes its own rows of the centres, and the z has
    the bits of the single pass."""
    from bisip_amd.chainview import ChainView
    case = (3, 300, 7, 65, 1, 2)
    E, Wp, ndim, n = case[:4]
    t, offset, stride = on_device(case)
    view = ChainView(t.reshape(-1), n, E, Wp, ndim, offset=offset, stride=stride)
    c = dc.medians(ec.cover_case(*case)[1], E)
    whole = es.device_rank_normalize(view, center=c).tensor.cpu().numpy()
    assert_bits(whole, run_rank((t, offset, stride), n, E, Wp, ndim, c), 'one pass')
    monkeypatch.setattr(es, 'RANK_PASS_BYTES', n * Wp * ndim * 8)
    assert_bits(es.device_rank_normalize(view, center=c).tensor.cpu().numpy(), whole, 'three passes')
    with pytest.raises(ValueError, match='center'):
        es.device_rank_normalize(view, center=c[:2])


def test_drivers_on_the_hand_built_chain():
    """NaN where the definition has it -- a value that is not finite, the constant parameter -- through the drivers, and
    a device tensor routed there by the definitions themselves."""
    import torch
    from bisip_amd.chainview import ChainView
    x, _, nan_ranked = ec.hand_built()
    n, W, ndim = x.shape
    E = nan_ranked.shape[0]
    Wp = W // E
    view = ChainView(torch.from_numpy(x).cuda(), n, E, Wp, ndim)
    constant = np.zeros((E, ndim), dtype=bool)
    constant[E - 1, ndim - 1] = True
    for split in (True, False):
        both, bulk, fold, tol = dc.rank_rhat_definition(x, E, split)
        np.testing.assert_array_equal(np.isnan(both), nan_ranked | constant)
        got = dg.device_rank_rhat(view, split, parts=True)
        for g, w in zip(got, (both, bulk, fold)):
            dc.assert_rhat_close(g, w, tol, f'hand-built split={split}')
        want = dc.per_ensemble(dg.ess_sd, x, E, split)
        ec.assert_margins(*dc_margins(x, E, split), ('hand-built', split))
        ec.assert_close(dg.device_ess_sd(view, split), want, what=f'hand-built ess_sd split={split}')
        err = dg.device_mcse_sd(view, split)
        np.testing.assert_array_equal(np.isnan(err), nan_ranked | constant)
        ec.assert_close(err, dc.per_ensemble(dg.mcse_sd, x, E, split), dc.MCSE_RTOL, f'hand-built mcse_sd split={split}')
    one = x[:, Wp:2 * Wp]
    t = torch.from_numpy(np.ascontiguousarray(one)).cuda()
    both, bulk, fold, tol = dc.rank_rhat_definition(one, 1, True)
    dc.assert_rhat_close(dg.rank_rhat(t), both[0], tol[0], 'a device tensor')
    ec.assert_close(dg.ess_sd(t), dg.ess_sd(one), what='ess_sd of a device tensor')
    ec.assert_close(dg.mcse_sd(t), dg.mcse_sd(one), dc.MCSE_RTOL, 'mcse_sd of a device tensor')
    s = dg.summary(t)
    assert tuple(s) == dg.SUMMARY_KEYS and all(v.shape == (ndim,) for v in s.values())


def dc_margins(x, E, split):
    """The decision margins of the squares series of ``x`` about np.mean."""
    _, gs, ge, _ = ec.definition_of_series(dc.squares(x, E, dc.means(x, E)), E, split)
    return gs, ge


# -- 5. the methods ---------------------------------------------------------------------------------------------------------
def check_against_definitions(chain, lp, E, get, label):
    """chain (n, E * Wp, ndim), lp (n, E * Wp): ``get(name, **kw)`` is the method ``name`` of a model or a batch.  The
    centre the device uses is device_moments' mean, not np.mean: a few ulp apart, which moves the squares by at most 2 u
    |m| / sd relative -- first order, many orders below ESS_RTOL."""
    n, W, ndim = chain.shape
    N = n * (W // E)
    for split in (True, False):
        both, bulk, fold, tol = dc.rank_rhat_definition(chain, E, split)
        got = get('get_rank_rhat', split=split, parts=True)
        for g, w, name in zip(got, (both, bulk, fold), ('rank_rhat', 'bulk', 'folded')):
            dc.assert_rhat_close(np.reshape(g, (E, ndim)), w, tol, f'{label} {name} split={split}')
        assert_bits(get('get_rank_rhat', split=split), got[0])
        both, _, _, tol = dc.rank_rhat_definition(lp[:, :, None], E, split)
        dc.assert_rhat_close(np.reshape(get('get_log_prob_rank_rhat', split=split), (E, 1)), both, tol,
                             f'{label} log-probability split={split}')
        ec.assert_margins(*dc_margins(chain, E, split), (label, split))
        ec.assert_close(np.reshape(get('get_ess_sd', split=split), (E, ndim)), dc.per_ensemble(dg.ess_sd, chain, E, split),
                        what=f'{label} ess_sd split={split}')
        cancel = np.stack([dc.second_mcse_sd(p, split)[1] for p in dc.ensembles(chain, E)])
        assert cancel.max() * 2 * (N + 7) * U <= 5e-11          # the moments' bound, magnified, leaves half of MCSE_RTOL
        ec.assert_close(np.reshape(get('get_mcse_sd', split=split), (E, ndim)), dc.per_ensemble(dg.mcse_sd, chain, E, split),
                        dc.MCSE_RTOL, f'{label} mcse_sd split={split}')


def check_summary(summary, get, E, ndim, N, mass, bitwise_moments=True):
    """Every entry of a summary against the getter that gives the same quantity: to the bit, the same entry point being
    behind both.  ``bitwise_moments=False``: the getter of the mean and the standard deviation works in NumPy (a batch with
    a host chain), so those two are compared in check_moments instead."""
    assert tuple(summary) == dg.SUMMARY_KEYS and all(np.shape(v) == ((E, ndim) if E > 1 else (ndim,)) for v in summary.values())
    if bitwise_moments:
        assert_bits(summary['mean'], get('get_param_mean'), 'mean')
        assert_bits(summary['sd'], get('get_param_std') * np.sqrt(N / (N - 1.0)), 'sd')
    lo, hi = get('get_param_hdi', mass)
    assert_bits(summary['hdi_lo'], lo, 'hdi_lo')
    assert_bits(summary['hdi_hi'], hi, 'hdi_hi')
    assert_bits(summary['mcse_mean'], get('get_mcse_mean'), 'mcse_mean')
    assert_bits(summary['mcse_sd'], get('get_mcse_sd'), 'mcse_sd')
    assert_bits(summary['ess_bulk'], get('get_ess', 'bulk'), 'ess_bulk')
    assert_bits(summary['ess_tail'], get('get_ess', 'tail'), 'ess_tail')
    assert_bits(summary['r_hat'], get('get_rank_rhat'), 'r_hat')


@functools.lru_cache(maxsize=None)
def fitted_model():
    return fitted.fitted_model('device', nsteps=120)


def test_model_methods(capsys):
    import warnings
    m = fitted_model()
    for used in (dict(discard=40, thin=2), dict(discard=60)):
        chain, lp = m.get_chain(**used), m._sampler.get_log_prob(**used)
        n, W, ndim = chain.shape

        def get(name, *args, **kw):
            return getattr(m, name)(*args, **kw, **used)

        check_against_definitions(chain, lp, 1, get, f'model {used}')
        assert isinstance(m.get_log_prob_rank_rhat(**used), float)
        check_summary(m.get_summary(0.9, **used), get, 1, ndim, n * W, 0.9)
        assert_bits(m.get_summary(**used)['hdi_lo'], m.get_param_hdi(**used)[0], 'the default mass')
    capsys.readouterr()
    m.print_summary(discard=60)
    assert capsys.readouterr().out == dg.format_summary(m.get_summary(discard=60), m.param_names) + '\n'
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        m.get_summary()
    assert len([w for w in caught if 'No samples were discarded' in str(w.message)]) == 1
    with pytest.raises(ValueError, match='no samples'):
        m.get_rank_rhat(discard=120)
    with pytest.raises(ValueError, match='4 used samples'):
        m.get_summary(discard=117)
    with pytest.raises(ValueError, match='unflattened'):
        m.get_rank_rhat(chain=m.get_chain(flat=True))
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_mcse_sd(chain=m.get_chain(), discard=5)
    np.testing.assert_array_equal(m.get_rank_rhat(chain=m.get_chain(discard=60)), dg.rank_rhat(m.get_chain(discard=60)))


@functools.lru_cache(maxsize=None)
def fitted_batch(where):
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    spectra = [bisip_amd.DataFiles()['SIP-K389175']] + [synthetic_columns(20, i) for i in range(2)]
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=32, nsteps=160, poly_deg=2)
    np.random.seed(5)
    b.fit(seed=11, chain=where)
    return b


@pytest.mark.parametrize('where', ['device', 'host'])
def test_spectra_batch_methods(where, capsys):
    b = fitted_batch(where)
    E, Wp, ndim = 3, 32, b.ndim
    for used in (dict(discard=60), dict(discard=40, thin=2)):
        chain, lp = b.get_chain(**used), b.get_log_prob(**used)              # (n, E, Wp, ndim), (n, E, Wp)
        n = chain.shape[0]
        chain, lp = chain.reshape(n, E * Wp, ndim), lp.reshape(n, E * Wp)

        def get(name, *args, **kw):
            return getattr(b, name)(*args, **kw, **used)

        assert b.get_rank_rhat(**used).shape == (E, ndim) and b.get_log_prob_rank_rhat(**used).shape == (E,)
        assert b.get_ess_sd(**used).shape == (E, ndim) and b.get_mcse_sd(**used).shape == (E, ndim)
        check_against_definitions(chain, lp, E, get, f'batch {where} {used}')
        s = b.get_summary(0.9, **used)
        check_summary(s, get, E, ndim, n * Wp, 0.9, bitwise_moments=where == 'device')
        ref = mb.reference_and_bounds(chain, E)                              # the mean and the sd: the moments' own bound
        mb.assert_within_bounds(s['mean'], s['sd'] / np.sqrt(n * Wp / (n * Wp - 1.0)), ref, f'batch {where}')
    got = b.get_rank_rhat(discard=60)
    np.testing.assert_array_equal(b.gather(got), got)                       # one rank: its own block
    capsys.readouterr()
    b.print_summary(1, discard=60)
    assert capsys.readouterr().out == dg.format_summary(b.get_summary(discard=60), b.param_names, spectrum=1) + '\n'
    with pytest.raises(ValueError, match='no samples'):
        b.get_summary(discard=160)


# -- 6. the shared pass -----------------------------------------------------------------------------------------------------
def test_summary_shares_the_rank_pass(monkeypatch):
    from bisip_amd import _hip
    calls = dict(plain=0, folded=0)
    plain, fold = _hip.chain_rank_normalize_dev, _hip.chain_rank_normalize_folded_dev

    def count_plain(*args, **kw):
        calls['plain'] += 1
        return plain(*args, **kw)

    def count_folded(*args, **kw):
        calls['folded'] += 1
        return fold(*args, **kw)

    monkeypatch.setattr(_hip, 'chain_rank_normalize_dev', count_plain)
    monkeypatch.setattr(_hip, 'chain_rank_normalize_folded_dev', count_folded)
    b = fitted_batch('device')
    b.get_summary(discard=60)
    assert calls == dict(plain=1, folded=1)
    calls.update(plain=0, folded=0)
    b.get_ess('bulk', discard=60)
    b.get_rank_rhat(discard=60)
    assert calls == dict(plain=2, folded=1)


# -- 7. refused arguments -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    import torch
    from bisip_amd import _hip
    n, E, Wp, ndim = 8, 2, 3, 4
    row = E * Wp * ndim
    t = torch.zeros(n * row, dtype=torch.float64, device='cuda')
    c = torch.zeros(E * 17, dtype=torch.float64, device='cuda')
    outs = [torch.full((n * E * Wp * 17,), SENTINEL, dtype=torch.float64, device='cuda') for _ in range(2)]
    work = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')
    nbytes = work.numel()

    def untouched(change):
        torch.cuda.synchronize()
        assert all((o == SENTINEL).all() for o in outs), change

    fold = dict(d_chain_ptr=t.data_ptr(), n_samples=n, sample_stride=row, n_ensembles=E, walkers_per_ensemble=Wp, ndim=ndim,
                d_center_ptr=c.data_ptr(), d_z_ptr=outs[0].data_ptr(), d_work_ptr=work.data_ptr(), work_bytes=nbytes)
    for change in [dict(d_chain_ptr=0), dict(d_center_ptr=0), dict(d_z_ptr=0), dict(d_work_ptr=0), dict(ndim=0), dict(ndim=17),
                   dict(n_samples=0), dict(n_ensembles=0), dict(walkers_per_ensemble=0), dict(sample_stride=row - 1),
                   dict(work_bytes=_hip.chain_rank_normalize_workspace(n, E, Wp, ndim) - 1)]:
        with pytest.raises(ValueError):
            _hip.chain_rank_normalize_folded_dev(**dict(fold, **change))
        untouched(change)
    squares = dict(d_chain_ptr=t.data_ptr(), n_samples=n, sample_stride=row, n_ensembles=E, walkers_per_ensemble=Wp,
                   ndim=ndim, splits=2, d_center_ptr=c.data_ptr(), d_ess_ptr=outs[0].data_ptr(), d_work_ptr=work.data_ptr(),
                   work_bytes=nbytes)
    for change in [dict(d_chain_ptr=0), dict(d_center_ptr=0), dict(d_ess_ptr=0), dict(d_work_ptr=0), dict(ndim=17),
                   dict(splits=0), dict(splits=3), dict(n_samples=3), dict(n_samples=1, splits=1), dict(n_ensembles=0),
                   dict(sample_stride=row - 1), dict(work_bytes=_hip.chain_ess_workspace(n, E, Wp, ndim, 2) - 1)]:
        with pytest.raises(ValueError):
            _hip.chain_ess_squares_dev(**dict(squares, **change))
        untouched(change)
    central = dict(d_chain_ptr=t.data_ptr(), n_samples=n, sample_stride=row, n_ensembles=E, walkers_per_ensemble=Wp,
                   ndim=ndim, d_center_ptr=c.data_ptr(), d_m2_ptr=outs[0].data_ptr(), d_m4_ptr=outs[1].data_ptr(),
                   d_work_ptr=work.data_ptr())
    for change in [dict(d_chain_ptr=0), dict(d_center_ptr=0), dict(d_m2_ptr=0), dict(d_m4_ptr=0), dict(d_work_ptr=0),
                   dict(ndim=0), dict(ndim=17), dict(n_samples=0), dict(n_ensembles=0), dict(n_ensembles=2 ** 31),
                   dict(walkers_per_ensemble=0), dict(sample_stride=row - 1)]:
        with pytest.raises(ValueError):
            _hip.chain_central_moments_dev(**dict(central, **change))
        untouched(change)
    _hip.chain_central_moments_dev(**central)                        # and the call they were variations of is taken
    torch.cuda.synchronize()
    for o in outs:                                                   # a chain of zeros about 0: both moments 0
        assert (o[:E * ndim] == 0.0).all() and (o[E * ndim:] == SENTINEL).all()
