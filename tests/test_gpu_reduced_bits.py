"""The QR-reduced log-probability kernels against their host emulation, bit for bit.

Every test reads the operands the device holds (HipContext.reduced_operands), runs the host emulation of
logprob_row_reduced<P, COMP> on them (_hip.reduced_emulate: host_emulate.inc's chi2_kernel, the arithmetic every
estimate behind BISIP_VARIANT_AUTO is measured on) and compares with what the kernel returned: equal int64 views
outside NaN, equal NaN masks.  No tolerance.  tests/test_reduced_emulation.py holds the emulation itself to an exact
rational statement of the documented sequence, so "bit-exact" has a root that does not depend on any kernel.
The sampler routes (ReducedLP direct and its register copy, logprob_row_reduced_staged, BatchReducedLP) are pinned by
array_equal to ctx.logprob in test_gpu_sampler.py and test_gpu_batch.py: those pins now end at the emulation."""

import numpy as np
import pytest

from conftest import extended_cases, golden_cases, valley_cases
from test_gpu_parity import _pd_context, _shell_rows, make_ctx
from test_reduced_emulation import assert_same_bits

pytestmark = pytest.mark.gpu

TIER = {'reduced': 0, 'reduced_comp': 1}
KERNEL = {'reduced': 'k_logprob_pd_reduced', 'reduced_comp': 'k_logprob_pd_reduced_comp'}
BULK = 131072 + 257            # past the 131,072 rows from which the bulk kernels launch; a ragged last block


def _emulate(ctx, tier, bounds, theta, spectrum=0):
    from bisip_amd import _hip
    ops = ctx.reduced_operands(spectrum, tier)
    assert ops['runs'], (spectrum, tier)
    return _hip.reduced_emulate(ops, bounds, theta)


def _logprob_shifted(ctx, theta):
    """The same rows from a device pointer 8 bytes past 16-byte alignment: the scalar staging path."""
    import torch
    W, n = theta.shape
    dev = torch.zeros(W * n + 2, dtype=torch.float64, device='cuda')
    view = dev[1:1 + W * n]
    assert view.data_ptr() % 16 == 8
    view.copy_(torch.from_numpy(np.ascontiguousarray(theta).reshape(-1)))
    out = torch.empty(W, dtype=torch.float64, device='cuda')
    ctx.logprob_dev(view.data_ptr(), W, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _box_rows(bounds, W, seed):
    """W rows uniform in the box, a part of them with small coefficients (where a decent fit lies), and edge rows:
    on a bound, outside, NaN."""
    rng = np.random.RandomState(seed)
    theta = rng.uniform(bounds[0], bounds[1], (W, bounds.shape[1]))
    theta[: W // 4, 1:] *= 1e-2
    if W >= 8:
        theta[W // 2, 0] = bounds[1, 0]
        theta[W // 2 + 1, -1] = bounds[0, -1]
        theta[W // 2 + 2, 1] = np.nan
        theta[W // 2 + 3, 0] = 2.0 * bounds[1, 0] + 1.0
    return theta


def _default_box(P):
    return np.array([[0.9] + [-1.0] * (P + 1), [1.1] + [1.0] * (P + 1)])


def _fixture_rows(P):
    """The golden fixtures' own rows (72 each: on-bound and NaN rows among them) at this degree, for the default box."""
    rows = []
    for path in golden_cases() + extended_cases():
        if 'PolynomialDecomposition' not in path:
            continue
        g = np.load(path)
        if int(g['poly_deg']) == P:
            assert np.array_equal(g['bounds'], _default_box(P)), path
            rows.append(g['theta'])
    return rows


def _context_shell_rows(d, taus, log_taus, c_exp, bounds, seed):
    from bisip_amd import _hip
    ops = _hip.polydecomp_operands(d['w'], d['zn'], d['zn_err'], taus, log_taus, c_exp)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        return _shell_rows(ops, bounds, 400, seed)


@pytest.mark.parametrize('variant', ['reduced', 'reduced_comp'])
@pytest.mark.parametrize('P', range(11))
def test_every_instantiation(P, variant):
    """logprob_row_reduced<P, COMP> for P = 0 ... 10, both tiers, on two designs each: 2,000 rows uniform in the box,
    the golden fixtures' rows of this degree, the rows of the context's shell logp = 0 inside the box; from degree 6 on
    the valley fixtures of this degree in contexts and boxes of their own."""
    tier, compared = TIER[variant], 0
    fixture = _fixture_rows(P)
    for c_exp in (1.0, 0.5):
        ctx, bounds, d, taus, log_taus = _pd_context(32, P, c_exp, variant=variant)
        ctx.reduced_guard(False)
        assert ctx.kernel_name == KERNEL[variant]
        shell = _context_shell_rows(d, taus, log_taus, c_exp, bounds, P)
        theta = np.vstack([_box_rows(bounds, 2000, 10 * P + tier)] + fixture + [shell])
        assert_same_bits(ctx.logprob(theta), _emulate(ctx, tier, bounds, theta))
        compared += len(theta)
        ctx.close()
    valleys = [p for p in valley_cases() if int(np.load(p)['poly_deg']) == P] if P >= 6 else []
    for path in valleys:
        g = np.load(path)
        ctx = make_ctx(g, 'PolynomialDecomposition', variant)
        ctx.reduced_guard(False)
        assert ctx.kernel_name == KERNEL[variant]
        assert_same_bits(ctx.logprob(g['theta']), _emulate(ctx, tier, g['bounds'], g['theta']))
        compared += len(g['theta'])
        ctx.close()
    assert P < 6 or valleys
    print(f'P={P} {variant}: {compared} rows, {len(fixture)} golden fixtures, {len(valleys)} valley fixtures')


@pytest.mark.parametrize('variant', ['reduced', 'reduced_comp'])
@pytest.mark.parametrize('P', [5, 9])
def test_row_counts_and_both_staging_paths(P, variant):
    """One row, a wave less one, a wave, a wave and one, a ragged fifth workgroup, sixteen workgroups: the 64-lane
    kernel through the LDS transposition, from a 16-byte-aligned pointer (vector staging) and from one 8 bytes past
    (scalar staging)."""
    tier = TIER[variant]
    ctx, bounds, *_ = _pd_context(32, P, 1.0, variant=variant)
    ctx.reduced_guard(False)
    assert ctx.kernel_name == KERNEL[variant]
    for W in (1, 63, 64, 65, 257, 1000):
        theta = _box_rows(bounds, W, 100 * P + W)
        want = _emulate(ctx, tier, bounds, theta)
        assert_same_bits(ctx.logprob(theta), want)
        assert_same_bits(_logprob_shifted(ctx, theta), want)
    ctx.close()


@pytest.mark.parametrize('P,variant', [(5, 'reduced'), (5, 'reduced_comp'), (6, 'reduced_comp'), (10, 'reduced_comp')])
def test_bulk_routes(P, variant):
    """131,329 rows: the plain tier's 128-lane streaming kernel, the compensated tier with its operands as kernel
    arguments (degree 5, 256 lanes) and with its operands read from memory through the scalar path (degrees 6 and 10),
    each from an aligned pointer and from one 8 bytes past."""
    tier = TIER[variant]
    ctx, bounds, *_ = _pd_context(32, P, 1.0, variant=variant)
    ctx.reduced_guard(False)
    assert ctx.kernel_name == KERNEL[variant]
    theta = _box_rows(bounds, BULK, P)
    want = _emulate(ctx, tier, bounds, theta)
    assert_same_bits(ctx.logprob(theta), want)
    assert_same_bits(_logprob_shifted(ctx, theta), want)
    ctx.close()


def test_small_and_bulk_routes_are_held_to_the_same_operands():
    """A lone spectrum at degree 6 on the compensated tier: 40 rows take the operands as a kernel argument, 2 x 256 x 256
    rows read them from the device image.  Both are cut from one host image, which reduced_operands(0, 1) reads once:
    both launches equal its emulation bit for bit, and the 40 rows, placed at the front of the big launch, give the
    same bits in both."""
    ctx, bounds, *_ = _pd_context(32, 6, 1.0, variant='reduced_comp')
    ctx.reduced_guard(False)
    assert ctx.kernel_name == KERNEL['reduced_comp']
    ops = ctx.reduced_operands(0, 1)
    assert ops['runs']
    from bisip_amd import _hip
    small = _box_rows(bounds, 40, 6)
    big = np.vstack([small, _box_rows(bounds, 2 * 256 * 256 - 40, 7)])
    got_small, got_big = ctx.logprob(small), ctx.logprob(big)
    assert_same_bits(got_small, _hip.reduced_emulate(ops, bounds, small))
    assert_same_bits(got_big, _hip.reduced_emulate(ops, bounds, big))
    assert_same_bits(got_big[:40], got_small)
    assert np.isfinite(got_small).sum() >= 30
    ctx.close()


@pytest.mark.parametrize('P,variant', [(6, 'reduced'), (8, 'reduced_comp')])
def test_operands_follow_a_moved_box(P, variant):
    """bisip_ctx_set_bounds re-centres the reduced form: the kernel arguments of the small launches and the device image
    of the bulk launch follow the host copies and the new box -- a stale one shows here.  The new box is narrower in
    the coefficients and ends short of the least-squares R0, so the plain tier's old expansion point is not in it and
    its operands must differ.  A lone spectrum's COMPENSATED tier expands about the least-squares point under every
    box (reduced_center_comp: e then vanishes to working precision, and d + dl is exact wherever bhat lies, so no
    other candidate reads better -- on none of thirteen designs tried under five to eleven boxes each, however far
    from the least-squares point), so there only the box itself moves; compensated kernels on operands that do move:
    test_batch_operands_follow_a_moved_box."""
    from bisip_amd import _hip
    tier = TIER[variant]
    ctx, bounds, d, taus, log_taus = _pd_context(32, P, 1.0, variant=variant)
    ctx.reduced_guard(False)
    before = ctx.reduced_operands(0, tier)
    theta = _box_rows(bounds, 1000, P)
    assert_same_bits(ctx.logprob(theta), _hip.reduced_emulate(before, bounds, theta))
    r0 = _hip.polydecomp_operands(d['w'], d['zn'], d['zn_err'], taus, log_taus, 1.0)['bhat'][0]
    assert 0.92 < r0 < 1.08
    moved = bounds * np.r_[1.0, np.full(P + 1, 1e-4)]
    moved[:, 0] = (0.9, 0.5 * (0.9 + r0)) if r0 >= 1.0 else (0.5 * (r0 + 1.1), 1.1)
    ctx.set_bounds(moved)
    assert ctx.kernel_name == KERNEL[variant]
    after = ctx.reduced_operands(0, tier)
    assert after['runs']
    if tier == 0:
        assert any(not np.array_equal(before[k], after[k]) for k in ('bhat', 'e', 'elo'))
    assert np.array_equal(before['R'], after['R']) and before['rest'] == after['rest']      # the triangle is the design's
    for W in (1000, BULK):
        theta = np.vstack([_box_rows(moved, W - 200, P + W), _box_rows(bounds, 200, P)])      # rows of the old box: outside now
        want = _hip.reduced_emulate(after, moved, theta)
        assert np.isfinite(want[:W - 200]).sum() > W // 2 and np.isneginf(want[W - 200:]).sum() > 100
        assert_same_bits(ctx.logprob(theta), want)
        assert_same_bits(_logprob_shifted(ctx, theta), want)
    ctx.close()


BATCH_E, BATCH_P = 16, 7


def _mixed_batch(monkeypatch):
    """A degree-7 batch on 'auto' whose spectra mix tiers: built, as test_guard_closes_a_batch_mix_before_it_closes_a_tier
    builds its batch, with the estimate's shell probes at a fifth of their weight -- 4 of these 16 designs then keep
    the plain tier."""
    import bisip_amd
    from test_gpu_batch import _tables
    monkeypatch.setenv('BISIP_SHELL_WEIGHT', '0.01')
    batch = bisip_amd.SpectraBatch('PolynomialDecomposition', _tables(BATCH_E, 32), nwalkers=64, nsteps=4, poly_deg=BATCH_P)
    monkeypatch.delenv('BISIP_SHELL_WEIGHT')
    batch.ctx.reduced_guard(False)
    assert batch.ctx.variant == 'reduced_comp' and batch.ctx.kernel_name == KERNEL['reduced_comp']
    return batch


def _batch_tiers_and_operands(ctx):
    """Per spectrum the tier it runs (0 / 1) and that tier's operands; both tiers exist in the batch."""
    tiers, ops = [], []
    for e in range(BATCH_E):
        o = ctx.reduced_operands(e, 0)             # 'auto' estimates the plain tier of every spectrum
        if not o['runs']:
            o = ctx.reduced_operands(e, 1)
        assert o['runs']
        tiers.append(int(o['comp']))
        ops.append(o)
    assert (tiers.count(0), tiers.count(1)) == ctx.reduced_tiers
    return tiers, ops


def _compare_batch(ctx, ops, bounds, seed, rows_per_spectrum=(40, 128, 8192)):
    """40 rows per spectrum: k_logprob_batch_reduced with rows of two spectra in a wave; 128: whole waves per spectrum;
    8,192 (131,072 rows in all, a multiple of 256 per spectrum): k_logprob_batch_reduced_stream."""
    from bisip_amd import _hip
    n = BATCH_P + 2
    for Wp in rows_per_spectrum:
        theta = _box_rows(bounds, BATCH_E * Wp, seed + Wp).reshape(BATCH_E, Wp, n)
        got = ctx.logprob(theta.reshape(-1, n)).reshape(BATCH_E, Wp)
        for e in range(BATCH_E):
            assert_same_bits(got[e], _hip.reduced_emulate(ops[e], bounds, theta[e]))


def test_batch_kernels_with_a_tier_per_spectrum(monkeypatch):
    """Every spectrum of a batch that mixes tiers against the emulation of the tier it runs on ITS operands, through the
    three batch kernels (a tier per lane, per wave, per workgroup); then the variant forced to 'reduced_comp' (no tier
    table)."""
    batch = _mixed_batch(monkeypatch)
    ctx, bounds = batch.ctx, np.array(batch.param_bounds)
    tiers, ops = _batch_tiers_and_operands(ctx)
    assert tiers.count(0) >= 1 and tiers.count(1) >= 1, tiers
    for e in range(BATCH_E):                       # a spectrum's other tier holds nothing for it, or does not run
        if tiers[e] == 0:
            with pytest.raises(ValueError):
                ctx.reduced_operands(e, 1)
        else:
            assert not ctx.reduced_operands(e, 0)['runs']
    _compare_batch(ctx, ops, bounds, 1)
    ctx.set_variant('reduced_comp')
    assert ctx.reduced_tiers == (0, BATCH_E)
    tiers_forced, ops_forced = _batch_tiers_and_operands(ctx)
    assert tiers_forced == [1] * BATCH_E
    for e in range(BATCH_E):                       # a compensated spectrum keeps its operands
        if tiers[e] == 1:
            assert all(np.array_equal(ops[e][k], ops_forced[e][k]) for k in ('R', 'Rlo', 'bhat', 'e', 'elo'))
    _compare_batch(ctx, ops_forced, bounds, 2)
    batch.close()


def test_batch_operands_follow_a_moved_box(monkeypatch):
    """The compensated batch kernels after bisip_ctx_set_bounds: with R0 held below 0.95 -- short of every spectrum's
    least-squares R0 -- and the coefficients to half their range the batch still mixes tiers, but other spectra take
    the plain tier and the plain tier expands about another point: both device images and the tier table have to
    follow.  Operands and tiers are read again and must differ from before."""
    batch = _mixed_batch(monkeypatch)
    ctx, bounds = batch.ctx, np.array(batch.param_bounds)
    tiers, ops = _batch_tiers_and_operands(ctx)
    _compare_batch(ctx, ops, bounds, 3, (40,))
    moved = bounds.copy()
    moved[:, 1:] *= 0.5
    moved[1, 0] = 0.95
    monkeypatch.setenv('BISIP_SHELL_WEIGHT', '0.01')
    ctx.set_bounds(moved)
    monkeypatch.delenv('BISIP_SHELL_WEIGHT')
    assert ctx.variant == 'reduced_comp'
    tiers2, ops2 = _batch_tiers_and_operands(ctx)
    assert tiers2.count(0) >= 1 and tiers2.count(1) >= 1, tiers2
    assert tiers2 != tiers                                                                  # the tier table moved
    kept_plain = [e for e in range(BATCH_E) if tiers[e] == 0 and tiers2[e] == 0]
    assert kept_plain and any(not np.array_equal(ops[e]['bhat'], ops2[e]['bhat']) for e in kept_plain)
    _compare_batch(ctx, ops2, moved, 4)
    batch.close()


@pytest.mark.parametrize('P,variant', [(5, 'reduced'), (8, 'reduced_comp')])
def test_the_estimate_measures_what_the_kernel_computes(P, variant):
    """bisip_ctx_reduced_check of the emulated values equals that of the kernel's: kernel = emulation, and the
    estimates measure the emulation."""
    tier = TIER[variant]
    ctx, bounds, d, taus, log_taus = _pd_context(32, P, 1.0, variant=variant)
    ctx.reduced_guard(False)
    theta = np.vstack([_box_rows(bounds, 1000, P), _context_shell_rows(d, taus, log_taus, 1.0, bounds, P)])
    emulated, kernel = _emulate(ctx, tier, bounds, theta), ctx.logprob(theta)
    assert_same_bits(kernel, emulated)
    assert ctx.reduced_check(theta, emulated) == ctx.reduced_check(theta, kernel)
    ctx.close()


def test_operands_entry_point_refuses_what_it_does_not_hold():
    ctx, *_ = _pd_context(32, 5, 1.0, 0)           # 'auto' on the headline shape: the plain tier, nothing else built
    assert ctx.variant == 'reduced' and ctx.reduced_operands(0, 0)['runs']
    for spectrum, tier in ((0, 1), (0, 2), (0, -1), (1, 0), (-1, 0)):
        with pytest.raises(ValueError):
            ctx.reduced_operands(spectrum, tier)
    ctx.set_variant('collapsed')
    assert not ctx.reduced_operands(0, 0)['runs']  # held, not run
    ctx.close()
    ctx, bounds, *_ = _pd_context(32, 5, 1.0, 0, variant='reduced_comp')
    assert ctx.reduced_operands(0, 1)['runs']
    assert not ctx.reduced_operands(0, 0)['runs']  # estimated when the context was created on 'auto': held, not run
    ctx.set_bounds(bounds * 0.5)                   # a new box: only what the forced variant runs is estimated again
    assert ctx.reduced_operands(0, 1)['runs']
    with pytest.raises(ValueError):
        ctx.reduced_operands(0, 0)
    ctx.close()
    cc = make_ctx(np.load([p for p in golden_cases() if 'case15_' in p][0]), 'PeltonColeCole')
    with pytest.raises(ValueError):
        cc.reduced_operands(0, 0)
    cc.close()
