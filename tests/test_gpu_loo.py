"""PSIS-LOO on the device (bisip_q_columns_dev, bisip_loo_columns_dev), from the C entry points up to the model and
SpectraBatch methods.  q and n_tail are held to the bits of the definition (bisip_amd.fitquality.pointwise_q,
bisip_amd.loo.psis_loo_columns); khat, sigma and elpd_rel to the bounds of tests/loo_bounds.py against its long-double
yardstick: the first-order bound where nothing is smoothed, else 16 times the float64 definition's own worst error over the
same family of columns.  Every call of the column pass goes through chain_harness.GuardedCall: the outputs and the
workspace carry guards and an output that is not asked for stays untouched; the chains are read through store()'s offset,
stride and NaN padding."""
import functools

import numpy as np
import pytest

import loo_bounds as lb
from chain_harness import GuardedCall, assert_same_bits, store
from fit_quality_bounds import inverse_variance
from test_gpu_fit_quality import batch_of, chain_near_a_centre, context, data_near, forward_rows
from test_gpu_response import make_batch

pytestmark = pytest.mark.gpu

NAMES = ('elpd_rel', 'khat', 'sigma', 'n_tail')


def run_columns(q, reff=1.0, asked=(True, True, True, True)):
    """One call of bisip_loo_columns_dev on the columns q (R, C): the four outputs (C,).  The columns come back unchanged."""
    import torch
    from bisip_amd import _hip, loo
    R, C = q.shape
    cols = np.ascontiguousarray(q.T)
    d = torch.from_numpy(cols).cuda()
    M = loo.tail_length(R, reff)
    call = GuardedCall()
    ptrs = [call.out(name, (C,), torch.int64 if name == 'n_tail' else None, asked=a) for name, a in zip(NAMES, asked)]
    nbytes = _hip.loo_columns_workspace(R, C, M)
    assert nbytes > 0
    _hip.loo_columns_dev(d.data_ptr(), R, C, M, *ptrs, call.work(nbytes), nbytes, call.stream)
    out = call.finish()
    np.testing.assert_array_equal(d.cpu().numpy().view(np.uint64), cols.view(np.uint64))
    return out


def same_bits(a, b, what):
    for x, y, name in zip(a, b, NAMES):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg=f'{what}: {name}')


def check_family(fam, what):
    """Every block of a family: within the bounds, and the same bits from a second call."""
    ratios = []
    for i, block in enumerate(fam.blocks):
        got = run_columns(block, fam.reff)
        ratios.append(fam.check(i, got, what))
        same_bits(run_columns(block, fam.reff), got, f'{what} block {i}, a second call')
    worst = tuple(max(r[i] for r in ratios) for i in range(3))
    print(f'{what}: device error / the definition\'s own worst: elpd_rel {worst[0]:.2f}, khat {worst[1]:.2f}, '
          f'sigma {worst[2]:.2f} (allowed {lb.FACTOR}); the definition\'s own: {fam.own}')
    return worst


@pytest.mark.parametrize('seed,kind', list(enumerate((lb.chi_square, lb.exponential, lb.quantised))),
                         ids=lambda v: getattr(v, '__name__', None))
def test_families_at_every_length(seed, kind):
    """Column lengths 2 ... 10,000: the smallest at which each branch turns (loo_bounds.LENGTHS)."""
    fam = lb.build(kind, seed)
    assert all(o > 0 for o in fam.own)
    tails = np.concatenate([ref['n_tail'] for ref in fam.refs])
    assert (tails <= 4).any() and (tails > 4).any()
    if kind is lb.quantised:                                            # ties at the threshold: n_tail < M
        from bisip_amd import loo
        assert any((ref['n_tail'] < loo.tail_length(b.shape[0])).any() and (ref['n_tail'] > 4).any()
                   for b, ref in zip(fam.blocks, fam.refs))
    check_family(fam, kind.__name__)


def test_long_columns():
    """128,000 values x 4 columns (31 chunks and a ragged one, a tail of 1074 from LDS), and two columns whose tail of 2100
    lies beyond the LDS capacity of 2048 and is fitted from memory."""
    fam = lb.Family('chi-square, 128,000', [lb.chi_square(128000, 4, 4)])
    assert (fam.refs[0]['n_tail'] == 1074).all()
    check_family(fam, fam.name)
    fam = lb.Family('chi-square, reff = 0.01', [lb.chi_square(10500, 2, 5), lb.exponential(10500, 2, 5)], reff=0.01)
    assert (fam.refs[0]['n_tail'] == 2100).all() and (fam.refs[1]['n_tail'] == 2100).all()
    check_family(fam, fam.name)


def test_special_columns_beside_clean_neighbours():
    """A constant column, a column with one NaN and a column with one huge outlier between clean columns whose bits must be
    those of a call without them."""
    from bisip_amd import loo
    R = 4097
    M = loo.tail_length(R)                                              # 193
    clean = lb.chi_square(R, 5, 9)
    fam_clean = lb.Family('clean', [clean])
    alone = run_columns(clean)
    fam_clean.check(0, alone)
    q = clean.copy()
    q[:, 1] = 2.25
    q[4000, 2] = np.nan
    q[4096, 3] = 5000.0
    got = run_columns(q)
    for g, a, name in zip(got, alone, NAMES):
        np.testing.assert_array_equal(g[[0, 4]].view(np.uint64), a[[0, 4]].view(np.uint64), err_msg=name)
    elpd, khat, sigma, n_tail = got
    np.testing.assert_array_equal(n_tail, [M, 0, 0, M, M])
    assert elpd[1] == -2.25 / 2 and np.isposinf(khat[1]) and np.isnan(sigma[1])                  # constant
    assert np.isnan(elpd[2]) and np.isnan(khat[2]) and np.isnan(sigma[2])                        # one NaN
    assert np.exp((np.sort(q[:, 3])[R - M - 1] - 5000.0) / 2) == 0.0                             # eu underflows (in double)
    want = loo.psis_loo_columns(q)
    assert np.isposinf(want[1][3]) and np.isposinf(khat[3]) and np.isnan(sigma[3]) and np.isfinite(elpd[3])
    ref = lb.column_ld(q[:, 3], M, fit=False)                                                    # the plain sum remains
    assert abs(lb.LD(elpd[3]) - ref['elpd']) <= ref['delpd']
    assert want[3].tolist() == n_tail.tolist()


def test_storage_order_changes_only_the_body_sum():
    """Ascending and descending storage: the sort removes the order of the tail, so khat and sigma keep their bits; the body
    is summed chunk by chunk in storage order, so elpd_rel stays within the bounds."""
    base = lb.chi_square(10000, 2, 12)
    fam = lb.Family('storage', [base, np.sort(base, axis=0), np.sort(base, axis=0)[::-1]])
    got = [run_columns(b) for b in fam.blocks]
    for i, g in enumerate(got):
        fam.check(i, g)
        for j in (1, 2, 3):
            np.testing.assert_array_equal(g[j].view(np.uint64), got[0][j].view(np.uint64))


def test_outputs_not_asked_for_are_not_written():
    q = lb.exponential(257, 3, 3)
    whole = run_columns(q)
    for asked in ((True, False, False, False), (False, True, False, False), (False, False, True, False),
                  (False, False, False, True), (True, False, False, True)):
        some = run_columns(q, asked=asked)                                # (finish() holds the others to their fill)
        for a, b, want_it, name in zip(some, whole, asked, NAMES):
            if want_it:
                np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=f'{asked}: {name}')


# -- through the model -------------------------------------------------------------------------------------------------
# model, options, N, E, Wp, samples: the six model shapes at N = 3 and 32; E = 1, 3 and 40; no Wp is a multiple of 64
CASES = [('PolynomialDecomposition', dict(poly_deg=0), 3, 1, 5, 60),
         ('PolynomialDecomposition', dict(poly_deg=0), 32, 3, 3, 21),
         ('PolynomialDecomposition', dict(poly_deg=5), 3, 3, 7, 33),
         ('PolynomialDecomposition', dict(poly_deg=5), 32, 1, 3, 85),
         ('PeltonColeCole', dict(n_modes=1), 3, 3, 5, 45),
         ('PeltonColeCole', dict(n_modes=1), 32, 1, 7, 37),
         ('PeltonColeCole', dict(n_modes=2), 3, 40, 3, 9),
         ('PeltonColeCole', dict(n_modes=2), 32, 40, 5, 13),
         ('Dias2000', {}, 3, 1, 1, 300),
         ('Dias2000', {}, 32, 3, 5, 45),
         ('Shin2015', {}, 3, 3, 65, 4),
         ('Shin2015', {}, 32, 1, 66, 70)]


def q_columns_on_device(ctx, chain, E, first=0):
    """(Z, q), (E, R, 2, N) each: what bisip_forward_columns_dev writes and what bisip_q_columns_dev makes of it."""
    import torch
    n, W, ndim = chain.shape
    Wp, N = W // E, ctx.N
    rows = np.ascontiguousarray(chain.reshape(n, E, Wp, ndim).transpose(1, 0, 2, 3).reshape(E, n * Wp, ndim))
    d = torch.from_numpy(rows).cuda()
    cols = torch.full((E * 2 * N * n * Wp + 8,), -7.25, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ctx.forward_columns_dev(first, E, d.data_ptr(), E * n * Wp, cols.data_ptr(), st)
    torch.cuda.synchronize()
    Z = cols[:-8].cpu().numpy().reshape(E, 2, N, n * Wp).transpose(0, 3, 1, 2).copy()
    ctx.q_columns_dev(first, E, cols.data_ptr(), n * Wp, st)
    torch.cuda.synchronize()
    host = cols.cpu().numpy()
    assert (host[-8:] == -7.25).all(), 'values after the columns were written'
    return Z, host[:-8].reshape(E, 2, N, n * Wp).transpose(0, 3, 1, 2).copy()


def view_of(chain, E, **storage):
    import torch
    from bisip_amd.chainview import ChainView
    n, W, ndim = chain.shape
    stored, offset, stride = store(chain, **storage)
    return ChainView(torch.from_numpy(stored).cuda(), n, E, W // E, ndim, offset, stride)


@pytest.mark.parametrize('model,kw,n_freq,E,Wp,n', CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_through_the_model(model, kw, n_freq, E, Wp, n, monkeypatch):
    from bisip_amd import decomposition, loo
    from bisip_amd import fitquality as fq
    b = batch_of(model, kw, n_freq, E)
    chain = chain_near_a_centre(b, E, Wp, n, seed=n + Wp)
    zn, err = data_near(forward_rows(b.ctx, chain, E), seed=n)
    ctx = context(b, zn, err)
    what = f'{model} {kw} N={n_freq} E={E} Wp={Wp} n={n}'
    # q, to the bit
    Z, q = q_columns_on_device(ctx, chain, E)
    want_q = fq.pointwise_q(Z, zn[:, None], inverse_variance(err)[:, None])
    assert_same_bits(q, want_q, what + ': q')
    assert np.isfinite(want_q).all() and want_q.max() < 1e6, 'the data lie near the model: else the inputs are wrong'
    if E == 3:                                                          # spectra 1 and 2 of the three
        sub = q_columns_on_device(ctx, np.ascontiguousarray(chain[:, Wp:]), 2, first=1)[1]
        np.testing.assert_array_equal(sub.view(np.uint64), q[1:].view(np.uint64))
    # the column pass over the chain where it lies, behind an offset, a stride and padding
    R = n * Wp
    fam = lb.Family(what, [q.transpose(1, 0, 2, 3).reshape(R, E * 2 * n_freq)])
    got = loo.device_loo(view_of(chain, E), ctx)
    assert all(g.shape == (E, 2, n_freq) for g in got) and got[2].dtype == np.int64
    elpd, khat, n_tail = (g.reshape(-1) for g in got)
    sigma = np.where(np.isfinite(khat), fam.refs[0]['sigma'].astype(np.float64), np.nan)     # (device_loo asks for no sigma)
    ratio = fam.check(0, (elpd, khat, sigma, n_tail), 'device_loo')
    print(f'{what}: elpd_rel {ratio[0]:.2f}, khat {ratio[1]:.2f} of the definition\'s own worst error (allowed {lb.FACTOR})')
    for storage in (dict(discard=0, thin=1, pad=0), dict(discard=3, thin=4, pad=11)):
        for a, g in zip(loo.device_loo(view_of(chain, E, **storage), ctx), got):
            np.testing.assert_array_equal(a.view(np.uint64), g.view(np.uint64), err_msg=f'{what} {storage}')
    if E > 1:
        # a pass split: one spectrum's columns per pass
        monkeypatch.setattr(decomposition, 'RTD_PASS_BYTES', R * 2 * n_freq * 8)
        for a, g in zip(loo.device_loo(view_of(chain, E), ctx), got):
            np.testing.assert_array_equal(a.view(np.uint64), g.view(np.uint64), err_msg=f'{what}: in {E} passes')
        monkeypatch.undo()
        # first_spectrum > 0
        part = loo.device_loo(view_of(np.ascontiguousarray(chain[:, Wp:]), E - 1), ctx, first_spectrum=1)
        for a, g in zip(part, got):
            np.testing.assert_array_equal(a.view(np.uint64), g[1:].view(np.uint64), err_msg=f'{what}: spectra 1 ...')
    ctx.close()
    b.close()


def test_refusals_of_q_columns():
    b = make_batch('PeltonColeCole', dict(n_modes=1), 20, 8, count=2)
    for match, args in (('null', (0, 1, 0, 64)), ('spectra', (2, 1, 4096, 64)), ('spectra', (1, 2, 4096, 64)),
                        ('bad shape', (0, 0, 4096, 64)), ('bad shape', (0, 1, 4096, 0)), ('aligned', (0, 1, 4100, 64))):
        with pytest.raises(ValueError, match=match):
            b.ctx.q_columns_dev(*args)
    with pytest.raises(AssertionError, match='not fitted'):
        b.get_loo()
    b.close()


# -- through the public interface -------------------------------------------------------------------------------------
KW = dict(discard=10, thin=3)
KEYS = {'elpd_loo', 'p_loo', 'looic', 'se', 'n_bad', 'k_threshold', 'elpd_i', 'p_loo_i', 'pareto_k', 'n_tail'}


def check_public(result, view, ctx, Z, zn, err, what):
    """A get_loo result of ONE spectrum: the composition, to the bit, of device_loo and device_fit_quality over the same
    samples; pareto_k and elpd_rel within the bounds against the definition on the host's q; and n_bad, a count of threshold
    crossings, the definition's own -- on inputs that the definition alone keeps outside the band of the bound."""
    from bisip_amd import fitquality as fq
    from bisip_amd import loo
    R, N = Z.shape[0], Z.shape[-1]
    assert set(result) == KEYS
    elpd_rel, khat, n_tail = (a[0] for a in loo.device_loo(view, ctx))
    lmeh = fq.device_fit_quality(view, ctx)[2][0]
    want = loo.loo_from_columns(elpd_rel, khat, n_tail, lmeh, np.log(err ** 2), R)
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(result[k]), np.asarray(want[k]), err_msg=f'{what}: {k}')
    assert all(isinstance(result[k], float) for k in ('elpd_loo', 'p_loo', 'looic', 'se', 'k_threshold'))
    assert isinstance(result['n_bad'], int) and result['looic'] == -2 * result['elpd_loo']
    assert result['elpd_i'].shape == result['p_loo_i'].shape == result['pareto_k'].shape == result['n_tail'].shape == (2, N)
    q = fq.pointwise_q(Z, zn, inverse_variance(err)).reshape(R, 2 * N)
    fam = lb.Family(what, [q])
    sigma = np.where(np.isfinite(khat), fam.refs[0]['sigma'].astype(np.float64).reshape(2, N), np.nan)
    fam.check(0, tuple(a.reshape(-1) for a in (elpd_rel, khat, sigma, n_tail)), 'get_loo')
    # n_bad: the definition's khat lies further from the threshold than its own error and the device's allowance together
    kdef = loo.psis_loo_columns(q)[1]
    kt = loo.k_threshold(R)
    band = fam.allowed[1] + fam.own[1]
    assert (np.abs(kdef[np.isfinite(kdef)] - kt) > band).all(), 'a point inside the band: choose other inputs'
    assert result['n_bad'] == int((kdef > kt).sum()) and result['k_threshold'] == kt


@functools.lru_cache(maxsize=None)
def fitted_model(chain='device'):
    import bisip_amd
    m = bisip_amd.PeltonColeCole(bisip_amd.DataFiles()['SIP-K389175'], n_modes=1, nwalkers=8, nsteps=40)
    p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(3).randn(8, 4)
    np.random.seed(8)
    m.fit(p0=p0, chain=chain)
    return m


def test_model_method():
    from bisip_amd import loo
    m = fitted_model()
    assert m._sampler.chain_on_device
    flat = m.get_chain(flat=True, **KW)
    Z = m._context().forward(np.ascontiguousarray(flat))
    with pytest.warns(UserWarning, match='No samples were discarded'):
        assert m.get_loo()['elpd_i'].shape == (2, Z.shape[-1])
    result = m.get_loo(**KW)
    view = m._sampler.used_samples_dev(**KW)
    check_public(result, view, m._sampler.backend.ctx, Z, m._data['zn'], m._data['zn_err'], 'model')
    # an explicit chain goes up once: the same columns, the same bits
    again = m.get_loo(chain=flat)
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(again[k]), np.asarray(result[k]), err_msg=k)
    # reff shortens the tail: R = 80, M = ceil(min(16, 3 sqrt(80 / 4))) = 14 (a rejected move repeats a row: ties, n_tail < M)
    short = m.get_loo(reff=4.0, **KW)
    assert flat.shape[0] == 80 and short['n_tail'].max() == 14 and result['n_tail'].max() == 16
    assert (short['n_tail'] <= result['n_tail']).all()
    rows = loo.compare_loo({'a': result, 'b': short})
    assert {r['name'] for r in rows} == {'a', 'b'} and rows[0]['d_elpd'] == 0.0 and rows[1]['d_elpd'] >= 0.0
    with pytest.raises(ValueError, match='Do not pass both'):
        m.get_loo(chain=flat, discard=3)
    with pytest.raises(ValueError, match='reff'):
        m.get_loo(reff=-1.0, **KW)


def test_a_host_chain_gives_the_results_of_the_device_chain():
    """fit(chain='device') and fit(chain='host') from the same start and seed store the same samples: get_loo takes the
    same columns from either."""
    dev, host = fitted_model('device'), fitted_model('host')
    np.testing.assert_array_equal(dev.get_chain(**KW), host.get_chain(**KW))
    a, b = dev.get_loo(**KW), host.get_loo(**KW)
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def test_spectra_batch_method():
    import bisip_amd
    from bisip_amd.chainview import ChainView
    files = bisip_amd.DataFiles()
    E, Wp = 3, 8
    names = sorted(files)[:E]
    b = bisip_amd.SpectraBatch('PeltonColeCole', [files[k] for k in names], nwalkers=Wp, nsteps=40, n_modes=1)
    p0 = np.array([1.0, 0.3, -6.0, 0.5]) + 1e-4 * np.random.RandomState(1).randn(E, Wp, 4)
    b.fit(p0, seed=6, chain='device')
    result = b.get_loo(**KW)
    assert set(result) == KEYS
    assert all(result[k].shape == (E,) for k in ('elpd_loo', 'p_loo', 'looic', 'se', 'n_bad'))
    assert all(result[k].shape == (E, 2, b.N) for k in ('elpd_i', 'p_loo_i', 'pareto_k', 'n_tail'))
    flat = b.get_chain(flat=True, **KW)                                # (E, n * Wp, ndim)
    Z = b.forward(flat)
    view = b._fitted().used_samples_dev(**KW)
    for e in range(E):
        one = {k: (v if k == 'k_threshold' else v[e]) for k, v in result.items()}
        one.update({k: float(one[k]) for k in ('elpd_loo', 'p_loo', 'looic', 'se')}, n_bad=int(one['n_bad']))
        sub = ChainView(view.tensor, view.n, 1, Wp, b.ndim, view.offset + e * Wp * b.ndim, view.stride, view.backend)
        ctx_e = bisip_amd.PeltonColeCole(files[names[e]], n_modes=1, nwalkers=Wp, nsteps=5)
        # row e is a lone model's result on the same rows
        lone = ctx_e.get_loo(chain=flat[e])
        for k in ('elpd_i', 'p_loo_i', 'pareto_k', 'n_tail', 'n_bad'):
            np.testing.assert_array_equal(np.asarray(lone[k]), np.asarray(one[k]), err_msg=f'spectrum {e}: {k}')
        # ... and holds what a lone result holds (the one-spectrum view: first_spectrum = e of the batch's context)
        from bisip_amd import loo
        part = loo.device_loo(sub, b._fitted().backend.ctx, first_spectrum=e)
        np.testing.assert_array_equal(part[1][0].view(np.uint64), result['pareto_k'][e].view(np.uint64))
        assert abs(lone['elpd_loo'] - one['elpd_loo']) <= 64 * lb.U * np.abs(one['elpd_i']).sum()
    with pytest.raises(ValueError):
        b.get_loo(discard=40)
    b.close()
