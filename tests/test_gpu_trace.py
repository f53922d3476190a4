"""Per-step walker statistics on the device (bisip_chain_trace_dev), from the C entry point up to the model and
SpectraBatch methods.  Percentiles are compared with np.percentile on a host copy of the same samples: the same doubles,
NaN at the same places, no tolerance.  The mean is held to the first-order bound of any summation order and, bit for
bit, to the summation order include/bisip_hip.h states."""
import functools
import math
import warnings

import numpy as np
import pytest

import fitted
from chain_harness import SENTINEL, GuardedCall, shape_id, store

pytestmark = pytest.mark.gpu

P_SETS = [[50.0], [0.0, 100.0], [2.5, 50.0, 97.5], [0.0, 2.5, 16.0, 33.3, 50.0, 84.0, 97.5, 100.0], None]


def lds_walkers(ndim):
    from bisip_amd import _hip
    return _hip.chain_trace_lds_walkers(ndim)


def shapes():
    """(n, E, Wp, ndim): one and two walkers, around the wave width, several small ensembles per workgroup, more than one
    workgroup, the last ensemble the LDS kernel takes and the first it does not, and a column too long for the selection
    kernel's registers."""
    out = [(5, 1, 2, 1), (4, 3, 1, 2), (3, 2, 63, 7), (3, 2, 64, 7), (3, 2, 65, 7), (2, 1, 257, 16), (6, 4, 256, 7),
           (3, 5, 9, 3)]
    for ndim in (1, 7):
        out += [(2, 1, lds_walkers(ndim), ndim), (2, 1, lds_walkers(ndim) + 1, ndim)]
    out.append((2, 1, 40961, 2))
    return out


@functools.lru_cache(maxsize=None)
def hand_built_chain(n, E, Wp, ndim):
    """store() of a chain whose used samples are (n, E, Wp, ndim), with a random filler between them: columns of widths 1e-8 ... 1e2 around centres of any size, a constant column, duplicated values, and in
    chosen (sample, ensemble, parameter) slices +NaN, -NaN, +inf, -inf and both infinities.  Returns (store()'s three, used
    (n, E, Wp, ndim), mask of the slices with a non-finite value (n, E, ndim))."""
    rng = np.random.default_rng(n * 1000003 + E * 10007 + Wp * 101 + ndim)
    centre = rng.normal(size=(1, E, 1, ndim)) * 10.0 ** rng.integers(-3, 4, (1, E, 1, ndim))
    width = 10.0 ** rng.integers(-8, 3, (1, E, 1, ndim)).astype(np.float64)
    used = centre + width * rng.normal(size=(n, E, Wp, ndim))
    used[0, 0, :, ndim - 1] = 0.25                                     # a constant column
    if Wp >= 4:                                                        # duplicates: a few distinct values only
        used[n - 1, E - 1, :, 0] = np.round(rng.normal(size=Wp) * 2.0) * 0.5
        used[n - 1, 0, : Wp // 2, ndim - 1] = used[n - 1, 0, Wp // 2: 2 * (Wp // 2), ndim - 1]
    slices = [(s, e, q) for s in range(1, n) for e in range(E) for q in range(ndim)]       # sample 0 stays finite
    plants = [[np.nan], [-np.nan], [np.inf], [-np.inf], [np.inf, -np.inf], [np.nan, np.inf]]
    bad = np.zeros((n, E, ndim), dtype=bool)
    step = max(1, len(slices) // len(plants))
    for (s, e, q), values in zip(slices[::step], plants):
        w = rng.choice(Wp, size=min(len(values), Wp), replace=False)
        used[s, e, w, q] = values[:w.size]
        bad[s, e, q] = True
    # -nan must really carry the sign bit
    neg = np.array([-np.nan])
    assert np.signbit(neg[0])
    return store(used, filler=lambda shape: rng.normal(size=shape) * 1e6), used, bad


def run_abi(stored, n, E, Wp, ndim, p, mean=True):
    import torch
    from bisip_amd import _hip
    samples, offset, stride = stored
    t = torch.from_numpy(samples).cuda()
    n_p = 0 if p is None else len(p)
    call = GuardedCall()
    pct = call.out('the percentiles', (n_p, n, E, ndim), asked=n_p > 0)
    avg = call.out('the mean', (n, E, ndim), asked=mean)
    nbytes = _hip.chain_trace_workspace(n, E, Wp, ndim, n_p)
    assert (nbytes == 0) == (Wp <= lds_walkers(ndim))
    _hip.chain_trace_dev(t.data_ptr() + 8 * offset, n, stride, E, Wp, ndim, p, pct, avg, call.work(nbytes), nbytes,
                         call.stream)
    return call.finish()


def fixed_order_mean(x):
    """The mean of x (..., Wp) over its last axis in the order include/bisip_hip.h states: value w goes to partial sum
    w mod 64, in turn; the 64 partial sums are added pairwise 32, 16, ... 1 apart; the sum is divided by Wp."""
    Wp = x.shape[-1]
    rows = -(-Wp // 64)
    padded = np.zeros(x.shape[:-1] + (rows * 64,))
    padded[..., :Wp] = x
    padded = padded.reshape(x.shape[:-1] + (rows, 64))
    acc = np.zeros(x.shape[:-1] + (64,))
    with np.errstate(invalid='ignore'):
        for r in range(rows):
            acc = acc + padded[..., r, :]
        d = 32
        while d >= 1:
            acc = acc[..., :d] + acc[..., d:2 * d]
            d //= 2
        return acc[..., 0] / Wp


def check_mean(got, used, bad):
    n, E, Wp, ndim = used.shape
    # whichever kernel ran, the sum is taken in the one documented order: the same bits as that order in NumPy
    order = fixed_order_mean(np.moveaxis(used, 2, -1))
    np.testing.assert_array_equal(got[~bad].view(np.uint64), order[~bad].view(np.uint64))
    with np.errstate(invalid='ignore'):
        want = np.mean(used, axis=2)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[bad], want[bad])                 # (inf, -inf, NaN at the same places)
    worst = 0.0
    for s, e, q in zip(*np.nonzero(~bad)):
        x = used[s, e, :, q]
        exact = math.fsum(x) / Wp
        # twice the first-order bound (Wp - 1) 2^-53 sum|x| / Wp of any summation order
        bound = Wp * 2.0 ** -52 * np.mean(np.abs(x))
        err = abs(got[s, e, q] - exact)
        worst = max(worst, err / bound if bound else float(err > 0))
        assert err <= bound, (s, e, q, got[s, e, q], exact, bound)
    return worst


@pytest.mark.parametrize('shape', shapes(), ids=shape_id)
def test_entry_point_against_numpy(shape):
    n, E, Wp, ndim = shape
    stored, used, bad = hand_built_chain(*shape)
    first_mean = None
    for p in P_SETS:
        pct, avg = run_abi(stored, n, E, Wp, ndim, p)
        assert not (pct == SENTINEL).any() and not (avg == SENTINEL).any()      # every element written
        if p is not None:
            with np.errstate(invalid='ignore'), warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                want = np.percentile(used, p, axis=2)
            np.testing.assert_array_equal(pct, want)
            assert np.isnan(pct[:, bad]).any() and np.isfinite(pct[:, ~bad]).all()
        if first_mean is None:
            first_mean = avg
            worst = check_mean(avg, used, bad)
            print(f'shape {shape}: mean error at most {worst:.3f} of its bound')
        else:       # the same chain gives the same bits, with or without percentiles beside it
            np.testing.assert_array_equal(avg.view(np.uint64), first_mean.view(np.uint64))
    # percentiles alone: the mean is not touched
    pct, avg = run_abi(stored, n, E, Wp, ndim, [50.0], mean=False)
    assert (avg == SENTINEL).all()
    with np.errstate(invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        np.testing.assert_array_equal(pct[0], np.percentile(used, 50.0, axis=2))


def fit_model(where):
    return fitted.fitted_model(where, nsteps=40)


def check_model(m, kw):
    chain = m.get_chain(**kw)
    lp = m._sampler.get_log_prob(**kw)
    p = [2.5, 50, 97.5]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        pct = m.get_trace_percentile(p, **kw)
        assert pct.shape == (3, chain.shape[0], m.ndim)
        np.testing.assert_array_equal(pct, np.percentile(chain, p, axis=1))
        np.testing.assert_array_equal(m.get_trace_percentile(**kw), pct)
        one = m.get_trace_percentile(50, **kw)
        assert one.shape == (chain.shape[0], m.ndim)
        np.testing.assert_array_equal(one, pct[1])
        mean = m.get_trace_mean(**kw)
        assert mean.shape == (chain.shape[0], m.ndim)
        W = chain.shape[1]
        assert (np.abs(mean - np.mean(chain, axis=1)) <= W * 2.0 ** -52 * np.mean(np.abs(chain), axis=1)).all()
        got = m.get_log_prob_trace(p, **kw)
        assert got.shape == (3, chain.shape[0])
        np.testing.assert_array_equal(got, np.percentile(lp, p, axis=1))
        np.testing.assert_array_equal(m.get_log_prob_trace(97.5, **kw), got[2])
        # an explicit chain takes the NumPy definition: the same doubles
        np.testing.assert_array_equal(m.get_trace_percentile(p, chain=chain), pct)


@pytest.mark.parametrize('where', ['device', 'host'])
def test_model_traces(where):
    m = fit_model(where)
    kw = dict(discard=10, thin=3)
    check_model(m, kw)
    check_model(m, {})
    with pytest.raises(ValueError, match='no samples'):
        m.get_trace_percentile(discard=40)
    with pytest.raises(ValueError, match='no samples'):
        m.get_log_prob_trace(discard=40)
    with pytest.raises(TypeError, match='flat'):
        m.get_trace_mean(flat=True)
    # a second chunk: several slabs, still one chain
    m._sampler.run_mcmc(None, 25)
    assert m._sampler.iteration == 65
    check_model(m, kw)
    assert m.get_trace_mean(**kw).shape[0] == len(range(12, 65, 3))


def test_plot_traces_of_a_device_chain():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from bisip_amd.trace import used_steps
    m = fit_model('device')
    fig = m.plot_traces(discard=10, thin=3)          # auto: the chain is on the device -> the band
    pct = m.get_trace_percentile(50, discard=10, thin=3)
    for i, ax in enumerate(fig.axes):
        assert len(ax.collections) == 1 and len(ax.lines) == 1
        np.testing.assert_array_equal(ax.lines[0].get_ydata(), pct[:, i])
        np.testing.assert_array_equal(ax.lines[0].get_xdata(), used_steps(40, 10, 3))
    plt.close('all')


def test_spectra_batch_traces():
    import bisip_amd
    from bisip_amd.synthetic import synthetic_columns
    spectra = [bisip_amd.DataFiles()['SIP-K389175']] + [synthetic_columns(20, i) for i in range(2)]
    E, Wp = 3, 16
    b = bisip_amd.SpectraBatch('PolynomialDecomposition', spectra, nwalkers=Wp, nsteps=30, poly_deg=2)
    np.random.seed(5)
    b.fit(seed=11, chain='device')
    assert b._sampler.chain_on_device
    p = [16, 50, 84]
    for kw in (dict(), dict(discard=7, thin=2)):
        chain = b.get_chain(**kw)                    # (n, E, Wp, ndim)
        lp = b.get_log_prob(**kw)                    # (n, E, Wp)
        pct = b.get_trace_percentile(p, **kw)
        assert pct.shape == (3, chain.shape[0], E, b.ndim)
        np.testing.assert_array_equal(pct, np.percentile(chain, p, axis=2))
        np.testing.assert_array_equal(b.get_trace_percentile(84, **kw), pct[2])
        mean = b.get_trace_mean(**kw)
        assert mean.shape == (chain.shape[0], E, b.ndim)
        assert (np.abs(mean - np.mean(chain, axis=2)) <= Wp * 2.0 ** -52 * np.mean(np.abs(chain), axis=2)).all()
        got = b.get_log_prob_trace(p, **kw)
        assert got.shape == (3, chain.shape[0], E)
        np.testing.assert_array_equal(got, np.percentile(lp, p, axis=2))
    with pytest.raises(ValueError, match='no samples'):
        b.get_trace_percentile(discard=30)
    with pytest.raises(ValueError, match='percentiles'):
        b.get_trace_percentile([101])
    b.close()
