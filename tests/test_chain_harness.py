"""tests/chain_harness.py on the CPU: it is what stands between a kernel that writes out of bounds and a green run of
the device-chain tests, so its storage, its guards and its comparison are held to their own statements here."""
import ctypes

import numpy as np
import pytest
import torch

import chain_harness as ch
import moments_bounds
from bisip_amd.chainview import used_range

STORAGE = [(1, 0, 1, 0), (1, 1, 2, 5), (3, 1, 2, 5), (4, 7, 3, 1)]          # (n, discard, thin, pad)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def strided(flat, offset, stride, n, row):
    """What an entry point reads: n samples of row doubles, ``stride`` apart, from ``offset`` on."""
    return torch.from_numpy(flat.reshape(-1)).as_strided((n, row), (stride, 1), offset).numpy()


@pytest.mark.parametrize('n,discard,thin,pad', STORAGE)
def test_store(n, discard, thin, pad):
    x = np.random.default_rng(n + discard).normal(size=(n, 3, 2))
    x[0, 0, 0] = -0.0
    row = 6
    first = discard + thin - 1
    unused = np.ones(discard + thin * n, dtype=bool)
    unused[first::thin] = False
    ramp = lambda shape: np.arange(np.prod(shape), dtype=np.float64).reshape(shape) + 0.5
    for kw, filling in ((dict(), lambda s: np.full(s.shape, 1e6)), (dict(filler=ramp), lambda s: ramp(s.shape))):
        stored, offset, stride = ch.store(x, discard, thin, pad, **kw)
        width = row + pad
        assert stored.shape == (discard + thin * n, width) and stored.dtype == np.float64
        np.testing.assert_array_equal(bits(stored[first::thin, :row]), bits(x.reshape(n, row)))
        np.testing.assert_array_equal(bits(strided(stored, offset, stride, n, row)), bits(x.reshape(n, row)))
        assert offset % width == 0 and stride == thin * width
        assert (offset // width, n) == used_range(stored.shape[0], discard, thin)
        assert np.isnan(stored[:, row:]).all()
        np.testing.assert_array_equal(stored[unused, :row], filling(stored)[unused, :row])
    # the defaults are the constants, and a two-dimensional x (a log-probability) is a row of its own width
    stored, offset, stride = ch.store(x[:, :, 0])
    assert stored.shape == (ch.DISCARD + ch.THIN * n, 3 + ch.PAD)
    assert (offset, stride) == ((ch.DISCARD + ch.THIN - 1) * (3 + ch.PAD), ch.THIN * (3 + ch.PAD))


@pytest.mark.parametrize('n,discard,thin,pad', STORAGE)
def test_used_window(n, discard, thin, pad):
    for extra in (0, thin - 1):                                     # stored samples after the last used one
        full = np.random.default_rng(thin).normal(size=(discard + thin * n + extra, 4, 3))
        offset, stride, count = ch.used_window(full.shape[0], 12, discard, thin)
        want = full[discard + thin - 1::thin]
        assert count == want.shape[0] == n
        np.testing.assert_array_equal(bits(strided(full, offset, stride, count, 12)), bits(want.reshape(n, 12)))
    with pytest.raises(ValueError, match='no samples'):
        ch.used_window(discard + thin - 1, 12, discard, thin)


def poke(ctype, address, value):
    """What a kernel that writes where it should not does: one value at an address."""
    ctype.from_address(address).value = value


def a_call(dtype, nbytes, asked=True):
    call = ch.GuardedCall(device='cpu')
    first = call.out('the first', (2, 3), dtype)
    second = call.out('the second', (5,), dtype, asked=asked)
    return call, first, second, call.work(nbytes)


@pytest.mark.parametrize('nbytes', [0, 1, 300])
@pytest.mark.parametrize('dtype,ctype,fill', [(torch.float64, ctypes.c_double, ch.SENTINEL),
                                              (torch.int64, ctypes.c_int64, ch.INT_FILL)], ids=['float64', 'int64'])
def test_guarded_call(dtype, ctype, fill, nbytes):
    width = 8
    # untouched, and written where it may be
    call, first, second, work = a_call(dtype, nbytes)
    assert call.stream == 0
    assert first and second and (work == 0) == (nbytes == 0)
    poke(ctype, first + 5 * width, 3)
    poke(ctype, second, 4)
    if nbytes:
        poke(ctypes.c_uint8, work + nbytes - 1, 0)
    a, b = call.finish()
    assert a.shape == (2, 3) and b.shape == (5,) and a.dtype == b.dtype == (np.float64 if fill == ch.SENTINEL else np.int64)
    assert a[1, 2] == 3 and b[0] == 4 and (a.ravel()[:5] == fill).all() and (b[1:] == fill).all()
    # one element just past an output: that output is named
    for name, size in (('first', 6), ('second', 5)):
        call, first, second, work = a_call(dtype, nbytes)
        poke(ctype, (first if name == 'first' else second) + size * width, 3)
        with pytest.raises(AssertionError, match=f'after the {name} were written'):
            call.finish()
    # the last value of the guard
    call, first, second, work = a_call(dtype, nbytes)
    poke(ctype, second + (5 + ch.GUARD - 1) * width, 3)
    with pytest.raises(AssertionError, match='after the second were written'):
        call.finish()
    # one byte just past the workspace, and the last one of its guard
    for at in (nbytes, nbytes + ch.WORK_GUARD - 1):
        call, first, second, work = a_call(dtype, nbytes)
        poke(ctypes.c_uint8, call.workspace[0].data_ptr() + at, 0)
        with pytest.raises(AssertionError, match='after the workspace were written'):
            call.finish()
    # an output that was not asked for: a null pointer, and nothing may be written to it
    call, first, second, work = a_call(dtype, nbytes, asked=False)
    assert second == 0
    a, b = call.finish()
    assert (a == fill).all() and (b == fill).all()
    call, first, second, work = a_call(dtype, nbytes, asked=False)
    poke(ctype, call.outputs[1][1].data_ptr() + 2 * width, 3)
    with pytest.raises(AssertionError, match='the second was not asked for'):
        call.finish()


def test_guarded_call_takes_the_workspace_as_it_is_asked():
    call = ch.GuardedCall(device='cpu')
    call.work(300)
    t, nbytes = call.workspace
    assert nbytes == 300 and t.numel() == 300 + ch.WORK_GUARD and (t.numpy() == ch.WORK_FILL).all()
    assert ch.WORK_FILL == 0xA5 and ch.SENTINEL == -7.25 and ch.INT_FILL == -7
    assert ch.GuardedCall(device='cpu').finish() == []              # a call without outputs or workspace


def test_assert_same_bits():
    nans = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001, 0xfff0000000000123],
                    dtype=np.uint64).view(np.float64)
    assert np.isnan(nans).all()
    want = np.concatenate([[1.0, -0.0, 0.0, 5e-324, np.inf, -np.inf], np.full(4, np.nan)])
    got = np.concatenate([want[:6], nans])
    for same in (ch.assert_same_bits, moments_bounds.assert_same_bits):
        same(want, want, 'itself')
        same(got, want, 'NaN of either sign and any payload')
        for i, other in ((0, np.nextafter(1.0, 2.0)), (0, np.nextafter(1.0, 0.0)), (1, 0.0), (2, -0.0), (3, 0.0),
                         (0, np.nan), (6, 1.0), (0, np.inf), (4, 1.0)):
            g = want.copy()
            g[i] = other
            with pytest.raises(AssertionError):
                same(g, want, 'differs')
        with pytest.raises(AssertionError, match='the label'):
            same(np.array([1.0]), np.array([2.0]), 'the label')
    # only ``isfinite`` is compared where ``want`` is not finite: the shared function takes +inf for -inf and an infinity
    # for a NaN, as the three copies it replaces did; the moments' stricter one refuses both
    for i, other in ((4, -np.inf), (5, np.inf), (4, np.nan), (6, np.inf)):
        g = want.copy()
        g[i] = other
        ch.assert_same_bits(g, want)
        with pytest.raises(AssertionError):
            moments_bounds.assert_same_bits(g, want)


def test_shape_id():
    assert ch.shape_id((7, 2, 65, 7)) == '7x2x65x7' and ch.shape_id((1,)) == '1'
