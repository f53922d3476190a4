"""What the device-chain summary tests (tests/test_gpu_*.py) share: how used samples are stored behind an offset, a stride
and padding, one guarded call of a C entry point, and the bit-for-bit comparison.  tests/test_chain_harness.py runs all
of it on the CPU."""
import numpy as np

DISCARD, THIN, PAD = 1, 2, 5       # every shape is read through an offset, a stride of two samples and padded samples
SENTINEL = -7.25                   # float outputs start as this; one that is not asked for must come back as this
INT_FILL = -7                      # int64 outputs start as this, so that a count the call does not clear shows
GUARD = 8                          # values after every output that must come back untouched
WORK_FILL, WORK_GUARD = 0xA5, 64   # the bytes after the workspace, and how many


def shape_id(s):
    return 'x'.join(map(str, s))


def store(x, discard=DISCARD, thin=THIN, pad=PAD, filler=1e6):
    """``(stored, offset, stride)``: the used samples x (n, ...) where emcee's get_chain(discard, thin) takes them, at
    discard + thin - 1 and every thin-th after it, of stored (discard + thin * n, row + pad).  ``filler``, a value or a
    callable of the shape, lies between them (not read), NaN in the ``pad`` columns after every sample.  offset and
    stride are in doubles: what the entry points take after ``data_ptr() + 8 * offset``."""
    n = x.shape[0]
    row = x.size // n
    shape = (discard + thin * n, row + pad)
    stored = filler(shape) if callable(filler) else np.full(shape, filler)
    stored[discard + thin - 1::thin, :row] = x.reshape(n, row)
    stored[:, row:] = np.nan
    return stored, (discard + thin - 1) * (row + pad), thin * (row + pad)


def used_window(n_total, row, discard, thin):
    """``(offset, stride, n)`` in doubles of the samples get_chain(discard, thin) keeps of n_total stored ones of ``row``
    doubles each."""
    from bisip_amd.chainview import used_range
    first, n = used_range(n_total, discard, thin)
    return first * row, thin * row, n


class GuardedCall:
    """The outputs and the workspace of one call of an entry point, each followed by values that must come back
    untouched::

        call = GuardedCall()
        mean, cov = call.out('the mean', (E, ndim), asked=want_mean), call.out('the covariance', (E, ndim, ndim))
        _hip.chain_cov_dev(..., mean, cov, call.work(nbytes), nbytes, call.stream)
        mean, cov = call.finish()
    """

    def __init__(self, device='cuda'):
        self.device = device
        self.outputs = []           # (name, tensor, shape, fill, asked)
        self.workspace = None       # (tensor, nbytes)

    def out(self, name, shape, dtype=None, fill=None, asked=True):
        """The pointer to pass for an output of ``shape`` (0 when it is not asked for).  dtype: float64 (None) or int64."""
        import torch
        dtype = dtype or torch.float64
        if fill is None:
            fill = SENTINEL if dtype.is_floating_point else INT_FILL
        t = torch.full((int(np.prod(shape)) + GUARD,), fill, dtype=dtype, device=self.device)
        self.outputs.append((name, t, tuple(shape), fill, asked))
        return t.data_ptr() if asked else 0

    def work(self, nbytes):
        """The pointer to a workspace of exactly nbytes, followed by WORK_GUARD bytes; a null pointer for 0 bytes."""
        import torch
        assert nbytes >= 0 and self.workspace is None
        t = torch.full((nbytes + WORK_GUARD,), WORK_FILL, dtype=torch.uint8, device=self.device)
        self.workspace = (t, nbytes)
        return t.data_ptr() if nbytes else 0

    @property
    def stream(self):
        import torch
        return torch.cuda.current_stream().cuda_stream if torch.device(self.device).type == 'cuda' else 0

    def finish(self):
        """Wait for the call, check every guard and every output not asked for, and return the outputs as NumPy arrays
        of their shapes, in the order they were asked in."""
        import torch
        if torch.device(self.device).type == 'cuda':
            torch.cuda.synchronize()
        if self.workspace is not None:
            t, nbytes = self.workspace
            assert (t[nbytes:].cpu().numpy() == WORK_FILL).all(), 'bytes after the workspace were written'
        results = []
        for name, t, shape, fill, asked in self.outputs:
            host = t.cpu().numpy()
            size = host.size - GUARD
            assert (host[size:] == fill).all(), f'values after {name} were written'
            assert asked or (host == fill).all(), f'{name} was not asked for and was written'
            results.append(host[:size].reshape(shape))
        return results


def assert_same_bits(got, want, what=''):
    """Finite where ``want`` is, and there the same bits (the sign of a zero included)."""
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=what)
    np.testing.assert_array_equal(got[fin].view(np.uint64), want[fin].view(np.uint64), err_msg=what)
