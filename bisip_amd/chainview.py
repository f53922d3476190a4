"""The used samples of a chain on the device, as every posterior summary takes them.

``used_range`` is emcee's discard / thin arithmetic.  A ``ChainView`` says where the used samples lie in a float64
device tensor and carries the stream and allocator the summary works with.  ``_DeviceSlabs`` is how a device sampler
keeps the stored samples of a run there (bisip_amd.sampler writes them, bisip_amd.summaries views them).
``device_moments`` and ``device_percentiles`` are the two summaries that any view has (bisip_chain_moments_dev,
bisip_chain_percentiles_dev); the others are in bisip_amd.autocorr, bisip_amd.histogram and bisip_amd.decomposition.
``moment_splits`` and ``ordered_moments`` are the summation order of bisip_chain_moments_dev in NumPy, bit for bit.
"""

import numpy as np

__all__ = ('used_range', 'ChainView', 'host_chain_view', 'device_moments', 'device_percentiles', 'moment_splits', 'ordered_sweep',
           'ordered_moments')


def used_range(n_total, discard, thin):
    """``(first, n)``: index of the first and number of the samples that ``get_chain(discard, thin)`` keeps of
    ``n_total`` stored ones, ``first`` and every ``thin``-th after it (emcee).  ValueError when there are none."""
    n_total, discard, thin = int(n_total), int(discard), int(thin)
    first = discard + thin - 1
    n = len(range(first, n_total, thin)) if thin >= 1 and discard >= 0 else 0
    if n < 1:
        raise ValueError(f'no samples left with discard={discard}, thin={thin} of {n_total} stored')
    return first, n


class ChainView:
    """Samples ``offset``, ``offset + stride``, ... (in doubles, ``n`` of them) of a float64 device tensor whose
    samples hold ``(n_ensembles * walkers_per_ensemble, ndim)`` rows.  ``stride``: None for a contiguous tensor of
    whole samples.  ``backend``: a HipStretchBackend (its stream and allocator), else torch's current stream on the
    tensor's device."""

    __slots__ = ('tensor', 'n', 'n_ensembles', 'walkers_per_ensemble', 'ndim', 'offset', 'stride', 'backend')

    def __init__(self, tensor, n, n_ensembles, walkers_per_ensemble, ndim, offset=0, stride=None, backend=None):
        import torch
        if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda or tensor.dtype != torch.float64:
            raise TypeError('the chain must be a float64 tensor on the GPU')
        n, E, Wp, ndim, offset = int(n), int(n_ensembles), int(walkers_per_ensemble), int(ndim), int(offset)
        if n < 1:
            raise ValueError('no samples')
        row = E * Wp * ndim
        if stride is None:
            if not tensor.is_contiguous():
                raise ValueError('a chain that is not contiguous needs an explicit sample_stride')
            stride = row
        stride = int(stride)
        if stride < row or offset < 0 or offset + (n - 1) * stride + row > tensor.numel():
            raise ValueError('the samples asked for lie outside the chain tensor')
        self.tensor, self.n, self.n_ensembles, self.walkers_per_ensemble, self.ndim = tensor, n, E, Wp, ndim
        self.offset, self.stride, self.backend = offset, stride, backend

    @classmethod
    def of_tensor(cls, x):
        """One ensemble: every sample of a device tensor ``(n, walkers, ndim)``, copied first if not contiguous."""
        n, Wp, ndim = x.shape
        return cls(x.contiguous(), n, 1, Wp, ndim)

    def derived(self, tensor):
        """The view of every sample of a new contiguous tensor ``(n, n_ensembles * walkers_per_ensemble, k)`` of
        quantities derived row by row from this one's samples, on the same backend."""
        return ChainView(tensor, self.n, self.n_ensembles, self.walkers_per_ensemble, tensor.shape[-1],
                         backend=self.backend)

    @property
    def ptr(self):
        return self.tensor.data_ptr() + 8 * self.offset

    @property
    def stream(self):
        if self.backend is not None:
            return self.backend.stream()
        import torch
        return torch.cuda.current_stream(self.tensor.device).cuda_stream

    def synchronize(self):
        if self.backend is not None:
            return self.backend.synchronize()
        import torch
        torch.cuda.current_stream(self.tensor.device).synchronize()

    def empty(self, shape, dtype):
        if self.backend is not None:
            return self.backend.empty(shape, dtype)
        import torch
        return torch.empty(shape, dtype=dtype, device=self.tensor.device)

    def upload(self, array):
        import torch
        a = np.array(array, dtype=np.float64, order='C')      # (a writable copy: broadcast views are read-only)
        t = self.empty(a.shape, torch.float64)
        t.copy_(torch.from_numpy(a))
        return t

    def samples(self):
        """The used samples as a strided tensor ``(n, n_ensembles * walkers_per_ensemble, ndim)``: no copy."""
        import torch
        t = self.tensor
        return torch.as_strided(t, (self.n, self.n_ensembles * self.walkers_per_ensemble, self.ndim),
                                (self.stride, self.ndim, 1), t.storage_offset() + self.offset)


def host_chain_view(flat, ctx):
    """The view of a host chain ``(n, ndim)`` of the model of ``ctx`` (a HipContext) as one ensemble of one walker.  The
    chain goes up once, to the context's device; its rows are the rows of get_chain(flat=True), so that a pass over the
    view takes the same sums in the same order as one over the chain where a sampler left it."""
    import torch
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    if flat.ndim != 2 or flat.shape[1] != ctx.ndim or flat.shape[0] < 1:
        raise ValueError(f'the chain must be (n, {ctx.ndim}), n >= 1, got {flat.shape}')
    t = torch.from_numpy(flat).to(torch.device('cuda', ctx.device))
    return ChainView(t, flat.shape[0], 1, 1, ctx.ndim)


class _DeviceSlabs:
    """Stored samples that stay in device memory (one torch tensor per chunk).  Behaves like a chain part for the
    bookkeeping (``shape``) and becomes a host array the first time the host asks for it."""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    @property
    def shape(self):
        return (sum(int(t.shape[0]) for t in self.tensors),) + tuple(self.tensors[0].shape[1:])

    def tensor(self):
        if len(self.tensors) > 1:
            import torch
            self.tensors = [torch.cat(self.tensors, dim=0)]
        return self.tensors[0]

    def materialize(self):
        """Host copy, made once; the samples also stay on the device for the summaries."""
        if getattr(self, '_host', None) is None:
            self._host = self.tensor().cpu().numpy()
        return self._host


def _merge_device_parts(parts):
    """True when the parts of a stored chain (one per run) all lie on the device; they then become ONE part, merged
    where they lie.  False, and nothing changes, when there are none or some are host arrays."""
    if not parts or not all(isinstance(p, _DeviceSlabs) for p in parts):
        return False
    if len(parts) > 1:
        parts[:] = [_DeviceSlabs(t for p in parts for t in p.tensors)]
    return True


def device_moments(view):
    """``np.mean`` / ``np.std`` over every ensemble's samples of a view: ``(mean, std)``, ``(n_ensembles, ndim)``
    each (NumPy)."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    mean, std = view.empty((E, ndim), torch.float64), view.empty((E, ndim), torch.float64)
    work = view.empty((max(1, _hip.chain_moments_workspace(n, E, ndim)),), torch.float64)
    _hip.chain_moments_dev(view.ptr, n, view.stride, E, Wp, ndim, mean.data_ptr(), std.data_ptr(), work.data_ptr(),
                           view.stream)
    view.synchronize()
    return mean.cpu().numpy(), std.cpu().numpy()


# -- the device's order of summation ------------------------------------------------------------------------------------
MOMENT_WORKGROUPS, MOMENT_SPLIT_MIN, MOMENT_THREADS = 4096, 4, 256      # chain_moments.hip: moment_splits, the block


def moment_splits(n_samples, n_ensembles):
    """Into how many ranges of samples bisip_chain_moments_dev cuts a chain: ``max(1, min(ceil(4096 / E), n / 4))`` -- a
    function of the shape alone.  Split ``sp`` takes samples ``[n * sp // splits, n * (sp + 1) // splits)``; its workspace
    is ``E * splits * ndim`` doubles."""
    n, E = int(n_samples), int(n_ensembles)
    return max(1, min(-(-MOMENT_WORKGROUPS // E), n // MOMENT_SPLIT_MIN))


def exact_fma(a, b, c):
    """``a * b + c`` of three doubles with one rounding (IEEE fusedMultiplyAdd, round to nearest even), in rational
    arithmetic: Python 3.10 has no math.fma."""
    import math
    from fractions import Fraction
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(all='ignore'):
            return float(np.float64(a) * np.float64(b) + np.float64(c))       # (the product is inf or NaN exactly)
    if not math.isfinite(c):
        return c                                                             # (a finite product, however large)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        if a * b == 0.0:                 # (a zero product is exact: the sum of two zeros has IEEE's sign)
            return a * b + c
        return 0.0                       # x + (-x): +0 when rounding to nearest
    try:
        r = float(exact)                 # (int / int is correctly rounded, subnormals included)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf
    return -0.0 if r == 0.0 and exact < 0 else r


def _ensemble_rows(x, n_ensembles):
    """``(v (n, E, Wp * ndim), n, E, Wp, ndim, lanes)`` of a chain ``(n, E * Wp, ndim)``: every ensemble's doubles of a
    sample as the moments kernels sweep them, and how many of their 256 lanes work."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError('the chain must be (n, walkers, ndim)')
    n, W, ndim = x.shape
    E = int(n_ensembles)
    if n < 1 or W < 1 or ndim < 1 or E < 1 or W % E:
        raise ValueError(f'a chain {x.shape} does not divide into {E} ensembles')
    lanes = (MOMENT_THREADS // ndim) * ndim
    if lanes < 1:
        raise ValueError(f'ndim={ndim} out of range')
    return x.reshape(n, E, (W // E) * ndim), n, E, W // E, ndim, lanes


def ordered_sweep(v, ndim, lanes, term):
    """One sweep of the moments kernels over ``v (n, E, Wp * ndim)`` in their stated order, ``(E, ndim)``: ``term(acc (E,
    k), values (E, k), k)`` gives the accumulators of lanes ``0 ... k - 1`` after one more value each (lane ``t`` holds
    parameter ``t % ndim``)."""
    n, E, length = v.shape
    splits = moment_splits(n, E)
    # the doubles i ... i + k - 1 of a sample go to lanes 0 ... k - 1 (a lane beyond the last double adds nothing)
    turns = [(i, min(lanes, length - i)) for i in range(0, length, lanes)]

    def add(acc, s, i, k):
        acc[:, :k] = term(acc[:, :k], v[s, :, i:i + k], k)

    total = np.zeros((E, ndim))
    for sp in range(splits):
        s, s1 = n * sp // splits, n * (sp + 1) // splits
        acc = np.zeros((4, E, lanes))
        while s + 4 <= s1:
            for i, k in turns:                       # for each double of the lane in turn, sample s + j to j
                for j in range(4):
                    add(acc[j], s + j, i, k)
            s += 4
        while s < s1:
            for i, k in turns:
                add(acc[0], s, i, k)
            s += 1
        lane = (acc[0] + acc[1]) + (acc[2] + acc[3])
        part = np.zeros((E, ndim))
        for k in range(lanes // ndim):
            part = part + lane[:, k * ndim:(k + 1) * ndim]
        total = total + part
    return total


def ordered_moments(x, n_ensembles=1):
    """``(mean, std)``, ``(n_ensembles, ndim)`` each, of a chain ``(n, n_ensembles * Wp, ndim)`` with the bits
    bisip_chain_moments_dev produces, in the order include/bisip_hip.h states: samples in ``moment_splits`` ranges; lane
    ``t`` of ``(256 // ndim) * ndim`` owns the doubles ``t, t + lanes, ...`` of the ensemble's ``Wp * ndim`` of a sample;
    four accumulators per lane over groups of four samples, the left-over samples to the first, ``(a0 + a1) + (a2 + a3)``;
    lanes of a parameter, then splits, in ascending order.  The second pass is ``fma(d, d, acc)`` with ``d = x - mean``,
    taken exactly value by value in Python (``exact_fma``): some 10 us per value, so this is for chains of a few ten
    thousand values -- the small shapes of the tests -- and not for a fit's."""
    v, n, E, Wp, ndim, lanes = _ensemble_rows(x, n_ensembles)
    fma = np.frompyfunc(exact_fma, 3, 1)

    def squares(mean):
        m = np.tile(mean, (1, lanes // ndim))        # lane t: parameter t % ndim

        def term(acc, values, k):
            d = values - m[:, :k]
            return fma(d, d, acc).astype(np.float64)
        return term

    with np.errstate(all='ignore'):
        count = float(n) * float(Wp)
        mean = ordered_sweep(v, ndim, lanes, lambda acc, values, k: acc + values) / count
        std = np.sqrt(ordered_sweep(v, ndim, lanes, squares(mean)) / count)
    return mean, std


def device_percentiles(view, p):
    """``np.percentile`` over every ensemble's samples of a view, sorted and interpolated on the device:
    ``(len(p), n_ensembles, ndim)`` (NumPy)."""
    import torch
    from . import _hip
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    nbytes = _hip.chain_percentiles_workspace(n, E, Wp, ndim, p.size)
    if nbytes <= 0:
        raise ValueError('chain too large for one device sort (more than 2^31 values); thin it or use get_chain()')
    work = view.empty((nbytes,), torch.uint8)
    out = view.empty((p.size, E, ndim), torch.float64)
    _hip.chain_percentiles_dev(view.ptr, n, view.stride, E, Wp, ndim, p, out.data_ptr(), work.data_ptr(), nbytes,
                               view.stream)
    view.synchronize()
    return out.cpu().numpy()
