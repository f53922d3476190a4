"""Differential-evolution and snooker moves beside the stretch move: the descriptors ``fit(moves=...)`` takes, and the
NumPy statement of the moves and of their random stream, to which the kernels of csrc/move_kernels.h are held bit for
bit (tests/test_gpu_moves.py) and which is itself held to a posterior that is drawn exactly (tests/test_moves.py).

The reference hands ``moves`` to emcee (src/bisip/models.py:84,111-118).  emcee's advice for multimodal targets -- two
Cole-Cole modes sharing one box, whose labellings a chain under the stretch move alone rarely exchanges -- is
``[(DEMove(), 0.8), (DESnookerMove(), 0.2)]``; the descriptors here carry emcee's names and arguments.

Red/blue halves and the active walker of slot ``t`` are the stretch contract's (``sampler.affine_splits``: walker
``pi^-1(2t + h)``).  Partners are members of the complementary half (``Nc`` of them), addressed by rank ``r`` ->
walker ``pi^-1(2r + 1 - h)``.

* **DE** (ter Braak 2006).  Ranks ``a != b``, uniform over ordered pairs; ``gamma = g0 (1 + sigma n)``, ``n ~ N(0,1)``,
  ``g0 = 2.38 / sqrt(2 ndim)`` and ``sigma = 1e-5`` unless given; ``q_k = s_k + gamma (ca_k - cb_k)``; factor 0.
* **Snooker** (ter Braak & Vrugt 2008), ``gammas = 1.7`` unless given.  Three distinct ranks ``z, z1, z2``;
  ``d = s - z``, ``n2 = sum d_k^2``, ``u = d / sqrt(n2)``, ``p1 = sum u_k z1_k``, ``p2 = sum u_k z2_k``,
  ``q_k = s_k + u_k (gammas (p1 - p2))``, ``m2 = sum (q_k - z_k)^2``, factor ``0.5 (ndim - 1) (ln m2 - ln n2)``;
  ``n2 == 0`` is a rejection.  Sums run ``k = 0 .. ndim-1``, multiply then add.
* **Accept** ``(factor + logp(q)) - logp(s) > ln u``.

Deliberately NOT emcee 3's snooker, which divides by ``sqrt(norm)`` and puts ``0.5 (ndim - 1)`` on the log of the norms:
that is not the published move.

The stream extends the Philox contract of csrc/sampler_kernels.h (same key, the counter's fourth word names the purpose;
purposes 0, 1, 2 untouched): purpose 3, counter ``(k, 0, 0, 3)``, picks the iteration's move (``move_schedule``);
purpose 4, counter ``(t, k, h | e << 1, 4)``, the ranks; purpose 5, same counter with 5, the normal deviate; ``ln u``
is the purpose-1 number of the slot (``move_stream``).
"""

import numpy as np

from .sampler import philox4x32_10

MOVE_STRETCH, MOVE_DE, MOVE_SNOOKER = 0, 1, 2      # BISIP_MOVE_* of include/bisip_hip.h
TWO_PI = 6.283185307179586


class StretchMove:
    """Goodman & Weare's stretch move (emcee's default), scale ``a``."""
    kind, name = MOVE_STRETCH, 'stretch'

    def __init__(self, a=2.0):
        self.a = float(a)
        if not self.a > 1.0:
            raise ValueError(f'StretchMove: a={a!r} must be greater than 1')

    def params(self):
        return (self.a,)


class DEMove:
    """Differential evolution: ``q = s + gamma (c_a - c_b)``, ``gamma = gamma0 (1 + sigma n)``; ``gamma0=None`` is
    ``2.38 / sqrt(2 ndim)``."""
    kind, name = MOVE_DE, 'de'

    def __init__(self, sigma=1.0e-5, gamma0=None):
        self.sigma = float(sigma)
        self.gamma0 = None if gamma0 is None else float(gamma0)
        if not np.isfinite(self.sigma) or (self.gamma0 is not None and not np.isfinite(self.gamma0)):
            raise ValueError('DEMove: sigma and gamma0 must be finite')

    def g0(self, ndim):
        return 2.38 / np.sqrt(2.0 * ndim) if self.gamma0 is None else self.gamma0

    def params(self):
        return (self.sigma, self.gamma0)


class DESnookerMove:
    """The snooker update: a jump of ``gammas`` times the projected difference of two walkers along the line
    through a third."""
    kind, name = MOVE_SNOOKER, 'snooker'

    def __init__(self, gammas=1.7):
        self.gammas = float(gammas)
        if not np.isfinite(self.gammas):
            raise ValueError('DESnookerMove: gammas must be finite')

    def params(self):
        return (self.gammas,)


_BY_NAME = {'stretch': StretchMove, 'de': DEMove, 'snooker': DESnookerMove}
_NATIVE = (StretchMove, DEMove, DESnookerMove)


def _is_entry(m):
    return isinstance(m, (str,) + _NATIVE)


def is_native(moves):
    """True when ``moves`` is written with this module's descriptors or strings alone -- one move, a list of moves or a
    list of ``(move, weight)``: what the device sampler runs itself.  Any other object is emcee's business.  (A string
    counts, and so does an empty list: they are then ``parse_moves``' to refuse.)"""
    if _is_entry(moves):
        return True
    if isinstance(moves, (list, tuple)):         # (an empty list is nobody's moves: parse_moves says so)
        return all(_is_entry(m) or (isinstance(m, (list, tuple)) and len(m) == 2 and _is_entry(m[0])) for m in moves)
    return False


def _one(m):
    if isinstance(m, str):
        if m not in _BY_NAME:
            raise ValueError(f"unknown move {m!r}: 'stretch', 'de' or 'snooker'")
        return _BY_NAME[m]()
    if isinstance(m, _NATIVE):
        return m
    raise TypeError(f'not a native move: {m!r}')


def parse_moves(moves):
    """One move, a list of moves (equal weights) or a list of ``(move, weight)`` -> ``(moves, weights)``: the
    descriptors in the order given and their weights as given (float64, positive, finite).  Two entries of one kind
    must agree in their parameters: a kind has one parameter set per run."""
    if _is_entry(moves):
        moves = [moves]
    if not isinstance(moves, (list, tuple)) or not len(moves):
        raise ValueError('moves must be a move, a list of moves or a list of (move, weight)')
    out, weights = [], []
    for m in moves:
        if isinstance(m, (list, tuple)):
            if len(m) != 2:
                raise ValueError(f'a weighted move is (move, weight), got {m!r}')
            out.append(_one(m[0]))
            weights.append(float(m[1]))
        else:
            out.append(_one(m))
            weights.append(1.0)
    weights = np.array(weights, dtype=np.float64)
    if not np.all(np.isfinite(weights)) or np.any(weights <= 0):
        raise ValueError(f'move weights must be positive and finite, got {weights.tolist()}')
    seen = {}
    for m in out:
        if seen.setdefault(m.kind, m.params()) != m.params():
            raise ValueError(f'two {m.name!r} moves with different parameters: a run has one parameter set per kind')
    return out, weights


def u53(a, b):
    """53-bit uniform in [0, 1) from two 32-bit words (csrc/philox.h)."""
    return (((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


def move_schedule(seed, step0, nsteps, weights):
    """Purpose 3: the index of the move of iterations ``step0 .. step0 + nsteps`` -- the first ``j`` with
    ``u < C_j``, ``C_j`` the running sum in the order given of ``w_j / sum w``, the last ``j`` if none; ``u =
    u53(x0, x1)`` of the block with counter ``(k, 0, 0, 3)``.  A pure function of (seed, step)."""
    w = np.asarray(weights, dtype=np.float64)
    k0, k1 = int(seed) & 0xffffffff, int(seed) >> 32
    steps = np.arange(step0, step0 + nsteps, dtype=np.uint64)
    x0, x1, _, _ = philox4x32_10(steps, 0, 0, 3, k0, k1)
    u = u53(x0, x1)
    C = np.cumsum(w / w.sum())
    below = u[:, None] < C[None, :]
    return np.where(below.any(axis=1), below.argmax(axis=1), len(w) - 1).astype(np.int32)


def move_stream(W, seed, step0, perm, g0, sigma=1.0e-5, E=1, e0=0):
    """Purposes 4, 5 and 1 for the ``n = len(perm)`` iterations from ``step0``: ``active``, ``p0``, ``p1``, ``p2``
    (int32 global walker ids ``e W + i``; ``p2`` is 0 where the other half has fewer than three members), ``gamma``
    ``= g0 (1 + sigma n)`` and ``logu``, each ``(n, 2, E * nh)`` as ``bisip_move_draw_dev`` writes them.  ``perm``:
    the rows of ``sampler.affine_splits``; ``e0``: survey index of ensemble 0."""
    n, nh = perm.shape[0], (W + 1) // 2
    ints = {name: np.zeros((n, 2, E, nh), np.int32) for name in ('active', 'p0', 'p1', 'p2')}
    gamma, logu = np.zeros((n, 2, E, nh)), np.zeros((n, 2, E, nh))
    k0, k1 = int(seed) & 0xffffffff, int(seed) >> 32
    es = np.arange(E, dtype=np.int64)[:, None]
    for k in range(n):
        _, Ainv, B = [int(x) for x in perm[k]]

        def walker(y):
            return es * W + (Ainv * ((y - B) % W)) % W

        for h in (0, 1):
            Ns = nh if h == 0 else W // 2
            Nc = W - Ns
            t = np.arange(Ns, dtype=np.uint64)[None, :]
            c2 = h | ((e0 + es) << 1)
            y0, y1, _, _ = philox4x32_10(t, step0 + k, c2, 1, k0, k1)
            x0, x1, x2, _ = philox4x32_10(t, step0 + k, c2, 4, k0, k1)
            n0, n1, n2, n3 = philox4x32_10(t, step0 + k, c2, 5, k0, k1)
            i0 = ((x0 * np.uint64(Nc)) >> np.uint64(32)).astype(np.int64)
            i1 = ((x1 * np.uint64(Nc - 1)) >> np.uint64(32)).astype(np.int64)
            i1 += i1 >= i0
            ints['active'][k, h, :, :Ns] = walker(2 * t.astype(np.int64) + h)
            ints['p0'][k, h, :, :Ns] = walker(2 * i0 + (1 - h))
            ints['p1'][k, h, :, :Ns] = walker(2 * i1 + (1 - h))
            if Nc >= 3:
                i2 = ((x2 * np.uint64(Nc - 2)) >> np.uint64(32)).astype(np.int64)
                i2 += i2 >= np.minimum(i0, i1)
                i2 += i2 >= np.maximum(i0, i1)
                ints['p2'][k, h, :, :Ns] = walker(2 * i2 + (1 - h))
            normal = np.sqrt(-2.0 * np.log(1.0 - u53(n0, n1))) * np.cos(TWO_PI * u53(n2, n3))
            gamma[k, h, :, :Ns] = g0 * (1.0 + sigma * normal)
            with np.errstate(divide='ignore'):
                logu[k, h, :, :Ns] = np.log(u53(y0, y1))
    out = {name: arr.reshape(n, 2, E * nh) for name, arr in ints.items()}
    out['gamma'], out['logu'] = gamma.reshape(n, 2, E * nh), logu.reshape(n, 2, E * nh)
    return out


def de_proposal(s, ca, cb, gamma):
    """``q_k = s_k + gamma (ca_k - cb_k)``: subtract, multiply, add.  Rows ``(m, ndim)``, ``gamma (m,)`` ->
    ``(q, factor)``, factor 0."""
    q = np.empty_like(s)
    for k in range(s.shape[1]):
        q[:, k] = s[:, k] + gamma * (ca[:, k] - cb[:, k])
    return q, np.zeros(s.shape[0])


def snooker_proposal(s, z, z1, z2, gammas):
    """The snooker proposal of rows ``(m, ndim)`` -> ``(q, factor)``; every sum over ``k`` in order, multiply then add
    (no ``np.dot``: its order is BLAS's).  A row with ``n2 == 0`` has no direction: ``q = s`` and factor ``-inf``, a
    rejection under the acceptance rule."""
    m, ndim = s.shape
    u = np.empty_like(s)
    n2 = np.zeros(m)
    for k in range(ndim):
        u[:, k] = s[:, k] - z[:, k]
        n2 = n2 + u[:, k] * u[:, k]
    with np.errstate(divide='ignore', invalid='ignore'):
        norm = np.sqrt(n2)
        p1, p2 = np.zeros(m), np.zeros(m)
        for k in range(ndim):
            u[:, k] = u[:, k] / norm
            p1 = p1 + u[:, k] * z1[:, k]
            p2 = p2 + u[:, k] * z2[:, k]
        jump = gammas * (p1 - p2)
        q = np.empty_like(s)
        m2 = np.zeros(m)
        for k in range(ndim):
            q[:, k] = s[:, k] + u[:, k] * jump
            e = q[:, k] - z[:, k]
            m2 = m2 + e * e
        factor = (0.5 * (ndim - 1)) * (np.log(m2) - np.log(n2))
    none = n2 == 0
    q[none] = s[none]
    factor[none] = -np.inf
    return q, factor
