"""The maximum a posteriori point before any chain exists: a multi-start Levenberg-Marquardt fit of the Gaussian misfit
inside the prior box, with a central-difference Jacobian.  This module holds the definitions in NumPy; the device runs
them in bisip_amd/csrc/dispatch_map.hip (bisip_gauss_newton_dev, bisip_map_fit_dev) and the dense step is
bisip_amd/csrc/lm_step.h (bisip_lm_step_host).

Quantities per parameter j, ``range_j = hi_j - lo_j``: the stencil step ``h_j = 1e-6 range_j`` and the inner box
``[lo_j + h_j, hi_j - h_j]``.  Every iterate is clipped into the inner box, so the stencil never leaves the prior box.  A box
that is not finite is refused.

Normal equations at theta (``normal_equations``; ``ordered_normal_equations`` restates the device's order of sums)::

    d = y - Z(theta)                                      chi2 = sum (d d) iv
    dZ_j = (Z(theta + h_j e_j) - Z(theta - h_j e_j)) / (2 h_j)
    g_j = -sum (dZ_j d) iv                                A_jk = sum (dZ_j dZ_k) iv

with iv = 1 / sigma^2 (fitquality.inverse_variance).  Ordered: every sum over the frequencies in ascending order, the real
part before the imaginary one, from 0.0, every product and sum rounded on its own.

One iteration (``lm_fit``), lambda starting at 1e-3:

1. Free set.  Parameter j is fixed when theta_j sits on the inner lower bound with g_j > 0 or on the inner upper bound with
   g_j < 0, and when A_jj is 0: every dZ_j is 0 then, so are g_j and row and column j of A, and the parameter's step is 0
   whether it counts as free or not; left out, it does not make A_ff singular where the misfit has simply stopped depending
   on it.  Every other parameter is free.
2. Scaling.  D = diag(A_ff) (no entry of it is 0: rule 1).
3. Predicted decrease.  pred = g_f' A_ff^-1 g_f / 2 by Cholesky (``cholesky_free``: the order of lm_step.h); +inf when A_ff
   is not positive definite.  pred <= pred_tol: converged.  max_iter iterations done: cap.
4. Candidates lambda, 10 lambda, ..., at most 12: (A_ff + lambda D) delta = -g_f by Cholesky, a failed factorisation is a
   rejected candidate; trial = clip(theta + delta) onto the inner box.  The first candidate whose chi2 is finite and
   strictly lower is taken and lambda = max(lambda / 10, 1e-12).  None: stalled.

``laplace`` turns the Gauss-Newton Hessian at the optimum into a covariance and an evidence; ``ball`` draws walkers from
it; ``ModelMapFit`` and ``BatchMapFit`` are the ``fit_map`` / ``get_map`` methods of the models and of SpectraBatch."""
import numpy as np

__all__ = ['STEP_REL', 'LAMBDA0', 'LAMBDA_MIN', 'CANDIDATES', 'MAX_ITER', 'STATUS', 'AGREE_TOL', 'inner_box', 'clip', 'stencil',
           'normal_equations', 'ordered_normal_equations', 'ordered_chi2', 'fixed_mask', 'cholesky_free', 'lm_pred',
           'lm_candidate', 'lm_fit', 'device_map_fit', 'laplace', 'ball', 'summarize', 'uniform_starts', 'ModelMapFit', 'BatchMapFit']

STEP_REL = 1e-6
LAMBDA0, LAMBDA_MIN = 1e-3, 1e-12
CANDIDATES = 12
MAX_ITER = 1000
STATUS = {0: 'converged', 1: 'stalled', 2: 'cap'}
AGREE_TOL = 1e-6            # n_agree: starts within this of the best chi2
BALL_FIXED_REL = 1e-3       # ball: the standard deviation of a parameter at a bound, as a fraction of its range
BALL_REDRAWS = 100


def inner_box(bounds):
    """``(h, lo_in, hi_in)`` of bounds (2, ndim); ValueError when the box is not finite."""
    b = np.asarray(bounds, dtype=np.float64)
    if b.ndim != 2 or b.shape[0] != 2:
        raise ValueError('bounds must have shape (2, ndim)')
    if not np.isfinite(b).all():
        raise ValueError('the prior box is not finite: the stencil step is a fraction of it')
    h = STEP_REL * (b[1] - b[0])
    return h, b[0] + h, b[1] - h


def clip(x, lo, hi):
    """x into [lo, hi]; a NaN stays a NaN."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def stencil(theta, h):
    """theta (..., ndim) -> (..., 2 ndim + 1, ndim): theta, theta + h_0 e_0, theta - h_0 e_0, theta + h_1 e_1, ..."""
    theta = np.asarray(theta, dtype=np.float64)
    n = theta.shape[-1]
    pts = np.repeat(theta[..., None, :], 2 * n + 1, axis=-2)
    for j in range(n):
        pts[..., 1 + 2 * j, j] = theta[..., j] + h[j]
        pts[..., 2 + 2 * j, j] = theta[..., j] - h[j]
    return pts


def _parts(Z, y, iv, h):
    Z = np.asarray(Z, dtype=np.float64)
    n = (Z.shape[-3] - 1) // 2
    d = np.asarray(y, dtype=np.float64) - Z[..., 0, :, :]
    J = (Z[..., 1::2, :, :] - Z[..., 2::2, :, :]) / (2.0 * np.asarray(h, dtype=np.float64))[:, None, None]
    iv = np.broadcast_to(np.asarray(iv, dtype=np.float64), d.shape)
    assert J.shape[-3] == n
    return d, J, iv


def normal_equations(Z, y, iv, h):
    """``(chi2, g, A)`` from the responses Z (..., 2 ndim + 1, 2, N) at the points of ``stencil``; y, iv (2, N) or
    broadcastable to (..., 2, N).  The definition: NumPy's own sums."""
    d, J, iv = _parts(Z, y, iv, h)
    chi2 = np.sum(d * d * iv, axis=(-2, -1))
    g = -np.sum(J * d[..., None, :, :] * iv[..., None, :, :], axis=(-2, -1))
    A = np.einsum('...jpf,...kpf,...pf->...jk', J, J, iv)
    return chi2, g, A


def ordered_normal_equations(Z, y, iv, h):
    """``normal_equations`` in the order bisip_gauss_newton_dev states: the same bits from the same responses."""
    d, J, iv = _parts(Z, y, iv, h)
    lead, n, N = d.shape[:-2], J.shape[-3], d.shape[-1]
    chi2, s = np.zeros(lead), np.zeros(lead + (n,))
    A = np.zeros(lead + (n, n))
    for f in range(N):
        for part in (0, 1):
            w, dd, jj = iv[..., part, f], d[..., part, f], J[..., :, part, f]
            chi2 = chi2 + (dd * dd) * w
            s = s + (jj * dd[..., None]) * w[..., None]
            A = A + (jj[..., :, None] * jj[..., None, :]) * w[..., None, None]
    return chi2, -s, A


def ordered_chi2(Z, y, iv):
    """chi2 of responses Z (..., 2, N) in the same order."""
    d = np.asarray(y, dtype=np.float64) - np.asarray(Z, dtype=np.float64)
    iv = np.broadcast_to(np.asarray(iv, dtype=np.float64), d.shape)
    chi2 = np.zeros(d.shape[:-2])
    for f in range(d.shape[-1]):
        for part in (0, 1):
            chi2 = chi2 + (d[..., part, f] * d[..., part, f]) * iv[..., part, f]
    return chi2


# -- the dense step: lm_step.h in NumPy ---------------------------------------------------------------------------------
def fixed_mask(theta, g, A, lo_in, hi_in):
    """(ndim,) bool: on the inner lower bound with g > 0, on the inner upper bound with g < 0, or A_jj = 0."""
    return ((theta <= lo_in) & (g > 0.0)) | ((theta >= hi_in) & (g < 0.0)) | (np.diagonal(A) == 0.0)


def cholesky_free(A, fixed, lam=0.0):
    """The lower factor of ``A_ff + lam D`` (lam <= 0: of A_ff) in the order of lm_step.h, over the free parameters
    compacted; None when it is not positive definite."""
    free = np.flatnonzero(~np.asarray(fixed, dtype=bool))
    M = np.array(A, dtype=np.float64)[np.ix_(free, free)]
    m = free.size
    L = np.zeros((m, m))
    for j in range(m):
        s = M[j, j]
        if lam > 0.0:
            s = s + lam * s
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        if not s > 0.0:
            return None
        L[j, j] = np.sqrt(s)
        if j + 1 < m:
            t = M[j + 1:, j].copy()
            for k in range(j):
                t = t - L[j + 1:, k] * L[j, k]
            L[j + 1:, j] = t / L[j, j]
    return L


def _forward_solve(L, g_f):
    m = L.shape[0]
    z = np.zeros(m)
    zz = 0.0
    for i in range(m):
        t = -g_f[i]
        for k in range(i):
            t = t - L[i, k] * z[k]
        t = t / L[i, i]
        z[i] = t
        zz = zz + t * t
    return z, 0.5 * zz


def _back_solve(L, z):
    m = L.shape[0]
    x = z.copy()
    for i in range(m - 1, -1, -1):
        t = x[i]
        for k in range(i + 1, m):
            t = t - L[k, i] * x[k]
        x[i] = t / L[i, i]
    return x


def lm_pred(A, g, fixed):
    """``g_f' A_ff^-1 g_f / 2``; +inf when A_ff is not positive definite."""
    with np.errstate(all='ignore'):
        L = cholesky_free(A, fixed)
        if L is None:
            return np.inf
        return float(_forward_solve(L, np.asarray(g, dtype=np.float64)[~np.asarray(fixed, dtype=bool)])[1])


def lm_candidate(A, g, theta, fixed, lam, lo_in, hi_in):
    """``(delta, trial)`` of the candidate with this lambda, or None when the factorisation fails."""
    fixed = np.asarray(fixed, dtype=bool)
    with np.errstate(all='ignore'):
        L = cholesky_free(A, fixed, lam)
        if L is None:
            return None
        z, _ = _forward_solve(L, np.asarray(g, dtype=np.float64)[~fixed])
        delta = np.zeros(fixed.size)
        delta[~fixed] = _back_solve(L, z)
    return delta, clip(theta + delta, lo_in, hi_in)


def lm_fit(forward, y, iv, bounds, starts, max_iter=60, pred_tol=1e-8):
    """The loop of the module docstring for any ``forward(theta (W, ndim)) -> (W, 2, N)``, from every row of ``starts``
    (S, ndim); the starts advance together, one call of ``forward`` per stencil and per round of candidates.  Returns a dict
    of theta (S, ndim), chi2, pred (S,), g (S, ndim), hessian (S, ndim, ndim), iterations, status (S,) int64."""
    if not 0 <= int(max_iter) <= MAX_ITER:
        raise ValueError(f'max_iter must lie in [0, {MAX_ITER}]')
    h, lo_in, hi_in = inner_box(bounds)
    theta = clip(np.atleast_2d(np.asarray(starts, dtype=np.float64)), lo_in, hi_in)
    S, n = theta.shape
    y, iv = np.asarray(y, dtype=np.float64), np.asarray(iv, dtype=np.float64)
    lam = np.full(S, LAMBDA0)
    it, status = np.zeros(S, dtype=np.int64), np.full(S, -1, dtype=np.int64)
    chi2, pred = np.full(S, np.nan), np.full(S, np.nan)
    g, A = np.full((S, n), np.nan), np.full((S, n, n), np.nan)
    active = np.arange(S)
    with np.errstate(all='ignore'):
        while active.size:
            Z = np.asarray(forward(stencil(theta[active], h).reshape(-1, n))).reshape(active.size, 2 * n + 1, 2, -1)
            chi2[active], g[active], A[active] = ordered_normal_equations(Z, y, iv, h)
            fixed = {}
            for s in active:
                fixed[s] = fixed_mask(theta[s], g[s], A[s], lo_in, hi_in)
                pred[s] = lm_pred(A[s], g[s], fixed[s])
                if pred[s] <= pred_tol:
                    status[s] = 0
                elif it[s] >= max_iter:
                    status[s] = 2
            pending = [s for s in active if status[s] < 0]
            lam_c = lam.copy()
            for _ in range(CANDIDATES):
                if not pending:
                    break
                tried = [(s, lm_candidate(A[s], g[s], theta[s], fixed[s], lam_c[s], lo_in, hi_in)) for s in pending]
                tried = [(s, c[1]) for s, c in tried if c is not None]
                if tried:
                    c2 = ordered_chi2(np.asarray(forward(np.array([t for _, t in tried]))), y, iv)
                    for (s, t), c in zip(tried, c2):
                        if np.isfinite(c) and c < chi2[s]:
                            theta[s] = t
                            lam[s] = max(lam_c[s] / 10.0, LAMBDA_MIN)
                            it[s] += 1
                            pending.remove(s)
                for s in pending:
                    lam_c[s] = lam_c[s] * 10.0
            for s in pending:
                status[s] = 1
            active = active[status[active] < 0]
    return dict(theta=theta, chi2=chi2, pred=pred, g=g, hessian=A, iterations=it, status=status)


def device_map_fit(ctx, starts, max_iter=60, pred_tol=1e-8, first_spectrum=0):
    """bisip_map_fit_dev around host arrays: starts (n_spectra, S, ndim) [or (S, ndim) for one spectrum] go up once, every
    spectrum and start runs in one launch, and the per-start arrays come back as a dict of theta, chi2, logp, pred, hessian,
    iterations, status and g (the gradient at theta, by bisip_gauss_newton_dev) with the leading axes of ``starts``."""
    import torch
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    lone = starts.ndim == 2
    s3 = starts[None] if lone else starts
    if s3.ndim != 3 or s3.shape[2] != ctx.ndim:
        raise ValueError(f'starts must have shape (n_spectra, S, {ctx.ndim}) or (S, {ctx.ndim}), got {starts.shape}')
    E, S, n = s3.shape
    dev = torch.device('cuda', ctx.device)
    with torch.cuda.device(dev):
        d = torch.from_numpy(s3).to(dev)
        f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        i = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
        out = dict(theta=f(E, S, n), chi2=f(E, S), logp=f(E, S), pred=f(E, S), hessian=f(E, S, n, n), iterations=i(E, S),
                   status=i(E, S))
        stream = torch.cuda.current_stream().cuda_stream
        ctx.map_fit_dev(first_spectrum, E, d.data_ptr(), S, max_iter, pred_tol, *[t.data_ptr() for t in out.values()], stream)
        # the gradient at the results, which decides the fixed set there: the normal equations once more (the kernel's own g)
        out['g'] = f(E, S, n)
        ctx.gauss_newton_dev(first_spectrum, E, out['theta'].data_ptr(), S, 0, out['g'].data_ptr(), 0, stream)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return {k: v[0] for k, v in out.items()} if lone else out


# -- what the optimum gives ----------------------------------------------------------------------------------------------
def laplace(logp, A, at_bound, bounds):
    """``(cov, log_evidence_laplace)`` of the Gauss-Newton Hessian A (ndim, ndim) at the optimum: cov is the inverse of A
    over the parameters that are not in ``at_bound`` (the fit's fixed set), NaN in the rows and columns of the others (all NaN when A_ff is not
    positive definite); ``log_evidence_laplace = logp + (k / 2) log 2 pi - log det A_ff / 2 - sum log range`` over the box,
    NaN when a parameter is at a bound."""
    A = np.asarray(A, dtype=np.float64)
    at_bound = np.asarray(at_bound, dtype=bool)
    b = np.asarray(bounds, dtype=np.float64)
    n = A.shape[0]
    cov = np.full((n, n), np.nan)
    free = np.flatnonzero(~at_bound)
    Aff = A[np.ix_(free, free)]
    try:
        if not np.isfinite(Aff).all():
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(Aff)
    except np.linalg.LinAlgError:
        return cov, np.nan
    Li = np.linalg.inv(L)
    cov[np.ix_(free, free)] = Li.T @ Li
    if at_bound.any():
        return cov, np.nan
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    return cov, float(logp + 0.5 * n * np.log(2.0 * np.pi) - 0.5 * logdet - np.sum(np.log(b[1] - b[0])))


def ball(theta, cov, at_bound, bounds, nwalkers, rng):
    """(nwalkers, ndim) walkers ``theta + L z``, z standard normal from ``rng`` (``standard_normal`` and ``uniform``: a
    RandomState or the numpy.random module), L the Cholesky factor of the Laplace covariance, a parameter at a bound taking
    a standard deviation of 1e-3 of its range (every parameter, when cov is not finite or not positive definite).  A walker
    that is not strictly inside the box is drawn again, and uniformly in the box after 100 redraws."""
    theta = np.asarray(theta, dtype=np.float64)
    b = np.asarray(bounds, dtype=np.float64)
    lo, hi = b[0], b[1]
    n = theta.size
    at_bound = np.asarray(at_bound, dtype=bool)
    C = np.array(cov, dtype=np.float64)
    small = (BALL_FIXED_REL * (hi - lo)) ** 2
    C[at_bound, :] = 0.0
    C[:, at_bound] = 0.0
    C[at_bound, at_bound] = small[at_bound]
    try:
        if not np.isfinite(C).all():
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        L = np.diag(np.sqrt(small))
    out = theta + rng.standard_normal((nwalkers, n)) @ L.T
    for _ in range(BALL_REDRAWS):
        bad = np.flatnonzero(~((out > lo) & (out < hi)).all(axis=1))
        if not bad.size:
            return out
        out[bad] = theta + rng.standard_normal((bad.size, n)) @ L.T
    bad = np.flatnonzero(~((out > lo) & (out < hi)).all(axis=1))
    if bad.size:
        out[bad] = rng.uniform(lo, hi, (bad.size, n))
    return out


def uniform_starts(bounds, shape, seed=None):
    """Starts drawn uniformly in the box from a ``RandomState(seed)`` of their own: NumPy's global state is not touched."""
    b = np.asarray(bounds, dtype=np.float64)
    return np.random.RandomState(seed).uniform(b[0], b[1], tuple(shape) + (b.shape[1],))


def summarize(raw, bounds):
    """The public result of ONE spectrum from the per-start arrays of ``device_map_fit`` (or ``lm_fit`` with a
    ``logp``): theta, logp, chi2, pred, status of the best start (lowest finite chi2), at_bound, hessian, cov,
    log_evidence_laplace, the per-start all_theta, all_logp, all_chi2, all_status, iterations, and n_agree, the number of
    starts within 1e-6 in chi2 of the best.  ``at_bound`` is the fixed set of the fit at the result (``fixed_mask``): a
    parameter on a bound with the gradient pushing outwards -- one on a bound that the gradient pushes inwards is free --
    and one the misfit no longer depends on (A_jj = 0: an element of Shin2015 whose R has gone to its bound takes its Q and
    n along); ``cov`` is NaN in their rows and columns and ``ball`` gives them 1e-3 of their range."""
    chi2 = np.asarray(raw['chi2'], dtype=np.float64)
    fin = np.isfinite(chi2)
    best = int(np.argmin(np.where(fin, chi2, np.inf))) if fin.any() else 0
    theta = np.array(raw['theta'][best], dtype=np.float64)
    _, lo_in, hi_in = inner_box(bounds)
    at = fixed_mask(theta, np.asarray(raw['g'][best]), np.asarray(raw['hessian'][best]), lo_in, hi_in)
    logp = float(raw['logp'][best])
    cov, lz = laplace(logp, raw['hessian'][best], at, bounds)
    return dict(theta=theta, logp=logp, chi2=float(chi2[best]), pred=float(raw['pred'][best]),
                status=STATUS.get(int(raw['status'][best]), 'unknown'), at_bound=at,
                hessian=np.array(raw['hessian'][best], dtype=np.float64), cov=cov, log_evidence_laplace=lz,
                all_theta=np.array(raw['theta']), all_logp=np.array(raw['logp']), all_chi2=chi2.copy(),
                all_status=np.array(raw['status']), iterations=np.array(raw['iterations']),
                n_agree=int(np.sum(chi2 <= chi2[best] + AGREE_TOL)) if fin.any() else 0)


def _check_starts(starts, n_starts, lead, bounds, seed):
    """The starts of a call, ``lead + (S, ndim)``: the caller's, or ``n_starts`` uniform ones."""
    ndim = np.asarray(bounds).shape[1]
    if starts is None:
        if int(n_starts) < 1:
            raise ValueError('n_starts must be at least 1')
        return uniform_starts(bounds, lead + (int(n_starts),), seed)
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    if starts.ndim != len(lead) + 2 or starts.shape[:len(lead)] != lead or starts.shape[-1] != ndim or starts.shape[-2] < 1:
        raise ValueError(f'starts must have shape {lead + ("S", ndim)}, got {starts.shape}')
    return starts


class ModelMapFit:
    """``fit_map`` / ``get_map`` of the models (mixed into bisip_amd.utils.utils)."""

    def fit_map(self, n_starts=32, starts=None, seed=None, max_iter=60, pred_tol=1e-8):
        """The least-squares optimum inside the prior box by Levenberg-Marquardt from ``n_starts`` uniform starts (a
        ``RandomState(seed)`` of its own; or ``starts`` (S, ndim)), every start in one kernel launch.  Returns the dict of
        ``mapfit.summarize``; ``get_map()`` returns it again."""
        bounds = self.param_bounds
        inner_box(bounds)
        starts = _check_starts(starts, n_starts, (), bounds, seed)
        ctx = self._context()
        ctx.set_bounds(bounds)
        self._map = summarize(device_map_fit(ctx, starts, max_iter, pred_tol), bounds)
        return self._map

    def get_map(self):
        """The result of the last ``fit_map`` (or of ``fit(p0='map')``)."""
        got = self.__dict__.get('_map')
        if got is None:
            raise AssertionError('No MAP fit yet: call fit_map() first.')
        return got

    def _map_walkers(self, rng):
        """fit(p0='map'): the walkers in a ball around the optimum (starts of fit_map from RandomState(0))."""
        m = self.fit_map(seed=0)
        return ball(m['theta'], m['cov'], m['at_bound'], self.param_bounds, self.nwalkers, rng)


class BatchMapFit:
    """``fit_map`` / ``get_map`` of SpectraBatch: the same with a leading axis of spectra, all spectra in one call."""

    def fit_map(self, n_starts=32, starts=None, seed=None, max_iter=60, pred_tol=1e-8):
        bounds = self.param_bounds
        inner_box(bounds)
        E = self.n_spectra
        starts = _check_starts(starts, n_starts, (E,), bounds, seed)
        self.ctx.set_bounds(bounds)
        raw = device_map_fit(self.ctx, starts, max_iter, pred_tol)
        one = [summarize({k: v[e] for k, v in raw.items()}, bounds) for e in range(E)]
        self._map = {k: np.array([o[k] for o in one]) for k in one[0]}
        return self._map

    def get_map(self):
        got = self.__dict__.get('_map')
        if got is None:
            raise AssertionError('No MAP fit yet: call fit_map() first.')
        return got

    def _map_walkers(self, rng):
        """fit(p0='map'): the starts of fit_map (RandomState(0)) and one seed per spectrum from ``rng`` are drawn for the
        WHOLE survey and this rank's block kept, as fit(p0=None) draws its starts: a spectrum's optimum, walkers and chain do
        not depend on how the survey is split over ranks."""
        first, last = self.spectrum_range
        m = self.fit_map(starts=uniform_starts(self.param_bounds, (self.n_spectra_total, 32), seed=0)[first:last])
        seeds = rng.randint(0, 2 ** 31 - 1, self.n_spectra_total)[first:last]
        return np.stack([ball(m['theta'][e], m['cov'][e], m['at_bound'][e], self.param_bounds, self.nwalkers,
                              np.random.RandomState(int(seeds[e]))) for e in range(self.n_spectra)])
