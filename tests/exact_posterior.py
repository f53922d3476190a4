"""A posterior of this project that can be drawn exactly, and the statistics that hold a sampler to it.

PolynomialDecomposition is linear in ``b = R0 * (1, a)`` (oracle/oracle.py, numpy_forward): ``Z = G b`` with a fixed real
``(2N, P+2)`` design.  Under the uniform box in ``theta = (R0, a_0 .. a_P)`` the posterior density of ``b`` is therefore
a Gaussian ``N(b_hat, H^-1)`` times the Jacobian ``|d theta / d b| = b0^-(P+1)`` times the indicator of the box, and
rejection sampling draws it exactly: propose from the Gaussian, keep a proposal inside the open box with probability
``(lo_r0 / b0)^(P+1) <= 1``.

An ensemble whose walkers all start at such draws is stationary from step 0, so the expectation of every stored sample
of a correct sampler is the posterior's, with no burn-in term; E independent ensembles give a standard error of their
mean that uses nothing of the code under test.  ``t_statistics`` compares the two, ``t_limit`` is the Student-t
quantile they are held to.  NumPy (and scipy.stats for the quantile) only; no GPU.
"""

import functools

import numpy as np

N_REF = 1 << 19            # reference draws per case: their error is in T's denominator, and small beside the ensembles'
FAMILY_ERROR = 1e-3        # chance that a correct sampler fails one case
QUANTILES = (0.1, 0.5, 0.9)


class Problem:
    """Operands of one synthetic spectrum as SpectraBatch builds them, the linear form of the model and its
    exact posterior under the box ``(lo, hi)``."""

    def __init__(self, n_freq, poly_deg, spectrum_index=1, c_exp=1.0, lo=None, hi=None):
        from bisip_amd.batch import default_params
        from bisip_amd.synthetic import synthetic_columns
        from bisip_amd.utils import tables_to_operands
        self.n_freq, self.poly_deg, self.c_exp = int(n_freq), int(poly_deg), float(c_exp)
        self.table = synthetic_columns(n_freq, spectrum_index)
        ops = tables_to_operands(self.table[None])                      # the load arithmetic of a batch
        self.w, self.zn, self.zn_err = ops['w'][0], ops['zn'][0], ops['zn_err'][0]
        N = self.N = self.w.size
        # the tau grid of bisip_amd/batch.py (one spectrum: the reference's per-file grid)
        period = np.log10(1. / self.w)
        self.log_tau = np.linspace(np.floor(period.min() - 1), np.floor(period.max() + 1), 2 * N)
        self.log_taus = np.array([self.log_tau ** i for i in range(poly_deg + 1)])
        self.taus = 10 ** self.log_tau
        box = np.array(list(default_params('PolynomialDecomposition', poly_deg=poly_deg).values()), dtype=np.float64).T
        self.lo = box[0].copy() if lo is None else np.array(lo, dtype=np.float64)
        self.hi = box[1].copy() if hi is None else np.array(hi, dtype=np.float64)
        self.ndim = poly_deg + 2
        assert self.lo.shape == self.hi.shape == (self.ndim,) and self.lo[0] > 0
        # Z = G b: column 0 is 1 (real part), column 1+i is -sum_k log_tau_k^i (1 - 1/(1 + (j w tau_k)^c))
        debye = 1 - 1.0 / (1 + (1j * self.w[:, None] * self.taus[None, :]) ** self.c_exp)      # (N, L)
        cols = [np.ones(N, dtype=np.complex128)] + [-(debye * self.log_taus[i]).sum(axis=1) for i in range(poly_deg + 1)]
        Gc = np.stack(cols, axis=1)
        self.G = np.concatenate([Gc.real, Gc.imag], axis=0)             # (2N, P+2), rows as zn.ravel()
        self.y = self.zn.ravel()
        self.sigma = self.zn_err.ravel()
        self.const = -np.sum(np.log(self.sigma ** 2))
        # whitened least squares through a QR (the normal matrix is only formed to be recorded): A = Q R,
        # H = A^T A = R^T R, so R^T is the Cholesky factor of H once R's diagonal is made positive
        A = self.G / self.sigma[:, None]
        Q, R = np.linalg.qr(A)
        s = np.sign(np.diag(R))
        Q, R = Q * s, R * s[:, None]
        self.chol = R.T.copy()
        self.H = A.T @ A
        self.b_hat = np.linalg.solve(R, Q.T @ (self.y / self.sigma))
        self.R_inv = np.linalg.solve(R, np.eye(self.ndim))              # b = b_hat + R^-1 z,  z ~ N(0, I)
        self.cond = float(np.linalg.cond(R) ** 2)                       # cond(H)
        # float64 is accepted while cond * 2^-53 <= 1e-4; a case beyond that is not loosened but dropped
        if self.cond * 2.0 ** -53 > 1e-4:
            raise ValueError(f'cond(H) = {self.cond:.2e}: this case needs more than float64')

    # -- what the other layers take ------------------------------------------------------------------------------
    @property
    def bounds(self):
        return np.array([self.lo, self.hi])

    def oracle_problem(self):
        import oracle
        return oracle.OracleProblem('PolynomialDecomposition', self.w, self.zn, self.zn_err, self.bounds,
                                    taus=self.taus, log_taus=self.log_taus, c_exp=self.c_exp)

    # -- the log-probability -------------------------------------------------------------------------------------
    def logp(self, theta):
        """``-1/2 |Sigma^-1/2 (G b - y)|^2 - sum log sigma^2``; ``-inf`` outside the OPEN box.  theta (..., ndim)."""
        theta = np.asarray(theta, dtype=np.float64)
        flat = theta.reshape(-1, self.ndim)
        out = np.full(flat.shape[0], -np.inf)
        inside = np.all((flat > self.lo) & (flat < self.hi), axis=1)
        for i in range(0, flat.shape[0], 1 << 16):
            rows = np.flatnonzero(inside[i:i + (1 << 16)]) + i
            th = flat[rows]
            b = np.concatenate([th[:, :1], th[:, 1:] * th[:, :1]], axis=1)
            r = (b @ self.G.T - self.y) / self.sigma
            out[rows] = -0.5 * np.einsum('ij,ij->i', r, r) + self.const
        return out.reshape(theta.shape[:-1])

    # -- exact draws ---------------------------------------------------------------------------------------------
    def gaussian_b(self, n, rng):
        return self.b_hat + rng.standard_normal((n, self.ndim)) @ self.R_inv.T

    def exact_draws(self, n, rng):
        """``n`` independent draws of theta from the posterior, and the acceptance rate of the rejection."""
        out, have, tried, kept = np.empty((n, self.ndim)), 0, 0, 0
        while have < n:
            m = max(1024, int(1.3 * (n - have) / max(kept / tried if tried else 0.3, 0.02)))
            m = min(m, 1 << 20)
            b = self.gaussian_b(m, rng)
            with np.errstate(divide='ignore', invalid='ignore'):
                theta = np.concatenate([b[:, :1], b[:, 1:] / b[:, :1]], axis=1)
                ok = np.all((theta > self.lo) & (theta < self.hi), axis=1)
                # the Jacobian b0^-(P+1), relative to its largest value in the box (at b0 = lo_r0)
                ok &= rng.random_sample(m) < np.where(ok, (self.lo[0] / b[:, 0]) ** (self.poly_deg + 1), 0.0)
            good = theta[ok]
            tried, kept = tried + m, kept + good.shape[0]
            take = min(n - have, good.shape[0])
            out[have:have + take] = good[:take]
            have += take
        return out, kept / tried

    # -- features and their reference ----------------------------------------------------------------------------
    def feature_names(self):
        x = ['r0'] + [f'a{i}' for i in range(self.poly_deg + 1)]
        iu = np.triu_indices(self.ndim)
        return x + [f'({x[i]}-mu)({x[j]}-mu)' for i, j in zip(*iu)] + [f'logp>=q{int(100 * q)}' for q in QUANTILES]

    def features(self, x, mu, q, logp=None):
        """x (..., ndim) -> (..., F): the coordinates, the upper triangle of (x-mu)(x-mu)^T about the FIXED mu -- unbiased
        under stationarity whatever the autocorrelation, unlike a per-ensemble sample variance -- and the indicators
        ``logp >= q`` (``logp``: the helper's own of x unless given, e.g. the sampler's stored one)."""
        x = np.asarray(x, dtype=np.float64)
        d = x - mu
        iu = np.triu_indices(self.ndim)
        lp = self.logp(x) if logp is None else np.asarray(logp)
        ind = (lp[..., None] >= np.asarray(q)).astype(np.float64)
        return np.concatenate([x, d[..., iu[0]] * d[..., iu[1]], ind], axis=-1)

    def reference(self, n=N_REF, seed=20240229):
        """mu, the logp quantiles and the mean / variance of every feature, from ``n`` exact draws only."""
        rng = np.random.RandomState(seed)
        draws, rate = self.exact_draws(n, rng)
        mu = draws.mean(axis=0)
        lp = self.logp(draws)
        q = np.quantile(lp, QUANTILES)
        total, total2 = 0.0, 0.0
        for i in range(0, n, 1 << 16):
            f = self.features(draws[i:i + (1 << 16)], mu, q, lp[i:i + (1 << 16)])
            total, total2 = total + f.sum(axis=0), total2 + (f * f).sum(axis=0)
        mean = total / n
        var = (total2 - n * mean * mean) / (n - 1)
        return dict(mu=mu, sd=draws.std(axis=0, ddof=1), q=q, mean=mean, var=var, n=n, rate=rate, names=self.feature_names())

    def t_statistics(self, chain, ref, logp=None):
        """chain (n, E, W, ndim) of E independent ensembles (or runs) -> T per feature:
        ``(mean_e - mean_ref) / sqrt(var_e / E + var_ref / N_ref)`` with the per-ensemble means of the features over
        samples and walkers, ddof = 1.  With ``logp`` (n, E, W), the stored log-probability stands for logp(x)."""
        chain = np.asarray(chain)
        n, E, W, ndim = chain.shape
        per = np.empty((E, ref['mean'].size))
        for e in range(E):
            f = self.features(chain[:, e], ref['mu'], ref['q'], None if logp is None else np.asarray(logp)[:, e])
            per[e] = f.reshape(n * W, -1).mean(axis=0)
        mean_e, var_e = per.mean(axis=0), per.var(axis=0, ddof=1)
        return (mean_e - ref['mean']) / np.sqrt(var_e / E + ref['var'] / ref['n'])


    @staticmethod
    def t_statistics_logp(logp, ref):
        """The same T for the three indicators alone, from a stored log-probability (n, E, W)."""
        logp = np.asarray(logp)
        E, k = logp.shape[1], len(QUANTILES)
        per = (logp[..., None] >= ref['q']).astype(np.float64).transpose(1, 0, 2, 3).reshape(E, -1, k).mean(axis=1)
        mean_e, var_e = per.mean(axis=0), per.var(axis=0, ddof=1)
        return (mean_e - ref['mean'][-k:]) / np.sqrt(var_e / E + ref['var'][-k:] / ref['n'])


@functools.lru_cache(maxsize=None)
def problem(n_freq, poly_deg, spectrum_index=1, c_exp=1.0, lo=None, hi=None):
    """The exact-posterior problem of one synthetic spectrum (cached: ``lo`` / ``hi`` as tuples or None)."""
    return Problem(n_freq, poly_deg, spectrum_index, c_exp, lo, hi)


@functools.lru_cache(maxsize=None)
def reference(prob):
    """The reference of ``prob``, computed once per process and never modified."""
    return prob.reference()


def truncated_problem():
    """(8, 2) with three faces moved into the posterior, mu and sd from the reference draws of the uncut case:
    hi[a0] = mu + 0.5 sd, lo[a2] = mu - sd, hi[r0] = mu + sd."""
    base = problem(8, 2)
    ref = reference(base)
    lo, hi = base.lo.copy(), base.hi.copy()
    hi[1] = ref['mu'][1] + 0.5 * ref['sd'][1]
    lo[3] = ref['mu'][3] - ref['sd'][3]
    hi[0] = ref['mu'][0] + ref['sd'][0]
    return problem(8, 2, lo=tuple(lo), hi=tuple(hi))


def face_rows(prob, rng, n_per_face=2, eps=1e-9):
    """Rows just inside and just outside every face of the box, the other coordinates at exact draws:
    ``(inside, outside)``, each (2 * ndim * n_per_face, ndim).  ``eps`` is relative to the width of the box."""
    base, _ = prob.exact_draws(2 * prob.ndim * n_per_face, rng)
    inside, outside = base.copy(), base.copy()
    width = prob.hi - prob.lo
    row = 0
    for d in range(prob.ndim):
        for face, sign in ((prob.lo[d], +1.0), (prob.hi[d], -1.0)):
            for _ in range(n_per_face):
                inside[row, d] = face + sign * eps * width[d]
                outside[row, d] = face - sign * eps * width[d]
                row += 1
    # the face itself belongs to the outside of the open box: the first row of every face sits on it
    for d in range(prob.ndim):
        outside[2 * d * n_per_face, d] = prob.lo[d]
        outside[(2 * d + 1) * n_per_face, d] = prob.hi[d]
    return inside, outside


def t_limit(E, n_features):
    """Two-sided Student-t quantile (E - 1 degrees of freedom) at a family-wise error of 1e-3, Bonferroni over the
    features of one case."""
    from scipy.stats import t
    return float(t.ppf(1.0 - FAMILY_ERROR / (2.0 * n_features), E - 1))


def worst(T, names):
    """(max |T|, the feature that attains it)."""
    i = int(np.argmax(np.abs(T)))
    return float(abs(T[i])), names[i]
