"""The log marginal likelihood (evidence) of a fit by bridge sampling: what Bayes factors and posterior model
probabilities are made of -- how many Cole-Cole modes, which polynomial degree, Dias or Shin.  ``get_waic`` and ``get_loo``
are predictive criteria; this is the evidence itself (Meng & Wong 1996, "Simulating ratios of normalizing constants via a
simple identity"; the arrangement of Gronau et al. 2017, "A tutorial on bridge sampling"; the error estimate of
Fruehwirth-Schnatter 2004).

Per ensemble (spectrum), of ``n`` used samples of ``Wp`` walkers: the first ``n0 = n // 2`` fit the proposal, the last ``n1 = n -
n0`` enter the estimator, ``N1 = n1 * Wp`` rows numbered ``k * Wp + w``.

* Proposal: ``mu``, ``Sigma`` = ``covariance.flat_cov`` of the first half, ``L = cholesky(Sigma)``, ``c = sum_j log L_jj + (ndim /
  2) log(2 pi)``; ``log_g(x) = -0.5 sum_j z_j^2 - c`` with ``L z = x - mu`` by forward substitution.
* ``l1 = logp - log_g(theta)`` over the second half's rows; ``l2 = logp(theta~) - log_g(theta~)`` over ``N2`` draws of the
  proposal (default ``N2 = N1``), ``-inf`` for a draw outside the prior box.
* ``lstar = median(l1)``, ``s1 = neff / (neff + N2)``, ``s2 = 1 - s1``; ``a1 = exp(-(l2 - lstar))``, ``a2 = exp(l1 - lstar)``.
* From ``r = 1``: ``r' = mean_i(1 / (s1 + s2 r a1_i)) / mean_j(1 / (s1 a2_j + s2 r))`` until ``|r' - r| <= tol r'``; ``log_ml = log r
  + lstar``.  An ``a1`` or ``a2`` of ``+inf`` contributes exactly 0: no overflow at either end.
* ``re2 = var(f1) / mean(f1)^2 / N2 + tau var(f2) / mean(f2)^2 / N1`` with ``f1``, ``f2`` the terms at the final ``r`` and ``tau``
  the integrated autocorrelation time of ``f2`` over the second half's steps; ``se = sqrt(re2)``.
* ``log_evidence = log_ml - sum_j log(hi_j - lo_j)``: the uniform prior normalised.  The likelihood is the project's own (``-q / 2
  - log sigma^2`` per point); ``gaussian_offset`` turns it into the properly normalised Gaussian's and is the same for every
  model of one spectrum.

* ``halves``, ``proposal_factor``, ``log_g``, ``host_draws``, ``bridge_terms``, ``bridge_iterate``, ``relative_error2``,
  ``series_tau``, ``bridge_evidence``, ``gaussian_offset``, ``compare_evidence``: the definitions, plain NumPy in float64;
* ``ordered_logg`` and ``ordered_iterate`` restate bisip_bridge_logg_dev and bisip_bridge_iterate_dev (include/bisip_hip.h)
  operation by operation: the same bits; ``draw_yardstick`` carries the Philox words of bisip_bridge_draw_dev through
  ``np.longdouble``;
* ``device_evidence`` strings the four device steps together where the chain lies;
* ``ModelEvidence`` and ``BatchEvidence`` are the ``get_evidence`` methods of the models (bisip_amd.utils.utils) and of
  SpectraBatch.
"""

import numpy as np

__all__ = ('halves', 'proposal_factor', 'log_g', 'host_draws', 'bridge_terms', 'bridge_iterate', 'relative_error2', 'series_tau',
           'bridge_evidence',
           'gaussian_offset', 'compare_evidence', 'ordered_logg', 'ordered_iterate', 'draw_yardstick', 'device_evidence',
           'ModelEvidence', 'BatchEvidence')

TOL, MAXITER = 1e-10, 1000
DRAW_DOMAIN = 0x42520000            # counter word 3 of the draws' Philox stream (chain_bridge.hip: BR_DOMAIN)
PASS_BYTES = 2 << 30                # the draws' theta~ of one pass of device_evidence stay under this


# -- the definitions -----------------------------------------------------------------------------------------------------
def halves(n, Wp, ndim):
    """``(n0, n1)``: how many of ``n`` used samples fit the proposal and how many enter the estimator.  ValueError when the
    first half has fewer than ``ndim + 2`` rows or the second fewer than 2 samples."""
    n0 = int(n) // 2
    n1 = int(n) - n0
    if n0 * int(Wp) < int(ndim) + 2 or n1 < 2:
        raise ValueError(f'{n} used samples of {Wp} walkers are too few for the evidence of {ndim} parameters: the first half '
                         f'needs {ndim + 2} rows, the second 2 samples')
    return n0, n1


def proposal_factor(mean, cov, first_spectrum=0):
    """``(mu (E, ndim), L (E, ndim, ndim), c (E,))`` of the normal proposals of mean ``(E, ndim)`` and covariance ``(E, ndim,
    ndim)``: ``L = np.linalg.cholesky``, ``c = sum_j log L_jj + (ndim / 2) log(2 pi)``.  ValueError names the spectrum whose
    covariance is not positive definite."""
    mu = np.atleast_2d(np.asarray(mean, dtype=np.float64))
    cov = np.asarray(cov, dtype=np.float64)
    cov = cov[None] if cov.ndim == 2 else cov
    E, ndim = mu.shape
    if cov.shape != (E, ndim, ndim):
        raise ValueError(f'a covariance of shape {cov.shape} for means of shape {mu.shape}')
    L = np.empty_like(cov)
    for e in range(E):
        try:
            if not np.isfinite(cov[e]).all():
                raise np.linalg.LinAlgError('not finite')
            L[e] = np.linalg.cholesky(cov[e])
        except np.linalg.LinAlgError:
            raise ValueError(f'spectrum {first_spectrum + e}: the covariance of the proposal is not positive definite (a '
                             'parameter that does not move, or too few samples)') from None
    c = np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1) + 0.5 * ndim * np.log(2 * np.pi)
    return mu, L, c


def log_g(x, mu, L, c):
    """The log density of the normal proposal ``(mu (ndim,), L (ndim, ndim), c)`` at the rows ``x (..., ndim)``: ``z_j = ((x_j -
    mu_j) - sum_{k<j} L_jk z_k) / L_jj``, ``-0.5 sum_j z_j^2 - c``."""
    x = np.asarray(x, dtype=np.float64)
    ndim = x.shape[-1]
    with np.errstate(all='ignore'):
        d = x - mu
        z = np.empty_like(d)
        for j in range(ndim):
            z[..., j] = (d[..., j] - (L[j, :j] * z[..., :j]).sum(axis=-1)) / L[j, j]
        return -0.5 * (z * z).sum(axis=-1) - c


def _philox_words(n_draws, ndim, seed, first_draw, ensemble):
    """The four words of every (draw, pair): uint64 arrays ``(n_draws, ceil(ndim / 2))``."""
    from .sampler import philox4x32_10
    seed = int(seed) & 0xffffffffffffffff
    di = np.uint64(int(first_draw)) + np.arange(int(n_draws), dtype=np.uint64)
    pairs = np.arange((int(ndim) + 1) // 2, dtype=np.uint64)
    lo, hi = (di & np.uint64(0xffffffff))[:, None], (di >> np.uint64(32))[:, None]
    return philox4x32_10(lo, hi, np.uint64(int(ensemble)), np.uint64(DRAW_DOMAIN) | pairs[None, :], seed & 0xffffffff, seed >> 32)


def _u53(a, b):
    return ((a >> np.uint64(5)) << np.uint64(26) | (b >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)


def _sincospi(x, pi):
    """``(sin(pi x), cos(pi x))`` of ``x`` in [0, 2) in the precision of ``x``: the argument is brought to ``[-1/4, 1/4]``
    exactly first."""
    q = np.rint(2 * x)
    y = x - q / 2
    s, c = np.sin(pi * y), np.cos(pi * y)
    q = q.astype(np.int64) % 4
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def _normals(n_draws, ndim, seed, first_draw, ensemble, dtype):
    v0, v1, v2, v3 = _philox_words(n_draws, ndim, seed, first_draw, ensemble)
    u0, u1 = _u53(v0, v1).astype(dtype), _u53(v2, v3).astype(dtype)
    pi = 4 * np.arctan(dtype(1))
    rad = np.sqrt(-2 * np.log(1 - u0))
    s, c = _sincospi(2 * u1, pi)
    z = np.empty((int(n_draws), 2 * v0.shape[1]), dtype=dtype)
    z[:, 0::2], z[:, 1::2] = rad * c, rad * s
    return z[:, :int(ndim)]


def _draws(mu, L, c, n_draws, seed, first_draw, ensemble, dtype):
    mu, L = np.asarray(mu, dtype=dtype), np.asarray(L, dtype=dtype)
    z = _normals(n_draws, mu.size, seed, first_draw, ensemble, dtype)
    theta = mu + z @ np.tril(L).T
    return theta, -(z * z).sum(axis=1) / 2 - dtype(c), z


def host_draws(mu, L, c, n_draws, seed=0, first_draw=0, ensemble=0):
    """``(theta (n_draws, ndim), log_g (n_draws,))``: draws ``first_draw ...`` of the proposal of one ensemble in float64 NumPy,
    from the Philox words bisip_bridge_draw_dev takes: draw ``i``, pair ``p`` from ``philox4x32_10(lo32(i), hi32(i), ensemble,
    0x42520000 | p, lo32(seed), hi32(seed))``, ``u0 = u53(v0, v1)``, ``u1 = u53(v2, v3)``, ``rad = sqrt(-2 log(1 - u0))``, ``(z_2p,
    z_2p+1) = rad (cospi(2 u1), sinpi(2 u1))``, ``theta = mu + L z``."""
    theta, lg, _ = _draws(mu, L, c, n_draws, seed, first_draw, ensemble, np.float64)
    return theta, lg


def draw_yardstick(mu, L, c, n_draws, seed=0, first_draw=0, ensemble=0):
    """``(theta, log_g, z)`` of ``host_draws`` carried through ``np.longdouble`` from the same (exact) Philox words: what the
    device's draws and the float64 definition are measured against."""
    return _draws(mu, L, c, n_draws, seed, first_draw, ensemble, np.longdouble)


def bridge_terms(l1, l2):
    """``(lstar, a1, a2)`` of ``l1 (..., N1)`` and ``l2 (..., N2)``: ``lstar = median(l1)``, ``a1 = exp(-(l2 - lstar))`` (``+inf``
    for a draw outside the box), ``a2 = exp(l1 - lstar)``."""
    l1, l2 = np.asarray(l1, dtype=np.float64), np.asarray(l2, dtype=np.float64)
    with np.errstate(all='ignore'):
        lstar = np.median(l1, axis=-1)
        return lstar, np.exp(-(l2 - lstar[..., None])), np.exp(l1 - lstar[..., None])


def _result(r, it, m1, v1, m2, v2, f2, history):
    with np.errstate(all='ignore'):
        return dict(r=r, log_r=float(np.log(r)), iterations=it, moments=np.array([m1, v1, m2, v2]), f2=f2, history=history)


def bridge_iterate(a1, a2, s1, tol=TOL, maxiter=MAXITER):
    """The iteration of ONE ensemble from ``r = 1``: ``r' = mean(1 / (s1 + s2 r a1)) / mean(1 / (s1 a2 + s2 r))`` until ``|r' - r|
    <= tol r'`` or ``maxiter`` passes.  A dict of ``r``, ``log_r``, ``iterations``, ``moments`` (mean and population variance of
    ``f1``, then of ``f2``, at the final ``r``), ``f2 (N1,)`` and the ``history`` of ``r``.  A pass whose ``r'`` is not a positive
    finite number ends with ``r = NaN``."""
    a1, a2 = np.asarray(a1, dtype=np.float64).ravel(), np.asarray(a2, dtype=np.float64).ravel()
    s1 = float(s1)
    s2 = 1.0 - s1
    if maxiter < 1 or not tol >= 0:
        raise ValueError('tol must be >= 0 and maxiter >= 1')
    r, it, history = 1.0, 0, []
    with np.errstate(all='ignore'):
        while True:
            rn = np.mean(1.0 / (s1 + s2 * r * a1)) / np.mean(1.0 / (s1 * a2 + s2 * r))
            it += 1
            if not (rn > 0.0 and rn < np.inf):
                r = np.nan
                break
            done = abs(rn - r) <= tol * rn
            r = float(rn)
            history.append(r)
            if done or it >= maxiter:
                break
        f1, f2 = 1.0 / (s1 + s2 * r * a1), 1.0 / (s1 * a2 + s2 * r)
        return _result(r, it, f1.mean(), f1.var(), f2.mean(), f2.var(), f2, history)


def relative_error2(moments, N1, N2, tau=1.0):
    """``var(f1) / mean(f1)^2 / N2 + tau var(f2) / mean(f2)^2 / N1`` of ``moments (..., 4)``: the squared relative error of ``r``,
    the squared standard error of ``log_ml``."""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(all='ignore'):
        return m[..., 1] / m[..., 0] ** 2 / N2 + tau * m[..., 3] / m[..., 2] ** 2 / N1


def series_tau(f2, n1, Wp):
    """The integrated autocorrelation time of the series ``f2 (n1 * Wp,)`` over its ``n1`` steps, the walkers averaged (emcee's
    estimator, bisip_amd.autocorr); 1.0 for a series that does not vary."""
    from .autocorr import integrated_time
    with np.errstate(all='ignore'):
        tau = float(integrated_time(np.asarray(f2, dtype=np.float64).reshape(n1, Wp, 1), tol=0, quiet=True)[0])
    return tau if np.isfinite(tau) else 1.0


def _warn_if_capped(iterations, maxiter, first_spectrum=0):
    capped = np.flatnonzero(np.atleast_1d(iterations) >= maxiter)
    if capped.size:
        import warnings
        warnings.warn(f'the bridge-sampling iteration of spectrum {first_spectrum + int(capped[0])}'
                      + (f' and {capped.size - 1} more' if capped.size > 1 else '') + f' stopped at maxiter={maxiter} '
                      'before it converged: the proposal covers the posterior badly (burn-in not discarded?)', RuntimeWarning)


def gaussian_offset(zn_err):
    """``sum_points(0.5 log sigma^2 - 0.5 log(2 pi))`` over the trailing two axes ``(2, N)``: added to ``log_evidence`` it gives
    the evidence under the properly normalised Gaussian likelihood.  Data only: equal for all models of one spectrum."""
    s = np.asarray(zn_err, dtype=np.float64)
    return (0.5 * np.log(s ** 2) - 0.5 * np.log(2 * np.pi)).sum(axis=(-2, -1))


def _log_volume(bounds, ndim):
    if bounds is None:
        return 0.0
    b = np.asarray(bounds, dtype=np.float64).reshape(2, ndim)
    return float(np.log(b[1] - b[0]).sum())


def _chain_arrays(chain, logp):
    x = np.asarray(chain, dtype=np.float64)
    lp = np.asarray(logp, dtype=np.float64)
    if x.ndim == 2:
        x, lp = x[:, None, :], lp.reshape(-1, 1)
    if x.ndim != 3 or lp.shape != x.shape[:2]:
        raise ValueError(f'expected a chain (n, nwalkers, ndim) with its log-probability (n, nwalkers), got {x.shape} and '
                         f'{lp.shape}')
    return x, lp


def bridge_evidence(chain, logp, log_prob_fn, bounds=None, n_draws=None, seed=0, neff='ess', proposal=None, use_all=None,
                    draws=None, tau=None, tol=TOL, maxiter=MAXITER, offset=np.nan, ensemble=0, order=None):
    """The evidence of ONE ensemble in NumPy: ``chain (n, Wp, ndim)`` (or flat ``(N, ndim)``: one walker) with its stored
    log-probability ``logp`` and ``log_prob_fn(theta (m, ndim)) -> (m,)``.  ``bounds (2, ndim)``: the prior box (None: ``log_evidence
    = log_ml``).  ``neff``: ``'ess'`` (the median over the parameters of ``ess.ess(second half, 'mean')``, at most ``N1``), None
    (``N1``) or a number.  ``proposal=(mean, cov)`` replaces the fit; all used samples then enter the estimator unless
    ``use_all=False``.  ``draws=(theta, log_g)``: the proposal's draws, instead of ``host_draws(seed)``.  ``tau``: a number
    replaces the estimate of ``series_tau``.  ``order=(n_modes, by)``: a Cole-Cole chain whose modes share one box
    (bisip_amd.modes): the samples are taken with their modes in order (their stored log-probability unchanged), a draw whose
    modes are not in order gets ``logp = -inf`` (and counts in ``frac_outside``), ``log_symmetry = log(n_modes!)`` is added to
    ``log_ml`` and ``log_evidence`` and returned beside them -- the estimate over one labelling, where a normal proposal fits.
    Returns the dict of ``get_evidence``."""
    x, lp = _chain_arrays(chain, logp)
    if order is not None:
        from .modes import log_symmetry, modes_moved, order_modes
        x = order_modes(x, *order)
    n, Wp, ndim = x.shape
    if proposal is None:
        n0, n1 = halves(n, Wp, ndim)
        from .covariance import flat_cov
        mean, cov = flat_cov(x[:n0])
    else:
        mean, cov = proposal
        if use_all is None or use_all:
            n0, n1 = 0, n
            if n1 < 2:
                raise ValueError(f'{n} used sample(s): the evidence needs 2')
        else:
            n0, n1 = halves(n, Wp, ndim)
    mu, L, c = proposal_factor(mean, cov, ensemble)
    mu, L, c = mu[0], L[0], float(c[0])
    x1, lp1 = x[n0:], lp[n0:]
    N1 = n1 * Wp
    l1 = (lp1 - log_g(x1, mu, L, c)).reshape(N1)
    if draws is None:
        N2 = N1 if n_draws is None else int(n_draws)
        theta2, lg2 = host_draws(mu, L, c, N2, seed, 0, ensemble)
    else:
        theta2, lg2 = (np.asarray(a, dtype=np.float64) for a in draws)
        N2 = theta2.shape[0]
    lp2 = np.asarray(log_prob_fn(theta2), dtype=np.float64).reshape(N2)
    if order is not None:
        lp2 = np.where(modes_moved(theta2, *order), -np.inf, lp2)
    with np.errstate(all='ignore'):
        l2 = lp2 - lg2
    if neff is None:
        ne = float(N1)
    elif isinstance(neff, str):
        if neff != 'ess':
            raise ValueError(f"neff={neff!r}: 'ess', None or a number")
        from .ess import ess
        with np.errstate(all='ignore'):
            ne = float(min(np.median(ess(x1, 'mean')), N1)) if n1 >= 4 else float(N1)
        ne = ne if np.isfinite(ne) and ne > 0 else float(N1)
    else:
        ne = float(neff)
    lstar, a1, a2 = bridge_terms(l1, l2)
    it = bridge_iterate(a1, a2, ne / (ne + N2), tol, maxiter)
    if maxiter > 2:
        _warn_if_capped(it['iterations'], maxiter, ensemble)
    t = series_tau(it['f2'], n1, Wp) if tau is None else float(tau)
    with np.errstate(all='ignore'):
        log_ml = it['log_r'] + float(lstar)
        se = float(np.sqrt(relative_error2(it['moments'], N1, N2, t)))
    sym = {}
    if order is not None:
        sym = dict(log_symmetry=log_symmetry(order[0]))
        log_ml = log_ml + sym['log_symmetry']
    return dict(log_evidence=log_ml - _log_volume(bounds, ndim), log_ml=log_ml, se=se, iterations=it['iterations'], n1=N1,
                n2=N2, neff=ne, tau_f2=t, frac_outside=float(np.mean(np.isneginf(lp2))), gaussian_offset=float(offset),
                proposal_mean=mu, proposal_cov=np.asarray(cov, dtype=np.float64).reshape(ndim, ndim), **sym)


def compare_evidence(results):
    """Models fitted to the SAME spectrum, ranked: ``results`` maps a name to a ``get_evidence`` / ``bridge_evidence`` result;
    returns a list of dicts ``name, log_evidence, log_bf, prob, se``, the largest ``log_evidence`` first.  ``log_bf`` is the log
    Bayes factor against the best model (<= 0) and ``prob`` the posterior model probability under equal prior odds."""
    if not results:
        raise ValueError('nothing to compare')
    for name, r in results.items():
        if np.ndim(r['log_evidence']) != 0:
            raise ValueError(f'{name!r}: one spectrum at a time')
    order = sorted(results, key=lambda name: -float(results[name]['log_evidence']))
    best = float(results[order[0]]['log_evidence'])
    with np.errstate(all='ignore'):
        bf = np.array([float(results[name]['log_evidence']) - best for name in order])
        w = np.exp(bf)
        prob = w / w.sum()
    return [dict(name=name, log_evidence=float(results[name]['log_evidence']), log_bf=float(b), prob=float(p),
                 se=float(results[name]['se'])) for name, b, p in zip(order, bf, prob)]


# -- the device's order of operations ------------------------------------------------------------------------------------
def ordered_logg(x, logp, mu, L, c):
    """``l = logp - log_g(x)`` of the rows ``x (R, ndim)`` with the bits of bisip_bridge_logg_dev: ``d_j = x_j - mu_j``; ``acc =
    fma(-L_jk, z_k, acc)`` in ascending ``k`` from ``d_j``, one division; ``m = fma(z_j, z_j, m)`` in ascending ``j`` from 0.0;
    ``log_g = fma(-0.5, m, -c)``.  Every fma is taken exactly in Python (``chainview.exact_fma``): for the shapes of the tests."""
    from .chainview import exact_fma
    fma = np.frompyfunc(exact_fma, 3, 1)
    x = np.asarray(x, dtype=np.float64)
    R, ndim = x.shape
    with np.errstate(all='ignore'):
        z = np.empty((R, ndim))
        m = np.zeros(R)
        for j in range(ndim):
            acc = x[:, j] - mu[j]
            for k in range(j):
                acc = fma(-L[j, k], z[:, k], acc).astype(np.float64)
            z[:, j] = acc / L[j, j]
            m = fma(z[:, j], z[:, j], m).astype(np.float64)
        lg = fma(-0.5, m, -float(c)).astype(np.float64)
        return np.asarray(logp, dtype=np.float64) - lg


def ordered_iterate(a1, a2, s1, tol=TOL, maxiter=MAXITER):
    """``bridge_iterate`` of one ensemble with the bits of bisip_bridge_iterate_dev: ``f1_i = 1 / (s1 + (s2 r) a1_i)``, ``f2_j = 1 /
    fma(s1, a2_j, s2 r)``; term ``i`` of a sum to slot ``i mod 256``, a slot in ascending order from 0.0, the slots pairwise
    within runs of 64, the four runs in ascending order (``loo._block_sum``); a mean is ``sum / float(count)``; the variances
    a second pass of ``fma(d, d, acc)`` per slot.  The same dict as ``bridge_iterate``."""
    from .chainview import exact_fma
    from .loo import SLOTS, _block_sum, _wave_tree
    fma = np.frompyfunc(exact_fma, 3, 1)
    a1, a2 = np.asarray(a1, dtype=np.float64).ravel(), np.asarray(a2, dtype=np.float64).ravel()
    N2, N1 = a1.size, a2.size
    s1 = float(s1)
    s2 = 1.0 - s1
    if maxiter < 1 or not tol >= 0:
        raise ValueError('tol must be >= 0 and maxiter >= 1')

    def terms(r):
        s2r = s2 * r
        return 1.0 / (s1 + s2r * a1), 1.0 / fma(s1, a2, s2r).astype(np.float64)

    def squares(f, mean):
        d = f - mean
        rows = -(-d.size // SLOTS)
        pad = np.zeros(rows * SLOTS)
        pad[:d.size] = d
        live = np.zeros(rows * SLOTS, bool)
        live[:d.size] = True
        pad, live = pad.reshape(rows, SLOTS), live.reshape(rows, SLOTS)
        acc = np.zeros(SLOTS)
        for k in range(rows):
            acc = np.where(live[k], fma(pad[k], pad[k], acc).astype(np.float64), acc)
        w = _wave_tree(acc)
        return ((w[0] + w[1]) + w[2]) + w[3]

    r, it, history = 1.0, 0, []
    with np.errstate(all='ignore'):
        while True:
            f1, f2 = terms(r)
            rn = (_block_sum(f1) / float(N2)) / (_block_sum(f2) / float(N1))
            it += 1
            if not (rn > 0.0 and rn < np.inf):
                r = np.nan
                break
            done = abs(rn - r) <= tol * rn
            r = float(rn)
            history.append(r)
            if done or it >= maxiter:
                break
        f1, f2 = terms(r)
        m1, m2 = _block_sum(f1) / float(N2), _block_sum(f2) / float(N1)
        v1, v2 = squares(f1, m1) / float(N2), squares(f2, m2) / float(N1)
        return _result(r, it, m1, v1, m2, v2, f2, history)


# -- on the device -------------------------------------------------------------------------------------------------------
def _tail_view(view, first, n):
    """Samples ``first ... first + n - 1`` of a ChainView."""
    from .chainview import ChainView
    return ChainView(view.tensor, n, view.n_ensembles, view.walkers_per_ensemble, view.ndim,
                     view.offset + first * view.stride, view.stride, view.backend)


def device_evidence(view, logp_view, ctx, n_draws=None, seed=0, neff='ess', proposal=None, use_all=None, first_ensemble=0,
                    tol=TOL, maxiter=MAXITER, keep_draws=False, order=None):
    """The bridge-sampling estimate of every ensemble of a ChainView with the stored log-probability of ``logp_view`` (a
    ChainView of ``ndim = 1`` over the same samples) and the model of ``ctx`` (a HipContext of ``view.n_ensembles`` spectra), where
    the chain lies: bisip_chain_cov_dev of the first half, the Cholesky factor on the host, bisip_bridge_logg_dev (``l1``),
    bisip_bridge_draw_dev and bisip_logprob_dev (``l2``), the median of ``l1`` by bisip_columns_percentiles_dev,
    bisip_bridge_scale_dev, bisip_bridge_iterate_dev, and ``tau`` of ``f2`` by bisip_chain_autocorr_time_dev.  The draws go in
    passes of whole ensembles' ranges of draws whose ``theta~`` stay under ``PASS_BYTES``; ``l1``, ``l2``, ``a1`` and ``a2`` stay on
    the device.  Ensemble ``e`` draws from the Philox stream of ``first_ensemble + e``.  ``bisip_logprob_dev`` runs the formulation
    the context holds after the sampler's guard.  Returns a dict of ``(E,)`` arrays ``log_ml``, ``se``, ``iterations``, ``neff``,
    ``tau_f2``, ``frac_outside``, the ints ``n1`` and ``n2`` and ``proposal_mean (E, ndim)``, ``proposal_cov (E, ndim, ndim)``; with
    ``keep_draws`` also ``theta2 (E, N2, ndim)``, ``logg2`` and ``logp2 (E, N2)`` (NumPy).  ``order=(n_modes, by)`` as
    ``bridge_evidence``: the samples are the ordered derived view (one bisip_mode_order_dev), every pass of draws takes one
    more bisip_mode_order_dev that asks for ``moved`` alone and a ``masked_fill_`` of ``logp2`` (kept as filled); the dict gains
    ``log_symmetry``."""
    import torch
    from . import _hip
    from .autocorr import device_integrated_time
    from .covariance import device_cov
    n, E, Wp, ndim = view.n, view.n_ensembles, view.walkers_per_ensemble, view.ndim
    if ndim != ctx.ndim or E != ctx.n_spectra:
        raise ValueError(f'a chain of {E} ensembles of {ndim} parameters for a context of {ctx.n_spectra} spectra of {ctx.ndim}')
    if order is not None:
        from .modes import device_mode_order, key_group, log_symmetry
        view = view.derived(device_mode_order(view, order[0], order[1], ordered=True, desc=False)[0])
    if (logp_view.n, logp_view.n_ensembles, logp_view.walkers_per_ensemble, logp_view.ndim) != (n, E, Wp, 1):
        raise ValueError('the log-probability does not belong to the samples of the chain')
    if proposal is None:
        n0, n1 = halves(n, Wp, ndim)
        mean, cov = device_cov(_tail_view(view, 0, n0), mean=True)
    else:
        mean, cov = (np.asarray(a, dtype=np.float64) for a in proposal)
        mean, cov = np.broadcast_to(mean, (E, ndim)), np.broadcast_to(cov, (E, ndim, ndim))
        n0, n1 = (0, n) if use_all is None or use_all else halves(n, Wp, ndim)
        if n1 < 2:
            raise ValueError(f'{n} used sample(s): the evidence needs 2')
    mu, L, c = proposal_factor(mean, cov, first_ensemble)
    v1, lv1 = _tail_view(view, n0, n1), _tail_view(logp_view, n0, n1)
    N1 = n1 * Wp
    N2 = N1 if n_draws is None else int(n_draws)
    if N2 < 1:
        raise ValueError('n_draws must be positive')
    if neff is None:
        ne = np.full(E, float(N1))
    elif isinstance(neff, str):
        if neff != 'ess':
            raise ValueError(f"neff={neff!r}: 'ess', None or a number")
        from .ess import device_ess
        with np.errstate(all='ignore'):
            ne = np.minimum(np.median(device_ess(v1, 'mean'), axis=1), N1) if n1 >= 4 else np.full(E, float(N1))
            ne = np.where(np.isfinite(ne) & (ne > 0), ne, float(N1))
    else:
        ne = np.broadcast_to(np.asarray(neff, dtype=np.float64), (E,)).copy()
    st = view.stream
    d_mu, d_L, d_c = view.upload(mu), view.upload(L), view.upload(c)
    l1 = view.empty((E, N1), torch.float64)
    _hip.bridge_logg_dev(v1.ptr, n1, v1.stride, E, Wp, ndim, lv1.ptr, lv1.stride, d_mu.data_ptr(), d_L.data_ptr(),
                         d_c.data_ptr(), l1.data_ptr(), st)
    # the draws, theta~ of a pass under PASS_BYTES: draws [d0, d0 + k) of every ensemble
    chunk = int(min(N2, max(1, PASS_BYTES // (E * ndim * 8))))
    logp2, logg2 = view.empty((E, N2), torch.float64), view.empty((E, N2), torch.float64)
    theta_host = np.empty((E, N2, ndim)) if keep_draws else None
    for d0 in range(0, N2, chunk):
        k = min(N2, d0 + chunk) - d0
        theta = view.empty((E * k, ndim), torch.float64)
        whole = k == N2
        lg, lp = (logg2, logp2) if whole else (view.empty((E, k), torch.float64), view.empty((E, k), torch.float64))
        _hip.bridge_draw_dev(d_mu.data_ptr(), d_L.data_ptr(), d_c.data_ptr(), E, ndim, k, seed, d0, first_ensemble,
                             theta.data_ptr(), lg.data_ptr(), st)
        ctx.logprob_dev(theta.data_ptr(), E * k, lp.data_ptr(), st)
        if order is not None:                                    # the draws as one sample of E ensembles of k rows
            moved = view.empty((E, k), torch.uint8)
            _hip.mode_order_dev(theta.data_ptr(), 1, E * k * ndim, E, k, order[0], key_group(order[1]), 0, 0, moved.data_ptr(), st)
            lp.masked_fill_(moved.bool(), float('-inf'))
        if not whole:                                           # (same stream: ordered after the kernels)
            logg2[:, d0:d0 + k].copy_(lg)
            logp2[:, d0:d0 + k].copy_(lp)
        view.synchronize()
        if keep_draws:
            theta_host[:, d0:d0 + k] = theta.cpu().numpy().reshape(E, k, ndim)
        del theta, lg, lp
    outside = torch.isneginf(logp2).sum(dim=1)
    kept = dict(theta2=theta_host, logg2=logg2.cpu().numpy(), logp2=logp2.cpu().numpy()) if keep_draws else {}
    lstar = view.empty((1, E), torch.float64)
    _hip.columns_percentiles_dev(l1.data_ptr(), E, N1, (50.0,), lstar.data_ptr(), st)
    a1, a2 = view.empty((E, N2), torch.float64), view.empty((E, N1), torch.float64)
    _hip.bridge_scale_dev(l1.data_ptr(), N1, logp2.data_ptr(), logg2.data_ptr(), N2, E, lstar.data_ptr(), 0, a1.data_ptr(),
                          a2.data_ptr(), st)
    d_s1 = view.upload(ne / (ne + N2))
    r, its = view.empty((E,), torch.float64), view.empty((E,), torch.int64)
    mom, f2 = view.empty((E, 4), torch.float64), view.empty((E, N1), torch.float64)
    _hip.bridge_iterate_dev(a1.data_ptr(), N2, a2.data_ptr(), N1, E, d_s1.data_ptr(), tol, maxiter, r.data_ptr(),
                            its.data_ptr(), mom.data_ptr(), f2.data_ptr(), st)
    view.synchronize()
    if maxiter > 2:
        _warn_if_capped(its.cpu().numpy(), maxiter, first_ensemble)
    # tau of f2 over the second half's steps: f2 (E, n1, Wp) as a chain (n1, E * Wp, 1) -- one copy, sample-major
    from .chainview import ChainView
    series = f2.view(E, n1, Wp).permute(1, 0, 2).contiguous()
    tau = device_integrated_time(ChainView(series, n1, E, Wp, 1, backend=view.backend), 5)[0][:, 0]
    tau = np.where(np.isfinite(tau), tau, 1.0)
    with np.errstate(all='ignore'):
        log_ml = np.log(r.cpu().numpy()) + lstar.cpu().numpy()[0]
        se = np.sqrt(relative_error2(mom.cpu().numpy(), N1, N2, tau))
    if order is not None:
        kept = dict(kept, log_symmetry=log_symmetry(order[0]))
        log_ml = log_ml + kept['log_symmetry']
    return dict(log_ml=log_ml, se=se, iterations=its.cpu().numpy(), n1=N1, n2=N2, neff=ne, tau_f2=tau,
                frac_outside=outside.cpu().numpy() / float(N2), proposal_mean=np.array(mean), proposal_cov=np.array(cov), **kept)


def _finish(res, bounds, ndim, offset, single):
    """The dict of get_evidence from device_evidence's: ``log_evidence`` and ``gaussian_offset`` added, scalars for one model."""
    out = dict(res)
    out['log_evidence'] = res['log_ml'] - _log_volume(bounds, ndim)
    out['gaussian_offset'] = np.asarray(offset, dtype=np.float64)
    if single:
        for k in ('log_evidence', 'log_ml', 'se', 'neff', 'tau_f2', 'frac_outside', 'gaussian_offset'):
            out[k] = float(np.ravel(out[k])[0])
        out['iterations'] = int(out['iterations'][0])
        out['proposal_mean'], out['proposal_cov'] = out['proposal_mean'][0], out['proposal_cov'][0]
    order = ('log_evidence', 'log_ml', 'se', 'iterations', 'n1', 'n2', 'neff', 'tau_f2', 'frac_outside', 'gaussian_offset',
             'proposal_mean', 'proposal_cov')
    return {k: out[k] for k in order + tuple(k for k in out if k not in order)}


# -- the methods of the models and of SpectraBatch -----------------------------------------------------------------------
class ModelEvidence:
    """Mixin of bisip_amd.utils.utils: the ``chain=`` / ``discard`` / ``thin`` rules are parse_chain's."""

    def _evidence_order(self, order_modes):
        """``(n_modes, by)`` of ``order_modes=by`` for a model with exchangeable Cole-Cole modes; None for None."""
        if order_modes is None:
            return None
        if not hasattr(self, 'n_modes') or getattr(self, 'model', 'PeltonColeCole') != 'PeltonColeCole':
            raise ValueError('order_modes belongs to PeltonColeCole: no other model has modes to order')
        from .modes import _order_argument
        return _order_argument(order_modes, self.n_modes, self.param_bounds, self.param_names)

    def get_evidence(self, chain=None, log_prob=None, n_draws=None, seed=0, neff='ess', proposal=None, order_modes=None,
                     **kwargs):
        """The log marginal likelihood of the fit by bridge sampling (bisip_amd.evidence): a dict of ``log_evidence`` (the
        uniform prior normalised), ``log_ml``, its standard error ``se``, ``iterations``, ``n1``, ``n2``, ``neff``, ``tau_f2``,
        ``frac_outside`` (the share of the proposal's draws outside the prior box), ``gaussian_offset``, ``proposal_mean
        (ndim,)`` and ``proposal_cov (ndim, ndim)``.  The first half of the used samples fits a normal proposal, the second
        half and ``n_draws`` draws of it (default: as many) enter the estimator; ``compare_evidence`` turns the results of
        several models of one spectrum into Bayes factors and posterior model probabilities.  ``neff``: ``'ess'`` (the median
        'mean' ESS of the second half), None (its size) or a number.  ``proposal=(mean, cov)`` replaces the fit: all used
        samples then enter the estimator.  ``discard`` / ``thin`` as for ``get_chain``.  A fit with the device sampler is taken
        on the GPU (``chain='device'``: where the chain lies); a host sampler's, or an explicit unflattened ``chain (n,
        nwalkers, ndim)`` with its ``log_prob (n, nwalkers)``, in NumPy with ``self.log_prob``.  ``order_modes``:
        ``'log_tau'``, ``'m'`` or ``'c'`` for a PeltonColeCole model whose modes share one prior box: the estimate is taken
        over one labelling of the modes (bisip_amd.modes: the samples in order, the draws that are not refused) and
        ``log_symmetry = log(n_modes!)`` added -- a posterior that mixes the labellings is not bridged by one normal."""
        from .utils import discard_thin, refuse_discard_of_a_chain
        offset = gaussian_offset(self._data['zn_err'])
        bounds = self.param_bounds
        order = {} if order_modes is None else dict(order=self._evidence_order(order_modes))
        s = self._device_chain_sampler(chain, kwargs)
        if s is not None and s.n_ensembles == 1:
            dt = discard_thin(kwargs)
            res = device_evidence(s.used_samples_dev(**dt), s.log_prob_samples_dev(**dt), s.backend.ctx, n_draws, seed, neff,
                                  proposal, **order)
            return _finish(res, bounds, s.ndim, offset, True)
        if chain is None:
            self._check_if_fitted()
            dt = discard_thin(kwargs)
            chain, log_prob = self.get_chain(**dt), self._sampler.get_log_prob(**dt)
        else:
            refuse_discard_of_a_chain(kwargs)
            if log_prob is None:
                raise ValueError('an explicit chain needs its log-probability: pass log_prob (n, nwalkers)')
        return bridge_evidence(chain, log_prob, self.log_prob, bounds, n_draws, seed, neff, proposal, offset=float(offset),
                               **order)


class BatchEvidence:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler, ``ctx`` its context)."""

    _evidence_order = ModelEvidence._evidence_order

    def get_evidence(self, discard=0, thin=1, n_draws=None, seed=0, neff='ess', proposal=None, order_modes=None):
        """The log marginal likelihood of every spectrum's fit by bridge sampling (bisip_amd.evidence): a dict of
        ``log_evidence``, ``log_ml``, ``se``, ``iterations``, ``neff``, ``tau_f2``, ``frac_outside``, ``gaussian_offset``, ``(E,)`` each,
        ``n1``, ``n2``, ``proposal_mean (E, ndim)`` and ``proposal_cov (E, ndim, ndim)``, taken on the device for ``chain='device'``
        and ``'host'`` alike.  Spectrum ``e`` draws from the Philox stream of its survey index.  Under torch.distributed every
        rank returns its own spectra.  ``order_modes`` as the models' ``get_evidence``: PeltonColeCole, the modes in one box."""
        s = self._fitted()
        order = {} if order_modes is None else dict(order=self._evidence_order(order_modes))
        res = s.evidence(discard=discard, thin=thin, n_draws=n_draws, seed=seed, neff=neff, proposal=proposal,
                         first_ensemble=self.spectrum_range[0], **order)
        return _finish(res, self.param_bounds, self.ndim, gaussian_offset(self.zn_err), False)
