"""What tests/test_model_bounds.py and tests/test_gpu_model_exact.py share: the probe spectrum that makes a log-probability
give back ONE residual bit for bit, the exact value of the reference's Cole-Cole / Dias / Shin formulas at the double inputs
(theta, w), and a first-order rounding bound of bisip_amd/csrc/kernels.h per (row, frequency, part).

THE PROBE.  logprob_row returns fma(-0.5, acc0 + acc1, lconst), acc0 = sum_j rr_j^2 (1 / sigma_re,j^2) in ascending j (acc1:
the imaginary parts).  With measured values 0, sigma = 2^-E at one (part, j) and 2^10 everywhere else, rr_j^2 2^(2E) is the
correctly rounded square scaled exactly; every other term (<= |Z|^2 2^-20 each) and lconst = -sum ln sigma^2 lie below half
an ulp of it as soon as |rr_j| exceeds ~2^(-E+32), the sums return it unchanged, and sqrt(-2 logp) 2^-E -- the square root of a
correctly rounded square returns its operand -- IS |rr_j| = |Re Z_j| as the residual path computes it (or |Im Z_j|).
`recover` checks that dominance with the numbers at hand; where a part is too small for it (sin(c pi/2) at c = 5e-324) it
returns, instead of 0, the uncertainty du that the other terms and the roundings of the sums leave on the recovered value,
and `assert_recovery_is_sharp` holds du to 1/64 of the bound for every asserted entry (to 2^-90 of the unit where the bound
itself is at the subnormal scale).  E = 100 (2^-40 does not dominate).

THE EXACT VALUE is that of the reference's formula (cython_funcs.pyx: C_ColeCole, C_Dias, C_Shin) at the doubles theta and
w: no rounded ln w, sqrt w, 1 - m.  `exact()` evaluates it in vectorised np.longdouble (u_L = 2^-64), arranged so that
nothing cancels (1/delta - 1 = (1 - delta)/delta, cos(c pi/2) = sin((1 - c) pi/2) beyond c = 1/2, 1 - sum m taken first: all
exact or one rounding in long double); its own error estimate `ref_err` (a count of its roundings, conditioning of the
exponent included) is held to 1/64 of the bound by `assert_reference_is_sharp` and to a 50-digit mpmath evaluation of the
LITERAL formula (`exact_mp`) by the host test.

THE BOUND.  u = 2^-53; "k ulp" of a stated figure is taken as the relative error 2 k u (an ulp of a mantissa next to 1).
Stated figures (kernels.h): exp2_finite 0.89 ulp, exp_finite 0.83, rcp_nr 1.00, rcp_joint<2> / <4> 2.4 / 3.7,
sincos_unit 1.5; sincospi (safe loop, forward()): 4 ulp, the OpenCL full-profile figure the device library is built to.
rcp_batch_n<K> states none: every result carries 2K - 2 roundings of products and rcp_nr's ulp (counted from its code).
T_i is a term (Cole-Cole: A_i / (1 + x_i), x_i = e_i omega_i, e_i = 2^y, omega = cos + i sin of c pi/2; Shin: 1 / y_i,
y_i = p_i omega_i + 1/R_i; Dias: A / den), |T_i| its modulus, T_i,p its real or imaginary part.

 Exponentials (Cole-Cole, Shin), direct loops and forward() of Cole-Cole.  c2 = fl(c fl(log2 e)) is 2u off, ln w (the host's
 long-double logarithm rounded) u, clt2 = fl(c2 lt) 3u, the fma u:  |dy| <= u (3 |c2 ln w| + 3 |clt2| + |y|)  (Shin: lq2 =
 fl(logQ fl(log2 e)): 2u in place of 3u).  e = 2^y is then ln2 |dy| + 0.89 ulp off, and dT/de e = -T x / (1 + x): the term moves
 by |T| s de with s = |x| / |1 + x| <= 1 (cos >= 0), in both parts.
 Grid loop.  The value at f = 16 k + q is base_k S4^(q / 4) S_(q % 4): base from fma(c2, ln w_16k, clt2): u (2 |c2 ln w_16k| +
 3 |clt2| + |y_16k|) and 0.89 ulp; the exponent it stands for is c log2e (ln w_16k + q d + lt) with |ln w_16k + q d - ln w_f|
 <= 4e-15 (host_precompute.cpp: grid_step; this covers the roundings of ln w_16k and d): c 4e-15 relative.  S1 =
 2^fl(c2 d): dS1 = ln2 3u |c2 d| + 0.89 ulp; S2 = S1 S1: 2 dS1 + u; S3 = S2 S1: 3 dS1 + 2u; S4 = S2 S2: 4 dS1 + 3u; a quarter
 costs dS4 + u, the step dS_s + u: at q = 4 m + s the product carries q (dS1 + u) whichever way q splits -- 15 (1.78 + 1) u =
 41.7 u = 20.9 ulp at q = 15 before the exponent's share (9.3 ulp more at c = 1 on 33 frequencies): the "<= 22 ulp" of
 kernels.h, here per q and not taken on trust.
 omega.  cos, sin are S ulp off (S = 1.5 FAST, 4 otherwise): |d omega| <= 2 S u, and dT = -T e d omega / (1 + x): |T| s 2 S u.
 The FAST form divides by 1 + e (e + 2 cos), |omega| = 1 assumed: 2 (e^2 / den) 2 S u more.
 Roundings of one term, relative to its own part.  FAST: A = fl(m r0), fl(A cos) or fl(A sin), the fma of nr or the product
 of ni, the inner sum and the fma of den: 5u, and the reciprocal of that frequency: rcp_joint<2 D> for a pair (2k, 2k + 1)
 of one or two modes, rcp_batch_n<D> for three and four modes and for a last unpaired frequency of two, rcp_nr for one.
 Safe loop and forward(): dr (in den twice and in the numerator) 3u, di likewise 3u, di di, the fma of den, A, A inv: 10u, and
 rcp_nr.  Shin: yr, yi, yi yi, the fma of den and yr or yi again in the numerator: 5u; rcp_joint<4> for a pair, rcp_batch_n<2>
 for a last unpaired frequency, rcp_nr in the safe loop and forward(); 1/R: a correctly rounded division, |T| (1/R)/|y| u; its
 clamp at 2^110 leaves <= 2^-110 absolute where 1/R exceeds it.  Shin forward(): fl(n ln w) and ln w: 2u |n ln w| on the
 exponent, two exp_finite and their product: 2 * 0.83 ulp + u.
 Sums.  C = r0 - A_1 - ... in order: u sum|A_i| + u sum_i |r0 - sum_(k<=i) A_k|; every fma of the accumulation u times the
 partial sum it returns (from C in the real part; the first imaginary term is a product: u |T_0,im|).  The measured value 0
 is taken last and exactly.  C cancels as sum m -> 1 and carries u r0 whatever is left of it, so the unit of all of this is
 sum|T_i| + |C| + r0 (Shin: sum|T_i|), not |Z|: at sum m = 1 and high frequency |Z| is a thousandth of the unit and a bound
 in |Z| would be false -- the reference's own doubles would miss it.
 Dias.  tau = exp_finite(lt): 0.83 ulp (lt is an input: no conditioning).  tau' = tau (1/delta - 1)/(1 - m): the division u
 amplified 1/(1 - delta) by the subtraction, and 4u; Z depends on tau' through T = A / (1 + z), Re z >= 0: |T| |z / (1 + z)| d tau'.
 Beyond the clamp of tau' at 1e50 both the exact and the clamped term are <= A / (w 1e50): twice that, absolute.  The rest
 is counted along den(): teh = fl(fl(tau |eta|) fl(1/sqrt2)): dtau + 3u; teh2: twice that + u; g = fma(u, tau, teh): dteh + u;
 n2 = fma(g, g, teh2): max(2 dg, dteh2) + u; b = fl(tau' fl(sqrt w)): 2u; X: max(db + dg, dn2) + u; Y: db + max(u + dn2, dteh) +
 2u; D: 2 max(dX, dY) + 2u; t = n2 (A rcp_nr(D)): dn2 + 3u + 1.00 ulp + dD (a pair: two more roundings, the partner's D
 cancels); real part t X, imaginary t Y and its product.  Positive terms throughout, so each d is relative; the count adds
 correlated errors as if they were not (n2 enters t, X, Y and D): it is an upper bound, about 70u.
Second order.  The sum of these first-order terms is doubled (SLACK = 2) for what the expansion drops.  No constant is
fitted to a measurement.  In the reference's default boxes the bound stays <= 1e-13 of that unit, a tenth of what
assert_Z_close allows: `assert_bound_is_worth_having` (5.5e-14 at worst: Dias; 1e-14 for the others).  A subnormal result
is 2^-1075 off, not u times itself: 32 * 2^-1074 per term is added.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ULP = 2.0 * U
ULD = float(np.finfo(LD).eps) / 2
SLACK = 2.0
PROBE_EXP = 100
OTHER_EXP = -10                       # the other sigmas are 2^10
WORTH = 1e-13
TINY = 32 * 2.0 ** -1074               # per term: a subnormal result is 2^-1075 off, not u times itself

EXP2_ULP, EXP_ULP, RCP_NR_ULP, SINCOS_UNIT_ULP, SINCOSPI_ULP = 0.89, 0.83, 1.00, 1.5, 4.0
RCP_JOINT_ULP = {2: 2.4, 4: 3.7}
GRID_DEV = 4e-15
GRID_BLOCK = 16
KERNEL = dict(exp2=EXP2_ULP, exp=EXP_ULP, sincos_fast=SINCOS_UNIT_ULP, sincos_safe=SINCOSPI_ULP, lnw=1.0)
GLIBC = dict(exp2=1.0, exp=1.0, sincos_fast=1.0, sincos_safe=1.0, lnw=1.0)      # 1 ulp each

MODELS = {'PeltonColeCole': 1, 'Dias2000': 2, 'Shin2015': 3}
LOOPS = ('grid', 'fast', 'safe')


# ------------------------------------------------------------------------------------------------------------------
# the probe
# ------------------------------------------------------------------------------------------------------------------
def probes(w, part, j, e=PROBE_EXP):
    """(zn, zn_err) of the probe spectrum for (part, frequency j): measured values 0, sigma 2^-e there, 2^10 elsewhere."""
    N = np.asarray(w).size
    zn = np.zeros((2, N))
    zn_err = np.full((2, N), 2.0 ** -OTHER_EXP)
    zn_err[part, j] = 2.0 ** -e
    return zn, zn_err


def probe_lconst(N, e=PROBE_EXP):
    """-sum ln sigma^2 of a probe spectrum."""
    return float(2.0 * np.log(2.0) * (e + (2 * N - 1) * OTHER_EXP))


def recover(logp, N, zmax, e=PROBE_EXP):
    """|r| from the log-probabilities of a probe spectrum, and the uncertainty du of that reading: 0 where the probed term
    dominates (then the value is the residual's bits), else what lconst, the 2 N - 1 other terms (each <= zmax^2 2^-20)
    and four roundings leave on it.  zmax: an upper bound of |Re Z|, |Im Z| over the spectrum, per row."""
    logp = np.asarray(logp, dtype=np.float64)
    S = -2.0 * logp
    assert np.all(np.isfinite(S)), 'a probe log-probability is not finite'
    rest = (2 * N - 1) * np.asarray(zmax, np.float64) ** 2 * 2.0 ** (2 * OTHER_EXP) + 2.0 * abs(probe_lconst(N, e))
    with np.errstate(invalid='ignore'):
        r = np.sqrt(np.maximum(S, 0.0)) * 2.0 ** -e
    dominant = rest < 2.0 ** -55 * np.maximum(S, 0.0)          # a quarter of an ulp of the probed term
    E = (rest + 4 * ULP * np.abs(S)) * 2.0 ** (-2 * e)          # |S 2^-2e - r^2| otherwise
    with np.errstate(divide='ignore', invalid='ignore'):
        du = np.where(dominant, 0.0, np.minimum(np.sqrt(E), np.where(r > 0, E / r, np.inf)))
    return r, du


# ------------------------------------------------------------------------------------------------------------------
# exact values (long double, and 50-digit mpmath of the literal formula)
# ------------------------------------------------------------------------------------------------------------------
def _omega(c):
    """cos(c pi/2), sin(c pi/2) in long double, relative accuracy kept at c -> 1 (1 - c is exact there)."""
    half = 2 * np.arctan(LD(1))
    up = c > 0.5
    a = np.where(up, 1 - c, c) * half
    s, k = np.sin(a), np.cos(a)
    return np.where(up, s, k), np.where(up, k, s)


def _n_modes(model, ndim):
    return (ndim - 1) // 3 if model == 'PeltonColeCole' else 0


def exact(model, theta, w):
    """The reference's formula at the doubles theta (R, ndim), w (N,), in long double.  dict:
    Z (R, 2, N); T (R, K, 2, N) the terms; Tabs (R, K, N); C (R,) the constant part (0 for Shin); unit (R, N) =
    sum|T| + |C| + r0; ref_err (R, 2, N): the evaluation's own error; and what `bound` needs."""
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    lnw = np.log(wl)
    R = th.shape[0]
    out = dict(model=model, lnw=lnw, w=wl)
    with np.errstate(under='ignore'):
        if model == 'PeltonColeCole':
            D = _n_modes(model, th.shape[1])
            r0, m, lt, c = th[:, 0], th[:, 1:1 + D], th[:, 1 + D:1 + 2 * D], th[:, 1 + 2 * D:]
            yln = c[:, :, None] * (lnw[None, None, :] + lt[:, :, None])
            e = np.exp(yln)
            cs, sn = _omega(c)
            dr, di = 1 + e * cs[:, :, None], e * sn[:, :, None]
            den = dr * dr + di * di
            A = r0[:, None] * m
            T = np.stack([A[:, :, None] * dr / den, -A[:, :, None] * di / den], axis=2)
            one = np.ones(R, dtype=LD)
            partial = []
            for i in range(D):
                one = one - m[:, i]
                partial.append(r0 * one)
            C = partial[-1]
            out.update(D=D, c=c, lt=lt, e=e, den=den, A=A, partial=np.stack(partial, axis=1),
                       sens=e / np.sqrt(den), cond=np.abs(yln))
        elif model == 'Dias2000':
            r0, m, lt, eta, delta = (th[:, k] for k in range(5))
            tau = np.exp(lt)
            taup = tau * ((1 - delta) / delta) / (1 - m)
            teh = tau * np.abs(eta) / np.sqrt(LD(2))
            u = np.sqrt(wl)[None, :]
            g = u * tau[:, None] + teh[:, None]
            n2 = g * g + (teh * teh)[:, None]
            b = taup[:, None] * u
            X, Y = n2 + b * g, b * (u * n2 + teh[:, None])
            Dd = X * X + Y * Y
            A, C = r0 * m, r0 * (1 - m)
            t = A[:, None] * n2 / Dd
            T = np.stack([t * X, -t * Y], axis=1)[:, None]
            out.update(D=1, A=A[:, None], taup=taup, delta=delta, sens=np.sqrt(((b * g) ** 2 + Y * Y) / Dd)[:, None],
                       cond=np.zeros((R, 1, wl.size), dtype=LD))
        else:
            Rr, lq, n = th[:, 0:2], th[:, 2:4], th[:, 4:6]
            yln = lq[:, :, None] + n[:, :, None] * lnw[None, None, :]
            p = np.exp(yln)
            cs, sn = _omega(n)
            invR = 1 / Rr
            yr, yi = p * cs[:, :, None] + invR[:, :, None], p * sn[:, :, None]
            den = yr * yr + yi * yi
            T = np.stack([yr / den, -yi / den], axis=2)
            C = np.zeros(R, dtype=LD)
            out.update(D=2, n=n, lq=lq, p=p, den=den, invR=invR, sens=p / np.sqrt(den),
                       sensR=invR[:, :, None] / np.sqrt(den), cond=np.abs(yln))
    Tabs = np.sqrt(T[:, :, 0] ** 2 + T[:, :, 1] ** 2)
    Z = T.sum(axis=1)
    Z[:, 0] += C[:, None]
    unit = Tabs.sum(axis=1) + np.abs(C)[:, None]
    if model != 'Shin2015':
        unit = unit + np.abs(th[:, 0])[:, None]              # r0: what C = r0 - sum A cancels from
    # the long double's own error, per part: ~40 roundings relative to the part itself, the exponent's conditioning
    # (three roundings of a sum of size cond, and the argument of cos / sin) through |T| s, and, in the real part, the
    # roundings of C = r0 (1 - sum m) (1 - m is not always exact in 64 bits: 2^-64 r0)
    ref_err = ULD * (40 * np.abs(T) + (Tabs * out['sens'] * 3 * (out['cond'] + 2))[:, :, None, :]).sum(axis=1)
    ref_err[:, 0] += 4 * ULD * (np.abs(C) + (np.abs(th[:, 0]) if model != 'Shin2015' else 0))[:, None]
    assert np.all(np.isfinite(Z.astype(np.float64))), 'non-finite exact values are not built'
    out.update(Z=Z, T=T, Tabs=Tabs, C=C, unit=unit, ref_err=ref_err)
    return out


def exact_mp(model, theta_row, w):
    """The literal formula of cython_funcs.pyx in 50-digit mpmath: (2, N) of mpf."""
    import mpmath as mp
    mp.mp.dps = 50
    th = [mp.mpf(float(x)) for x in theta_row]
    out = [[], []]
    for wj in w:
        jw = mp.mpc(0, 1) * mp.mpf(float(wj))
        if model == 'PeltonColeCole':
            D = _n_modes(model, len(th))
            z = mp.mpc(0)
            for i in range(D):
                z += th[1 + i] * (1 - 1 / (1 + (jw * mp.exp(th[1 + D + i])) ** th[1 + 2 * D + i]))
            z = th[0] * (1 - z)
        elif model == 'Dias2000':
            r0, m, lt, eta, delta = th
            tau_p = mp.exp(lt) * (1 / delta - 1) / (1 - m)
            tau_pp = mp.exp(lt) ** 2 * eta ** 2
            mu = jw * mp.exp(lt) + (jw * tau_pp) ** mp.mpf('0.5')
            z = r0 * (1 - m * (1 - 1 / (1 + jw * tau_p * (1 + 1 / mu))))
        else:
            z = mp.mpc(0)
            for i in range(2):
                z_cpe = 1 / (mp.exp(th[2 + i]) * jw ** th[4 + i])
                z += (1 / z_cpe + 1 / th[i]) ** -1
        out[0].append(z.real)
        out[1].append(z.imag)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------
def _rcp_ulps(model, D, N, loop):
    """Relative error (in u) of the reciprocal used at each frequency of the residual path: (N,)."""
    batch = lambda K: (2 * K - 2) + RCP_NR_ULP * 2 if K > 1 else RCP_NR_ULP * 2     # noqa: E731
    if loop == 'safe':
        return np.full(N, RCP_NR_ULP * 2)
    if model == 'Dias2000':
        pair, last = RCP_NR_ULP * 2 + 2, RCP_NR_ULP * 2
    elif model == 'Shin2015':
        pair, last = RCP_JOINT_ULP[4] * 2, batch(2)
    elif D <= 2:
        pair, last = RCP_JOINT_ULP[2 * D] * 2, batch(D)
    else:
        pair = last = batch(min(D, 4))           # groups of at most four within one frequency (D <= 4 here)
    r = np.full(N, float(pair))
    if N % 2:
        r[N - 1] = last
    return r


def grid_extra(q, a2d, consts=KERNEL):
    """What quarter and step add to the relative error of a stepped exponential at q = f mod 16: q (dS1 + u), dS1 the error
    of S1 = 2^fl(c2 d) with a2d = |c2 d| (module docstring)."""
    return q * (float(np.log(2.0)) * 3 * U * a2d + consts['exp2'] * ULP + U)


def bound(ex, loop, path='residual', consts=KERNEL):
    """First-order bound (times SLACK) of |computed - exact| per (row, part, frequency): (R, 2, N) float64.
    ex: what `exact` returned; loop: 'grid' | 'fast' | 'safe' (which frequency loop the context runs; forward() reads
    only whether it is given, its arithmetic is the same in every box); path: 'residual' | 'eval'."""
    model, T, Tabs = ex['model'], np.abs(ex['T']), ex['Tabs']
    R, K, _, N = T.shape
    lnw = ex['lnw']
    assert loop in LOOPS and path in ('residual', 'eval')
    log2e = LD(1) / np.log(LD(2))
    ln2 = float(np.log(2.0))
    fast = path == 'residual' and loop != 'safe'
    dsc = (consts['sincos_fast'] if fast else consts['sincos_safe']) * ULP
    rcp = (_rcp_ulps(model, ex['D'], N, loop) if path == 'residual' else np.full(N, RCP_NR_ULP * 2))[None, None, :] * U
    err = np.zeros((R, 2, N), dtype=LD)
    if model == 'Dias2000':
        dtau = consts['exp'] * 2
        dteh = dtau + 3
        dteh2 = 2 * dteh + 1
        dg = dteh + 1
        dn2 = max(2 * dg, dteh2) + 1
        db = 2.0
        dX = max(db + dg, dn2) + 1
        dY = db + max(1 + dn2, dteh) + 2
        dD = 2 * max(dX, dY) + 2
        dt = dn2 + 3 + dD                                   # and the reciprocal
        dtaup = (dtau + 4 + 1 / (1 - ex['delta'])) * U
        A = np.abs(ex['A'][:, 0])
        clamp = np.where(ex['taup'] > 1e50, 1.0, 0.0)[:, None] * 2 * A[:, None] / (ex['w'][None, :] * LD(1e50))
        common = Tabs[:, 0] * ex['sens'][:, 0] * dtaup[:, None] + clamp
        for p, dpart in ((0, dX), (1, dY + 1)):
            err[:, p] = common + T[:, 0, p] * ((dt + dpart) * U + rcp[0])
        err[:, 0] += U * np.abs(ex['Z'][:, 0]) + U * (A + np.abs(ex['C']))[:, None]
        return (SLACK * err + TINY).astype(np.float64)
    # exponent of term (row, i, frequency), base 2, and its error
    if model == 'PeltonColeCole':
        a2, b2, bk = np.abs(ex['c'] * log2e), np.abs(ex['c'] * log2e * ex['lt']), 3.0
    else:
        a2, b2, bk = np.abs(ex['n'] * log2e), np.abs(ex['lq'] * log2e), 2.0
    y2 = ex['cond'] * log2e
    alnw = np.abs(lnw)[None, None, :]
    if path == 'eval' and model == 'Shin2015':
        de = 2 * U * np.abs(ex['n'])[:, :, None] * alnw + 2 * consts['exp'] * ULP + U
    elif loop == 'grid' and path == 'residual':
        j = np.arange(N)
        blk, q = j - j % GRID_BLOCK, (j % GRID_BLOCK)[None, None, :]
        d = abs(float((lnw[-1] - lnw[0]) / (N - 1)))
        dyb = U * (2 * a2[:, :, None] * alnw[:, :, blk] + bk * b2[:, :, None] + y2[:, :, blk])
        de = ln2 * dyb + (a2 / log2e)[:, :, None] * GRID_DEV + consts['exp2'] * ULP + grid_extra(q, a2[:, :, None] * d, consts)
    else:
        dy = U * ((2 + consts['lnw']) * a2[:, :, None] * alnw + bk * b2[:, :, None] + y2)
        de = ln2 * dy + consts['exp2'] * ULP
    ex['de'] = de
    s = ex['sens']
    if model == 'PeltonColeCole':
        omega = dsc * (s + (2 * ex['e'] ** 2 / ex['den'] if fast else 0))
        moved = Tabs * (s * de + omega)
        kround = 5.0 if fast else 10.0
    else:
        clamp = np.where(ex['invR'] > 2.0 ** 110, LD(2.0) ** -110, LD(0))[:, :, None]
        moved = Tabs * (s * (de + dsc) + ex['sensR'] * U) + clamp
        kround = 5.0
    for p in (0, 1):
        err[:, p] = (moved + T[:, :, p] * (kround * U + rcp)).sum(axis=1)
        run = np.cumsum(T[:, :, p], axis=1)                  # partial sums of the accumulation, an fma each
        if model == 'PeltonColeCole' and p == 0:
            run = run + np.abs(ex['C'])[:, None, None]
        err[:, p] += U * run.sum(axis=1)
    if model == 'PeltonColeCole':
        err[:, 0] += (U * (np.abs(ex['A']).sum(axis=1) + np.abs(ex['partial']).sum(axis=1)))[:, None]
    return (SLACK * err + K * TINY).astype(np.float64)


def assert_reference_is_sharp(ex, bnd):
    """The long double's own error stays under 1/64 of the bound, every row, frequency and part."""
    worst = np.max(ex['ref_err'].astype(np.float64) / bnd)
    assert worst <= 1.0 / 64, f'the long-double reference is {worst:.3g} of the bound'
    return float(worst)


def assert_bound_is_worth_having(ex, bnd):
    """bound <= 1e-13 (sum|T| + |C| + r0): a tenth of the parity tolerance, in the unit that does not cancel."""
    worst = np.max(bnd / ex['unit'].astype(np.float64)[:, None, :])
    assert worst <= WORTH, f'bound / unit = {worst:.3g} > {WORTH:g}'
    return float(worst)


def assert_recovery_is_sharp(du, bnd, unit):
    """du <= bound / 64.  A part at the subnormal scale (m or c = 5e-324: bound ~ 1e-322) no probe can dominate: there the
    reading is good to 2^-90 of the unit -- 1e-11 of the bound of any ordinary entry -- and forward() holds the entry to its
    bound itself."""
    unit = np.asarray(unit, dtype=np.float64)
    ok = (du <= bnd / 64) | (du <= 2.0 ** -90 * unit)
    assert np.all(ok), f'a probe leaves {np.max(du / bnd):.3g} of the bound undetermined'
    return float(np.max(np.where(du <= bnd / 64, du / bnd, 0.0)))


def excess(got_abs, ex, bnd, du=0.0):
    """max over everything of (| got - |exact part| | - du) / bound, got_abs (R, 2, N) magnitudes."""
    want = np.abs(ex['Z'])
    d = np.abs(np.asarray(got_abs, dtype=np.float64).astype(LD) - want).astype(np.float64)
    with np.errstate(over='ignore'):
        return (d - du) / bnd


def signed_excess(got, ex, bnd):
    """(got - exact) / bound for forward()'s signed values."""
    with np.errstate(over='ignore'):
        return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ex['Z']).astype(np.float64) / bnd


# ------------------------------------------------------------------------------------------------------------------
# frequencies, boxes and rows
# ------------------------------------------------------------------------------------------------------------------
def frequencies(N, loop, seed=0):
    """The synthetic geometric grid (descending, 6 kHz .. 11 mHz); off the grid for the direct loops: ln w jittered
    by 1e-3 so that grid_step refuses."""
    f = np.logspace(np.log10(6e3), np.log10(1.1444e-2), N)
    w = 2 * np.pi * f
    if loop != 'grid':
        w = w * np.exp(1e-3 * np.random.RandomState(100 + seed).uniform(-1, 1, N))
    return w


def default_box(model, n_modes=1):
    from bisip_amd.batch import default_params
    kw = dict(n_modes=n_modes) if model == 'PeltonColeCole' else {}
    return np.array(list(default_params(model, **kw).values()), float).T


def wide_box(model, n_modes=1):
    """The default box widened until the safe loop runs (loop_flags == 0), as test_shared_reciprocal... does: tau up to
    e^150 (Cole-Cole), e^40 (Dias), Q up to e^120 (Shin).  The asserted rows stay inside the default box."""
    b = default_box(model, n_modes)
    if model == 'PeltonColeCole':
        b[1, 1 + n_modes:1 + 2 * n_modes] = 150.0
    elif model == 'Dias2000':
        b[1, 2] = 40.0
    else:
        b[1, 2:4] = 120.0
    return b


def _solve_half_integer(c, lnw, k):
    """lt with c log2e (ln w + lt) = k + 1/2: the edge of exp2_finite's reduced range."""
    return (k + 0.5) * np.log(2.0) / c - lnw


def rows(model, n_modes, w, n=256, seed=0):
    """n asserted rows inside the open default box: uniform rows and the edges at which these kernels can go wrong."""
    lo, hi = default_box(model, n_modes)
    rng = np.random.RandomState(seed)
    th = rng.uniform(lo, hi, (n, lo.size))
    up, dn = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
    lnw = np.log(w)
    k = 0

    def take(count):
        nonlocal k
        sl = slice(k, k + count)
        k += count
        return sl

    if model == 'PeltonColeCole':
        D = n_modes
        M, L, Cc = slice(1, 1 + D), slice(1 + D, 1 + 2 * D), slice(1 + 2 * D, 1 + 3 * D)
        th[take(4), Cc] = up(0.0)
        th[take(4), Cc] = dn(1.0)
        s = take(16)
        th[s, Cc] = 0.5 + np.linspace(-8, 7, 16)[:, None] * 2.0 ** -53          # both sides of x > 0.25
        s = take(8)
        th[s, M] = 10.0 ** rng.uniform(-14, -6, (8, D))                         # m -> 0
        th[take(2), M] = up(0.0)
        s = take(8)
        th[s, 1] = 1.0 - 10.0 ** rng.uniform(-16, -6, 8)                        # m -> 1
        if D >= 2:
            s = take(16)                                                        # sum m = 1 +- a few ulp
            m = rng.dirichlet(np.ones(D), 16)
            m[:, 0] = 1.0 - m[:, 1:].sum(axis=1) + np.linspace(-8, 7, 16) * 2.0 ** -53
            th[s, M] = m
        if D >= 2:                                                              # one mode at an edge, the others anywhere
            for col, val in ((Cc.start, up(0.0)), (Cc.stop - 1, dn(1.0)), (M.start, up(0.0)), (M.stop - 1, up(0.0))):
                th[take(2), col] = val
        th[take(4), L] = up(lo[L])
        th[take(4), L] = dn(hi[L])
        s = take(8)                                                             # w tau = 1 at some frequency
        th[s, L] = -lnw[rng.randint(0, w.size, (8, D))]
        s = take(16)                                                            # y = k +- 1/2 at some frequency
        c = th[s, Cc]
        jj = rng.randint(0, w.size, (16, D))
        kk = rng.randint(-6, 6, (16, D))
        lt = _solve_half_integer(c, lnw[jj], kk)
        lt = np.where(np.arange(16)[:, None] % 2, up(lt), dn(lt))
        ok = (lt > lo[L]) & (lt < hi[L])
        th[s, L] = np.where(ok, lt, th[s, L])
    elif model == 'Dias2000':
        th[take(8), 4] = 10.0 ** rng.uniform(-120, -20, 8)                      # delta -> 0: tau' at its clamp
        s = take(16)                                                            # tau' at and beside 1e50
        tau, m = np.exp(th[s, 2]), th[s, 1]
        th[s, 4] = 1.0 / (1e50 * (1 - m) / tau * (1 + np.linspace(-8, 7, 16) * 2.0 ** -50) + 1.0)
        th[take(2), 4] = up(0.0)
        th[take(8), 1] = 1.0 - 10.0 ** rng.uniform(-16, -3, 8)                  # m -> 1
        th[take(2), 1] = dn(1.0)
        th[take(2), 1] = up(0.0)
        th[take(4), 3] = up(0.0)
        th[take(4), 3] = dn(150.0)
        th[take(4), 2] = up(-20.0)
        th[take(4), 2] = dn(0.0)
        s = take(8)
        th[s, 2] = -lnw[rng.randint(0, w.size, 8)]                              # w tau = 1
        th[s, 2] = np.where((th[s, 2] > lo[2]) & (th[s, 2] < hi[2]), th[s, 2], -1.0)
    else:
        th[take(8), 0] = 10.0 ** rng.uniform(-60, -30, 8)                       # R -> 1e-60, one element at a time
        th[take(8), 1] = 10.0 ** rng.uniform(-60, -30, 8)
        th[take(2), 0] = 1e-60
        th[take(2), 1] = 1e-60
        th[take(4), 4:6] = up(0.0)
        th[take(4), 4:6] = dn(1.0)
        s = take(16)
        th[s, 4:6] = 0.5 + np.linspace(-8, 7, 16)[:, None] * 2.0 ** -53
        th[take(4), 2:4] = up(lo[2:4])
        th[take(4), 2:4] = dn(hi[2:4])
        th[take(4), 0:2] = dn(1.0)
        s = take(16)                                                            # y = k +- 1/2 at some frequency
        nn = th[s, 4:6]
        jj = rng.randint(0, w.size, (16, 2))
        y0 = (nn * lnw[jj] + th[s, 2:4]) / np.log(2.0)
        lq = (np.floor(y0) + 0.5) * np.log(2.0) - nn * lnw[jj]
        lq = np.where(np.arange(16)[:, None] % 2, up(lq), dn(lq))
        ok = (lq > lo[2:4]) & (lq < hi[2:4])
        th[s, 2:4] = np.where(ok, lq, th[s, 2:4])
    assert k <= n
    assert np.all((th > lo) & (th < hi)), 'an asserted row left the open box'
    return th


def filler(model, n_modes, count, seed=1):
    lo, hi = default_box(model, n_modes)
    return np.random.RandomState(1000 + seed).uniform(lo, hi, (count, lo.size))


CASES = [('PeltonColeCole', 1), ('PeltonColeCole', 2), ('PeltonColeCole', 3), ('PeltonColeCole', 4), ('Dias2000', 0),
         ('Shin2015', 0)]


def shapes(model, n_modes):
    """(loop, N) at which the loops differ (module docstring of tests/test_gpu_model_exact.py)."""
    out = []
    if model != 'Dias2000' and (n_modes <= 3):
        out += [('grid', 33), ('grid', 21)]
    if model == 'Dias2000' or n_modes <= 2:
        out += [('fast', 5), ('fast', 2)]
    else:
        out += [('fast', 5)]
    out += [('safe', 5)]
    return out
