// host_emulate.inc -- the inner loops of the reduced-form estimates, included TWICE by host_precompute.cpp:
// once as plain x86-64 code and once inside __attribute__((target("fma"))) functions, where __builtin_fma is
// one instruction instead of a libm call (a context's estimate is ~100,000 of them); the caller picks at run
// time with __builtin_cpu_supports("fma").  Both are correctly rounded fused multiply-adds: the same bits.
// EMU(name) names the instantiation, EMU_ATTR carries the target attribute.
// What holds chi2_kernel and the kernels together: tests/test_reduced_emulation.py compares it (through
// bisip_reduced_emulate) with an exact rational statement of the sequence, tests/test_gpu_reduced_bits.py compares
// every instantiation and launch route of logprob_row_reduced with it -- both by equality of bits.  Change one side
// and the other has to follow.

// logprob_row_reduced<P, COMP> (kernels.h) in the same double arithmetic, operation for operation.
// R: (n,n) the triangle the kernel holds; Rlo: its low word as the kernel holds it (floats; compensated form only)
EMU_ATTR static double EMU(chi2_kernel)(int n, const double *R, const float *Rlo, const double *bhat, const double *e,
                                        const double *elo, double rest, const double *th, bool comp)
{
    double chi2 = rest;
    double d[BISIP_HOST_MAXN], dl[BISIP_HOST_MAXN];
    if (!comp) {
        d[0] = bhat[0] - th[0];
        for (int q = 1; q < n; ++q) {
            const double prod = th[0] * th[q];
            d[q] = bhat[q] - prod;
        }
        for (int i = 0; i < n; ++i) {
            double u = e[i];
            for (int j = i; j < n; ++j) u = __builtin_fma(R[(size_t)i * n + j], d[j], u);
            chi2 = __builtin_fma(u, u, chi2);
        }
        return chi2;
    }
    {   // two_diff(bhat[0], th[0])
        const double a = bhat[0], b = th[0], s = a - b, bb = s - a;
        d[0] = s;
        dl[0] = (a - (s - bb)) + ((-b) - bb);
    }
    for (int q = 1; q < n; ++q) {
        const double p = th[0] * th[q];
        const double pe = __builtin_fma(th[0], th[q], -p);
        const double a = bhat[q], s = a - p, bb = s - a;
        const double err = (a - (s - bb)) + ((-p) - bb);
        d[q] = s;
        dl[q] = err - pe;
    }
    for (int i = 0; i < n; ++i) {
        double s = e[i], c = elo[i];
        for (int j = i; j < n; ++j) {
            const double Rk = R[(size_t)i * n + j];
            const double h = Rk * d[j];
            const double l = __builtin_fma(Rk, d[j], -h);
            const double t = s + h;
            const double bb = t - s;
            const double er = (s - (t - bb)) + (h - bb);
            s = t;
            c += er + l;
            c = __builtin_fma(Rk, dl[j], c);
            c = __builtin_fma((double)Rlo[(size_t)i * n + j], d[j], c);
        }
        const double u = s + c;
        chi2 = __builtin_fma(u, u, chi2);
    }
    return chi2;
}

// chi^2 of the reduced form from operands of twice the working precision -- R = Rhi + Rlo and Q^T y = qhi + qlo,
// exact splits of the long-double QR -- every row  qty_i - sum_j R_ij b_j  accumulated as a double-double
// (TwoProduct by fma, TwoSum; Ogita-Rump-Oishi Dot2, b_j = R0 a_j split the same way) and squared in long
// double: good to ~1e-30 of the terms, i.e. as good as its operands.  The yardstick of the plain tier.
EMU_ATTR static long double EMU(chi2_dd)(int n, const double *Rhi, const double *Rlo, const double *qhi, const double *qlo,
                                         double rest, const double *th)
{
    double bh[BISIP_HOST_MAXN], bl[BISIP_HOST_MAXN];
    bh[0] = th[0];
    bl[0] = 0.0;
    for (int j = 1; j < n; ++j) {
        const double p = th[0] * th[j];
        bh[j] = p;
        bl[j] = __builtin_fma(th[0], th[j], -p);
    }
    long double chi2 = rest;
    for (int i = 0; i < n; ++i) {
        double hi = qhi[i], lo = qlo[i];
        for (int j = i; j < n; ++j) {
            const double r = -Rhi[(size_t)i * n + j];
            const double p = r * bh[j];
            const double pe = __builtin_fma(r, bh[j], -p);
            const double s = hi + p;
            const double bb = s - hi;
            const double se = (hi - (s - bb)) + (p - bb);
            hi = s;
            lo += (se + pe) + (r * bl[j] - Rlo[(size_t)i * n + j] * bh[j]);
        }
        const long double u = (long double)hi + (long double)lo;
        chi2 += u * u;
    }
    return chi2;
}

// worst weighted relative log-probability error of the kernel arithmetic over the probe rows, for one
// candidate expansion point (exact[ip] = the yardstick's chi^2 of probe ip)
EMU_ATTR static double EMU(worst_error)(int n, const double *R, const float *Rlo, const double *bhat, const double *e,
                                        const double *elo, double rest, bool comp, const double *rows, size_t count,
                                        size_t n_regular, const long double *exact, double lconst, double w_shell)
{
    double worst = 0.0;
    for (size_t ip = 0; ip < count; ++ip) {
        const double got = EMU(chi2_kernel)(n, R, Rlo, bhat, e, elo, rest, rows + ip * (size_t)n, comp);
        const long double lp = -0.5L * exact[ip] + (long double)lconst;
        const long double scale = fabsl(lp) > 1.0L ? fabsl(lp) : 1.0L;
        double rel = (double)(fabsl(-0.5L * ((long double)got - exact[ip])) / scale);
        if (ip >= n_regular) rel *= w_shell;    // shell probes
        if (!(rel <= worst)) worst = rel;       // NaN counts as worst
    }
    return worst;
}
