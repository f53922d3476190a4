// rtd_descriptors.h -- the relaxation descriptors of ONE row of a PolynomialDecomposition chain: the RTD's peak and the
// cumulative relaxation times log_tau_q.  The definitions, step by step, are in the module docstring of
// bisip_amd/decomposition.py ("Relaxation descriptors"); this is their only implementation in C++.  The kernel
// k_rtd_descriptors<ND> and the host entry point bisip_rtd_descriptors_host (chain_rtd_descriptors.hip) both call
// rtd_descriptor_row<ND>, so that the device's bits can be held to the host's.  Explicit fma() only, plain additions,
// one multiplication and one IEEE division per fraction: nothing here may be contracted or reordered.
// Plain C++ when no HIP compiler reads it (tests/native/sanitize_rtd_descriptors.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define BISIP_HD __host__ __device__
#else
#define BISIP_HD
#endif

namespace bisip {

constexpr int RTD_MAX_FRACTIONS = 8;      // 1 <= n_q <= 8: t_j and the values stay in registers

// th: the row (r0, a_0, ..., a_P), ND = P + 2 values (r0 is not used); x: log_tau (L,), strictly ascending; q: (nq,)
// fractions in (0, 1].  out: 2 + nq doubles (log_tau_peak, m_peak, log_tau_q1, ..., log_tau_qJ), all NaN for a row
// whose clipped RTD has no finite positive sum.
template <int ND>
BISIP_HD inline void rtd_descriptor_row(const double *th, const double *x, int L, const double *q, int nq, double *out)
{
    constexpr int P = ND - 2;
    const double nan = __builtin_nan("");
    // pass 1: g_l = g_{l-1} + c_l, c_l = m_l > 0 ? m_l : 0; the first l of the largest m_l (unclipped, strict >)
    // (x_{l+1} is asked for before x_l is used: on the device the load is a scalar one, and its latency is then hidden)
    double g = 0.0, pm = 0.0, px = 0.0, xn = x[0];
    for (int l = 0; l < L; ++l) {
        const double xl = xn;
        xn = x[l + 1 < L ? l + 1 : l];
        double m = th[1 + P];
#pragma unroll
        for (int p = P - 1; p >= 0; --p) m = fma(m, xl, th[1 + p]);
        g = g + (m > 0.0 ? m : 0.0);
        if (l == 0 || m > pm) { pm = m; px = xl; }
    }
    const double total = g;
    if (!(total > 0.0 && total < INFINITY)) {
        for (int k = 0; k < 2 + nq; ++k) out[k] = nan;
        return;
    }
    out[0] = px;
    out[1] = pm != pm ? nan : pm;
    // pass 2: the same additions give the same g_l; t_j = q_j * total is met first at k_j.  A fraction that has been
    // met gets t_j = inf and is not met again.
    double t[RTD_MAX_FRACTIONS], v[RTD_MAX_FRACTIONS];
#pragma unroll
    for (int j = 0; j < RTD_MAX_FRACTIONS; ++j) {
        t[j] = j < nq ? q[j] * total : INFINITY;
        v[j] = nan;
    }
    double xp = 0.0;
    g = 0.0;
    xn = x[0];
    for (int l = 0; l < L; ++l) {
        const double xl = xn;
        xn = x[l + 1 < L ? l + 1 : l];
        double m = th[1 + P];
#pragma unroll
        for (int p = P - 1; p >= 0; --p) m = fma(m, xl, th[1 + p]);
        const double c = m > 0.0 ? m : 0.0;
        const double gl = g + c;
#pragma unroll
        for (int j = 0; j < RTD_MAX_FRACTIONS; ++j)
            if (gl >= t[j]) {                    // g_{l-1} < t_j <= g_l, hence c > 0 for l > 0
                v[j] = l == 0 ? xl : fma((t[j] - g) / c, xl - xp, xp);
                t[j] = INFINITY;
            }
        g = gl;
        xp = xl;
    }
#pragma unroll
    for (int j = 0; j < RTD_MAX_FRACTIONS; ++j)
        if (j < nq) out[2 + j] = v[j];
}

// every row of every sample on the host: chain and out as bisip_rtd_descriptors_dev takes them, host pointers
template <int ND>
inline void rtd_descriptor_rows_host(const double *chain, int64_t n_samples, int64_t sample_stride, int64_t rows,
                                     const double *x, int L, const double *q, int nq, double *out)
{
    for (int64_t s = 0; s < n_samples; ++s)
        for (int64_t r = 0; r < rows; ++r)
            rtd_descriptor_row<ND>(chain + s * sample_stride + r * ND, x, L, q, nq, out + (s * rows + r) * (2 + nq));
}

// rtd_descriptor_rows_host<ndim> for ndim = 2 ... MAXND; false for an ndim outside
template <int MAXND, int ND = 2>
inline bool rtd_descriptor_rows_host_by_ndim(int ndim, const double *chain, int64_t n_samples, int64_t sample_stride,
                                             int64_t rows, const double *x, int L, const double *q, int nq, double *out)
{
    if (ndim == ND) {
        rtd_descriptor_rows_host<ND>(chain, n_samples, sample_stride, rows, x, L, q, nq, out);
        return true;
    }
    if constexpr (ND < MAXND)
        return rtd_descriptor_rows_host_by_ndim<MAXND, ND + 1>(ndim, chain, n_samples, sample_stride, rows, x, L, q, nq, out);
    else
        return false;
}

}  // namespace bisip
