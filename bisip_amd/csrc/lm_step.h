// lm_step.h -- the dense step of the Levenberg-Marquardt MAP fit (bisip_amd/mapfit.py holds the definitions): the inner
// box, the free set, the Cholesky factorisation of A_ff + lambda D in its stated order, the solve, the predicted
// decrease and the clipped trial.  This is their only implementation in C++: the kernel k_map_fit (dispatch_map.hip) and
// the host entry point bisip_lm_step_host both call the functions below, so that the device's step can be held to the
// host's.  Every array is reached through a pointer and a run-time index (LDS in the kernel: nothing here needs a
// register array, so nothing can go to scratch); every product and sum is rounded on its own (the units are built with
// -ffp-contract=off; no fma is written here).
//
// Order.  `fixed` is a bit mask over the parameters; every loop below runs over the FREE parameters in ascending index
// and skips the fixed ones, which is the factorisation of the compacted matrix A_ff.
//   factor:  for j ascending:  s = A_jj (+ lambda d_j when damped), then s = s - L_jk L_jk for k < j ascending;
//            s > 0 or the factorisation fails (a NaN fails);  L_jj = sqrt(s);
//            for i > j ascending:  t = A_ij, then t = t - L_ik L_jk for k < j ascending;  L_ij = t / L_jj.
//   forward: z_i = (-g_i - sum_{k<i} L_ik z_k) / L_ii, the sum taken from -g_i one term at a time, k ascending.
//   pred:    0.5 * (z_0 z_0 + z_1 z_1 + ...) from 0.0, ascending  (= g_f' A_ff^-1 g_f / 2 of the undamped factor).
//   back:    delta_i = (z_i - sum_{k>i} L_ki delta_k) / L_ii, i descending, k ascending from i + 1;  delta = 0 where fixed.
// Plain C++ when no HIP compiler reads it (tests/native/sanitize_lm_step.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef BISIP_HD            // as philox.h and mode_order.h define it (a unit may hold several of them)
#ifdef __HIPCC__
#define BISIP_HD __host__ __device__ __forceinline__
#else
#define BISIP_HD inline
#endif
#endif

namespace bisip {

constexpr int LM_MAX_NDIM = 16;              // BISIP_MAX_NDIM: the mask has room for 32
constexpr int LM_CANDIDATES = 12;            // lambda, 10 lambda, ..., at most this many per iteration
constexpr int LM_MAX_ITER = 1000;            // the hard bound of the kernel's work
constexpr double LM_STEP_REL = 1e-6;         // stencil step and inner-box margin, as a fraction of hi - lo
constexpr double LM_LAMBDA0 = 1e-3, LM_LAMBDA_MIN = 1e-12;
constexpr int LM_CONVERGED = 0, LM_STALLED = 1, LM_CAP = 2;      // status of the C ABI

// h = 1e-6 (hi - lo);  inner box [lo + h, hi - h]
BISIP_HD void lm_inner_box(int n, const double *lo, const double *hi, double *h, double *lo_in, double *hi_in)
{
    for (int j = 0; j < n; ++j) {
        const double step = LM_STEP_REL * (hi[j] - lo[j]);
        h[j] = step;
        lo_in[j] = lo[j] + step;
        hi_in[j] = hi[j] - step;
    }
}

// x into [lo, hi]; a NaN stays a NaN
BISIP_HD double lm_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// bit j set: theta_j sits on the inner lower bound with g_j > 0 or on the inner upper bound with g_j < 0 -- or A_jj is 0:
// every dZ_j is 0 then, so are g_j and the whole row and column j of A, and the parameter's step is 0 whether it is
// counted as free (lambda D_jj delta_j = 0) or not; left out, it does not make A_ff singular and pred infinite where the
// misfit has simply stopped depending on it (an element of Shin2015 whose R has gone to the bound).
BISIP_HD uint32_t lm_fixed_mask(int n, const double *theta, const double *g, const double *A, const double *lo_in,
                                const double *hi_in)
{
    uint32_t fixed = 0;
    for (int j = 0; j < n; ++j)
        if ((theta[j] <= lo_in[j] && g[j] > 0.0) || (theta[j] >= hi_in[j] && g[j] < 0.0) || A[j * n + j] == 0.0)
            fixed |= 1u << j;
    return fixed;
}

// (D = diag(A_ff).  A zero entry of it never occurs: a parameter whose A_jj is 0 is not in the free set -- lm_fixed_mask.)

// L (n x n, row-major, the lower triangle of the free rows is written) of A_ff + lambda D; lambda <= 0: of A_ff itself
BISIP_HD bool lm_factor(int n, uint32_t fixed, const double *A, double lambda, double *L)
{
    for (int j = 0; j < n; ++j) {
        if (fixed >> j & 1) continue;
        double s = A[j * n + j];
        if (lambda > 0.0) s = s + lambda * s;
        for (int k = 0; k < j; ++k)
            if (!(fixed >> k & 1)) s = s - L[j * n + k] * L[j * n + k];
        if (!(s > 0.0)) return false;
        const double d = std::sqrt(s);
        L[j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            if (fixed >> i & 1) continue;
            double t = A[i * n + j];
            for (int k = 0; k < j; ++k)
                if (!(fixed >> k & 1)) t = t - L[i * n + k] * L[j * n + k];
            L[i * n + j] = t / d;
        }
    }
    return true;
}

// z of L z = -g over the free set (0 where fixed); returns 0.5 z'z
BISIP_HD double lm_forward(int n, uint32_t fixed, const double *L, const double *g, double *z)
{
    double zz = 0.0;
    for (int i = 0; i < n; ++i) {
        if (fixed >> i & 1) { z[i] = 0.0; continue; }
        double t = -g[i];
        for (int k = 0; k < i; ++k)
            if (!(fixed >> k & 1)) t = t - L[i * n + k] * z[k];
        t = t / L[i * n + i];
        z[i] = t;
        zz = zz + t * t;
    }
    return 0.5 * zz;
}

// delta of L' delta = z over the free set, in place (z becomes delta; 0 where fixed)
BISIP_HD void lm_back(int n, uint32_t fixed, const double *L, double *z)
{
    for (int i = n - 1; i >= 0; --i) {
        if (fixed >> i & 1) continue;
        double t = z[i];
        for (int k = i + 1; k < n; ++k)
            if (!(fixed >> k & 1)) t = t - L[k * n + i] * z[k];
        z[i] = t / L[i * n + i];
    }
}

// pred = g_f' A_ff^-1 g_f / 2; +inf when A_ff is not positive definite.  L and z are workspaces (n x n, n).
BISIP_HD double lm_pred(int n, uint32_t fixed, const double *A, const double *g, double *L, double *z)
{
    if (!lm_factor(n, fixed, A, 0.0, L)) return HUGE_VAL;
    return lm_forward(n, fixed, L, g, z);
}

// One candidate: trial = clip(theta + delta) with (A_ff + lambda D) delta = -g_f; lambda <= 0: the undamped system.
// false: the factorisation failed and neither trial nor half_zz is written.  half_zz = z'z / 2 of the forward solve: with
// lambda <= 0 it is pred (lm_pred).  L and delta are workspaces (n x n, n); delta holds the step afterwards.
BISIP_HD bool lm_candidate(int n, uint32_t fixed, const double *A, const double *g, const double *theta, const double *lo_in,
                           const double *hi_in, double lambda, double *L, double *delta, double *trial, double *half_zz)
{
    if (!lm_factor(n, fixed, A, lambda, L)) return false;
    *half_zz = lm_forward(n, fixed, L, g, delta);
    lm_back(n, fixed, L, delta);
    for (int j = 0; j < n; ++j) trial[j] = lm_clip(theta[j] + delta[j], lo_in[j], hi_in[j]);
    return true;
}

// What bisip_lm_step_host returns for one (A, g, theta, box, lambda): every pointer a host pointer.
inline void lm_step_host(int n, const double *A, const double *g, const double *theta, const double *lo, const double *hi,
                         double lambda, double *delta, double *trial, double *pred, int64_t *fixed_out, int *ok)
{
    double h[LM_MAX_NDIM], lo_in[LM_MAX_NDIM], hi_in[LM_MAX_NDIM], L[LM_MAX_NDIM * LM_MAX_NDIM], z[LM_MAX_NDIM],
        t[LM_MAX_NDIM];
    lm_inner_box(n, lo, hi, h, lo_in, hi_in);
    const uint32_t fixed = lm_fixed_mask(n, theta, g, A, lo_in, hi_in);
    if (fixed_out) *fixed_out = (int64_t)fixed;
    const double p = lm_pred(n, fixed, A, g, L, z);
    if (pred) *pred = p;
    for (int j = 0; j < n; ++j) { z[j] = 0.0; t[j] = theta[j]; }
    double half_zz = 0.0;
    const bool good = lm_candidate(n, fixed, A, g, theta, lo_in, hi_in, lambda, L, z, t, &half_zz);
    if (ok) *ok = good ? 1 : 0;
    for (int j = 0; j < n; ++j) {
        if (delta) delta[j] = good ? z[j] : NAN;
        if (trial) trial[j] = good ? t[j] : NAN;
    }
}

}  // namespace bisip
