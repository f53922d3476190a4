// dispatch_map.hip -- the Gauss-Newton normal equations of the Gaussian misfit at given points (bisip_gauss_newton_dev)
// and the multi-start Levenberg-Marquardt MAP fit built on them (bisip_map_fit_dev), with the dense step on the host for
// tests (bisip_lm_step_host).  The definitions are bisip_amd/mapfit.py (normal_equations, lm_fit);
// mapfit.ordered_normal_equations restates the order of every sum below in NumPy: the same bits from the same responses.
//
// One wave (a workgroup of 64 threads) takes one (spectrum, point).  With h_j = 1e-6 (hi_j - lo_j):
//   * Stencil.  Lane 0 holds the point theta, lane 1 + 2j theta + h_j e_j, lane 2 + 2j theta - h_j e_j (j < ndim: 33 lanes
//     at ndim = 16); the lanes beyond hold theta again.  Every lane runs M::setup once and eval_const<M> per frequency (the
//     bits of forward()); the records are wave-uniform and go through the scalar path.
//   * Differences.  Per frequency lane j < ndim fetches the responses of lanes 1 + 2j and 2 + 2j (cross-lane reads) and
//     takes dZ_j = (Z+ - Z-) / (2 h_j), a division; d = y - Z(theta), iv = rec[2], rec[3] as fq_q of dispatch_fit.hip reads
//     them.
//   * Sums.  chi2 = sum (d d) iv;  g_j = -sum (dZ_j d) iv;  A_jk = sum (dZ_j dZ_k) iv -- lane j keeps g_j and row j of A in
//     registers, dZ_k comes from lane k.  Frequencies ascending, the real part before the imaginary one, every sum from 0.0,
//     every product and sum rounded on its own (no fma).
//   * A point with a parameter that is not finite gives NaN in every output of that point.
//
// k_map_fit runs the loop of mapfit.lm_fit for one (spectrum, start) per wave, without host round trips or waits between
// workgroups: normal equations as above, then lanes 0 ... 11 each factor A_ff + lambda 10^c D and solve for their
// candidate while lane 12 factors A_ff itself for pred (lm_step.h: every lane has a workspace of its own in LDS), then the
// twelve lanes evaluate chi2 of their trials side by side and the FIRST candidate in the order lambda, 10 lambda, ... that
// is finite and strictly lower is taken (a ballot): the sequential rule's result.  A and every Cholesky factor live in LDS
// (13 workspaces of ndim^2 + 2 ndim doubles: 30 KB at ndim = 16); a start's result does not depend on any other wave.
//
// Resource report (-Rpass-analysis=kernel-resource-usage, gfx950): no scratch and no AGPRs in any of the 36 kernels.
// k_gauss_newton: no LDS; 44-126 VGPRs for PolynomialDecomposition of degree 0-10 (8 waves per SIMD up to degree 3, 4 from
// degree 8), 77 / 90 / 120 / 108 / 127 for one to five Cole-Cole modes (6, 5, 4, 4, 4 waves), Dias 60 (8), Shin 78 (6).
// k_map_fit: 64-190 VGPRs and 728 B - 19 KB of LDS for PolynomialDecomposition (8 waves at degree 0, 4 at degree 5, 2 at
// degree 10), 124 / 113 / 154 / 225 / 235 VGPRs and 2.3 / 6.5 / 13.6 / 22.1 / 32.7 KB for one to five Cole-Cole modes
// (4, 4, 3, 2, 2 waves), Dias 118 VGPRs and 3.5 KB (4), Shin 123 and 4.9 KB (4).
#include "host.h"
#include "lm_step.h"

using namespace bisip;
using namespace bisip::host;

namespace {

typedef const double __attribute__((address_space(4))) *const_ptr;   // scalar loads, as eval_const

struct GnArgs {
    const double *theta;         // (n_spectra, S, ndim)
    long long S;
    int N;
    const double *cb;            // records of the call's first spectrum
    long long cb_stride;
    Bounds b;
    double *chi2, *g, *A;        // (n_spectra, S), (n_spectra, S, ndim), (n_spectra, S, ndim, ndim); any may be null
};

struct MapArgs {
    const double *starts;        // (n_spectra, S, ndim)
    long long S;
    int N;
    const double *cb;
    long long cb_stride;
    Bounds b;
    const double *lconst_dev;    // the constant of the call's first spectrum and its successors; null: lconst
    double lconst;
    int max_iter;
    double pred_tol;
    double *theta, *chi2, *logp, *pred, *A;
    long long *iterations, *status;
};

// chi2, g and A at the point th, which every lane holds.  Afterwards every lane holds chi2, lane j < NDIM g_j and row j of A.
template <class M>
__device__ __forceinline__ void normal_equations(const double (&th)[M::NDIM], const Bounds &b, const double *cb, int N,
                                                 double &chi2, double &g, double (&row)[M::NDIM])
{
    constexpr int NDIM = M::NDIM;
    const int lane = threadIdx.x;
    const int p = lane <= 2 * NDIM ? lane : 0;
    const int jp = (p - 1) >> 1;                          // the parameter this lane moves (p >= 1)
    const bool minus = ((p - 1) & 1) != 0;
    double tp[NDIM], two_h = 1.0;
#pragma unroll
    for (int q = 0; q < NDIM; ++q) {
        const double h = LM_STEP_REL * (b.hi[q] - b.lo[q]);
        tp[q] = (p >= 1 && q == jp) ? (minus ? th[q] - h : th[q] + h) : th[q];
        if (q == lane) two_h = 2.0 * h;
    }
    const typename M::Setup s = M::setup(tp);
    const int src_plus = lane < NDIM ? 1 + 2 * lane : 0, src_minus = lane < NDIM ? 2 + 2 * lane : 0;
    double sc = 0.0, sg = 0.0;
#pragma unroll
    for (int k = 0; k < NDIM; ++k) row[k] = 0.0;
#pragma unroll 1
    for (int f = 0; f < N; ++f) {
        const double *rec = cb + (long long)f * M::REC;
        const const_ptr r = (const_ptr)rec;
        double zr, zi;
        eval_const<M>(s, rec, zr, zi);
        const double dr = r[0] - __shfl(zr, 0, 64), di = r[1] - __shfl(zi, 0, 64);
        const double jr = (__shfl(zr, src_plus, 64) - __shfl(zr, src_minus, 64)) / two_h;
        const double ji = (__shfl(zi, src_plus, 64) - __shfl(zi, src_minus, 64)) / two_h;
        const double ivr = r[2], ivi = r[3];
        sc = sc + (dr * dr) * ivr;
        sc = sc + (di * di) * ivi;
        sg = sg + (jr * dr) * ivr;
        sg = sg + (ji * di) * ivi;
#pragma unroll
        for (int k = 0; k < NDIM; ++k) {
            const double kr = __shfl(jr, k, 64), ki = __shfl(ji, k, 64);
            row[k] = row[k] + (jr * kr) * ivr;
            row[k] = row[k] + (ji * ki) * ivi;
        }
    }
    chi2 = sc;
    g = -sg;
}

// chi2 at this lane's own point, in the order of normal_equations
template <class M>
__device__ __forceinline__ double chi2_at(const double (&th)[M::NDIM], const double *cb, int N)
{
    const typename M::Setup s = M::setup(th);
    double sc = 0.0;
#pragma unroll 1
    for (int f = 0; f < N; ++f) {
        const double *rec = cb + (long long)f * M::REC;
        const const_ptr r = (const_ptr)rec;
        double zr, zi;
        eval_const<M>(s, rec, zr, zi);
        const double dr = r[0] - zr, di = r[1] - zi;
        sc = sc + (dr * dr) * r[2];
        sc = sc + (di * di) * r[3];
    }
    return sc;
}

// grid (n_spectra * S): workgroup b takes point b % S of spectrum b / S
template <class M>
__global__ __launch_bounds__(64) void k_gauss_newton(const GnArgs a)
{
    constexpr int NDIM = M::NDIM;
    const int lane = threadIdx.x;
    const long long pt = blockIdx.x, e = pt / a.S;
    const double *__restrict__ cb = a.cb + e * a.cb_stride;
    const double *__restrict__ src = a.theta + pt * NDIM;
    double th[NDIM];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < NDIM; ++q) {
        th[q] = src[q];
        bad |= !(fabs(th[q]) < HUGE_VAL);                           // NaN or +-inf
    }
    double chi2, g, row[NDIM];
    normal_equations<M>(th, a.b, cb, a.N, chi2, g, row);
    const double nan = __builtin_nan("");
    if (lane == 0 && a.chi2) a.chi2[pt] = bad ? nan : chi2;
    if (lane < NDIM) {
        if (a.g) a.g[pt * NDIM + lane] = bad ? nan : g;
        if (a.A) {
            double *__restrict__ out = a.A + (pt * NDIM + lane) * NDIM;
#pragma unroll
            for (int k = 0; k < NDIM; ++k) out[k] = bad ? nan : row[k];
        }
    }
}

// grid (n_spectra * S): workgroup b takes start b % S of spectrum b / S
template <class M>
__global__ __launch_bounds__(64) void k_map_fit(const MapArgs a)
{
    constexpr int NDIM = M::NDIM, NC = LM_CANDIDATES, NW = NC + 1;  // workspace NC: the undamped factor, for pred
    __shared__ double s_lo[NDIM], s_hi[NDIM], s_h[NDIM], s_lo_in[NDIM], s_hi_in[NDIM];
    __shared__ double s_th[NDIM], s_g[NDIM], s_A[NDIM * NDIM];
    __shared__ double s_L[NW][NDIM * NDIM], s_delta[NW][NDIM], s_trial[NW][NDIM];
    __shared__ double s_pred;

    const int lane = threadIdx.x;
    const long long pt = blockIdx.x, e = pt / a.S;
    const double *__restrict__ cb = a.cb + e * a.cb_stride;
    const double *__restrict__ src = a.starts + pt * NDIM;

    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NDIM; ++q) { s_lo[q] = a.b.lo[q]; s_hi[q] = a.b.hi[q]; }
        lm_inner_box(NDIM, s_lo, s_hi, s_h, s_lo_in, s_hi_in);
    }
    __syncthreads();
    double th[NDIM];
#pragma unroll
    for (int q = 0; q < NDIM; ++q) th[q] = lm_clip(src[q], s_lo_in[q], s_hi_in[q]);

    double lambda = LM_LAMBDA0, chi2, g, row[NDIM], pred;
    int it = 0, status = LM_CAP;
    for (;;) {
        normal_equations<M>(th, a.b, cb, a.N, chi2, g, row);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NDIM; ++q) s_th[q] = th[q];
        }
        if (lane < NDIM) {
            s_g[lane] = g;
#pragma unroll
            for (int k = 0; k < NDIM; ++k) s_A[lane * NDIM + k] = row[k];
        }
        __syncthreads();
        bool ok = false;
        if (lane < NW) {
            const uint32_t fixed = lm_fixed_mask(NDIM, s_th, s_g, s_A, s_lo_in, s_hi_in);
            double lam = lane == NC ? 0.0 : lambda, half_zz = 0.0;
            for (int i = 0; i < lane && lane < NC; ++i) lam = lam * 10.0;
            ok = lm_candidate(NDIM, fixed, s_A, s_g, s_th, s_lo_in, s_hi_in, lam, s_L[lane], s_delta[lane], s_trial[lane],
                              &half_zz);
            if (lane == NC) s_pred = ok ? half_zz : HUGE_VAL;
        }
        __syncthreads();
        pred = s_pred;
        if (pred <= a.pred_tol) { status = LM_CONVERGED; break; }
        if (it >= a.max_iter) { status = LM_CAP; break; }
        // Every lane of the wave runs chi2_at, as a wave executes all its lanes together anyway: the twelve that hold a
        // candidate on their trial, the others -- and a lane whose factorisation failed, whose row of s_trial was never
        // written: what is read there is discarded by the select below, on purpose -- on a copy of theta.
        const bool mine = lane < NC && ok;
        double tc[NDIM];
#pragma unroll
        for (int q = 0; q < NDIM; ++q) {
            const double t = s_trial[lane < NC ? lane : 0][q];
            tc[q] = mine ? t : th[q];
        }
        const double c2 = chi2_at<M>(tc, cb, a.N);
        const unsigned long long good = __ballot(mine && fabs(c2) < HUGE_VAL && c2 < chi2);
        if (!good) { status = LM_STALLED; break; }
        const int taken = __ffsll((long long)good) - 1;
#pragma unroll
        for (int q = 0; q < NDIM; ++q) th[q] = s_trial[taken][q];
        for (int i = 0; i < taken; ++i) lambda = lambda * 10.0;
        lambda = lambda / 10.0;
        if (!(lambda > LM_LAMBDA_MIN)) lambda = LM_LAMBDA_MIN;
        ++it;
        __syncthreads();                                            // s_th, s_g, s_A and the workspaces are rewritten
    }
    if (lane == 0) {
        if (a.theta) {
#pragma unroll
            for (int q = 0; q < NDIM; ++q) a.theta[pt * NDIM + q] = th[q];
        }
        if (a.chi2) a.chi2[pt] = chi2;
        if (a.logp) a.logp[pt] = -0.5 * chi2 + (a.lconst_dev ? a.lconst_dev[e] : a.lconst);
        if (a.pred) a.pred[pt] = pred;
        if (a.iterations) a.iterations[pt] = it;
        if (a.status) a.status[pt] = status;
    }
    if (lane < NDIM && a.A) {
        double *__restrict__ out = a.A + (pt * NDIM + lane) * NDIM;
#pragma unroll
        for (int k = 0; k < NDIM; ++k) out[k] = row[k];
    }
}

template <class M>
int launch_gauss_newton(const GnArgs &a, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL((k_gauss_newton<M>), dim3(blocks), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

template <class M>
int launch_map_fit(const MapArgs &a, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL((k_map_fit<M>), dim3(blocks), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

// what both entry points ask of the context, the spectra and the points
int check_map_shape(const bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const void *points, int64_t S)
{
    if (!c || !points) return fail(BISIP_EINVAL, "null argument");
    if (n_spectra < 1 || first_spectrum < 0 || first_spectrum + n_spectra > c->E)
        return fail(BISIP_EINVAL, "spectra [%lld, %lld) of %d", (long long)first_spectrum, (long long)(first_spectrum + n_spectra), c->E);
    if (S < 1 || S > 0x7fffffffLL / n_spectra)
        return fail(BISIP_EINVAL, "%lld points for each of %lld spectra: one workgroup each, at most 2^31 - 1", (long long)S, (long long)n_spectra);
    for (int q = 0; q < c->ndim; ++q)
        if (!(std::fabs(c->bounds.lo[q]) < HUGE_VAL) || !(std::fabs(c->bounds.hi[q]) < HUGE_VAL))
            return fail(BISIP_EINVAL, "the prior box of parameter %d is not finite: the stencil step is a fraction of it", q);
    return BISIP_OK;
}

}  // namespace

extern "C" {

int bisip_gauss_newton_dev(bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const double *d_theta, int64_t S,
                           double *d_chi2, double *d_g, double *d_A, void *stream)
{
    int rc = check_map_shape(c, first_spectrum, n_spectra, d_theta, S);
    if (rc != BISIP_OK) return rc;
    if (((uintptr_t)d_theta % 8) || ((uintptr_t)d_chi2 % 8) || ((uintptr_t)d_g % 8) || ((uintptr_t)d_A % 8))
        return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    if (!d_chi2 && !d_g && !d_A) return BISIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    GnArgs a{};
    a.theta = d_theta; a.S = S; a.N = c->N;
    a.cb = c->d_cb + first_spectrum * c->cb_stride; a.cb_stride = c->cb_stride;
    a.b = c->bounds;
    a.chi2 = d_chi2; a.g = d_g; a.A = d_A;
    const unsigned blocks = (unsigned)(n_spectra * S);
    hipStream_t st = (hipStream_t)stream;
    return with_model(c, "gauss-newton", [&](auto m) { return launch_gauss_newton<typename decltype(m)::type>(a, blocks, st); });
}

int bisip_map_fit_dev(bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const double *d_starts, int64_t S,
                      int64_t max_iter, double pred_tol, double *d_theta, double *d_chi2, double *d_logp, double *d_pred,
                      double *d_A, int64_t *d_iterations, int64_t *d_status, void *stream)
{
    int rc = check_map_shape(c, first_spectrum, n_spectra, d_starts, S);
    if (rc != BISIP_OK) return rc;
    if (max_iter < 0 || max_iter > LM_MAX_ITER) return fail(BISIP_EINVAL, "max_iter %lld outside [0, %d]", (long long)max_iter, LM_MAX_ITER);
    if (pred_tol != pred_tol) return fail(BISIP_EINVAL, "pred_tol is NaN");
    if (((uintptr_t)d_starts % 8) || ((uintptr_t)d_theta % 8) || ((uintptr_t)d_chi2 % 8) || ((uintptr_t)d_logp % 8) ||
        ((uintptr_t)d_pred % 8) || ((uintptr_t)d_A % 8) || ((uintptr_t)d_iterations % 8) || ((uintptr_t)d_status % 8))
        return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    if (!d_theta && !d_chi2 && !d_logp && !d_pred && !d_A && !d_iterations && !d_status) return BISIP_OK;
    if (c->E > 1 && !c->d_lconst) return fail(BISIP_EINVAL, "the batch holds no constants of its spectra");
    HIP_TRY(hipSetDevice(c->device));
    MapArgs a{};
    a.starts = d_starts; a.S = S; a.N = c->N;
    a.cb = c->d_cb + first_spectrum * c->cb_stride; a.cb_stride = c->cb_stride;
    a.b = c->bounds;
    a.lconst_dev = c->E > 1 ? c->d_lconst + first_spectrum : nullptr;
    a.lconst = c->lconst;
    a.max_iter = (int)max_iter; a.pred_tol = pred_tol;
    a.theta = d_theta; a.chi2 = d_chi2; a.logp = d_logp; a.pred = d_pred; a.A = d_A;
    a.iterations = (long long *)d_iterations; a.status = (long long *)d_status;
    const unsigned blocks = (unsigned)(n_spectra * S);
    hipStream_t st = (hipStream_t)stream;
    return with_model(c, "map-fit", [&](auto m) { return launch_map_fit<typename decltype(m)::type>(a, blocks, st); });
}

int bisip_lm_step_host(int ndim, const double *A, const double *g, const double *theta, const double *lo, const double *hi,
                       double lambda, double *delta, double *trial, double *pred, int64_t *fixed, int *ok)
{
    if (ndim < 1 || ndim > LM_MAX_NDIM) return fail(BISIP_EINVAL, "ndim %d outside [1, %d]", ndim, LM_MAX_NDIM);
    if (!A || !g || !theta || !lo || !hi) return fail(BISIP_EINVAL, "null argument");
    lm_step_host(ndim, A, g, theta, lo, hi, lambda, delta, trial, pred, fixed, ok);
    return BISIP_OK;
}

}  // extern "C"
