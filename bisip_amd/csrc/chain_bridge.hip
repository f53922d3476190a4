// chain_bridge.hip -- the four device steps of the bridge-sampling estimate of the log marginal likelihood of every
// ensemble of a device-resident chain (Meng & Wong 1996; the arrangement of Gronau et al. 2017).  The definitions are
// bisip_amd/evidence.py (bridge_terms, bridge_iterate); evidence.ordered_logg and evidence.ordered_iterate restate the
// order of every operation of bisip_bridge_logg_dev and bisip_bridge_iterate_dev in NumPy and give the same bits.
//
// The proposal of ensemble e is the normal density of mean mu (ndim) and lower Cholesky factor L (ndim, ndim, row-major,
// the upper triangle is never read), with c = sum_j log L_jj + (ndim / 2) log(2 pi) taken by the caller.
//
//   * bisip_bridge_logg_dev: l = logp - log_g(x) of every stored row.  Rows are cut as chain_cov.hip cuts them (a
//     workgroup of 256 threads per (ensemble, segment), tiles of 256 rows staged through LDS in whole lines, row pitch
//     ndim | 1); L and mu go to LDS once per workgroup; one lane takes one row.  No sum crosses a row, so the cut changes
//     no bit.
//   * bisip_bridge_draw_dev: draws of the proposal from a Philox4x32-10 stream of their own (counter word 3 =
//     0x42520000 | pair), one lane per draw.
//   * bisip_bridge_scale_dev: a1 = exp(-(l2 - lstar)), a2 = exp(l1 - lstar), elementwise.
//   * bisip_bridge_iterate_dev: one workgroup of 256 threads per ensemble iterates r on the device; value i of a sum goes
//     to slot i mod 256, the slots are added pairwise within each wave, the four waves in ascending order.
#include <climits>

#include "chain.h"
#include "philox.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int BR_THREADS = 256;
constexpr long long BR_WGS = 2048;            // workgroups wanted of few ensembles (bisip_bridge_logg_dev)
constexpr long long BR_SEG_MIN = 1024;        // rows of a segment at least
constexpr long long BR_ONE_SEGMENT = 256;     // ensembles from which a workgroup per ensemble fills the chip
constexpr long long BR_SEG_MAX = 1LL << 30;   // rows of a segment at most: 32-bit row numbers inside it
constexpr uint32_t BR_DOMAIN = 0x42520000u;   // counter word 3 of the draws; the samplers' streams use 0, 1 and 2

struct Segments {
    long long seg_rows, nseg;
};

Segments logg_segments(long long N, long long E)
{
    Segments p{};
    if (E >= BR_ONE_SEGMENT) {
        p.seg_rows = N;
    } else {
        const long long want = BR_WGS / E;
        p.seg_rows = (N + want - 1) / want;
        if (p.seg_rows < BR_SEG_MIN) p.seg_rows = BR_SEG_MIN;
    }
    if (p.seg_rows > BR_SEG_MAX) p.seg_rows = BR_SEG_MAX;
    p.nseg = (N + p.seg_rows - 1) / p.seg_rows;
    return p;
}

// -- l = logp - log_g ------------------------------------------------------------------------------------------------------
struct LoggArgs {
    const double *chain, *logp, *mean, *chol, *cst;
    long long cstride, lstride, N, seg_rows, nseg;
    int Wp;
    double *l;                   // (E, N)
};

// z by forward substitution and m = sum z_j^2 of the row d + mu; L (NDIM, NDIM) and mu in LDS
template <int NDIM>
__device__ __forceinline__ double br_logg_row(const double *__restrict__ x, const double *__restrict__ L,
                                              const double *__restrict__ mu, double negc)
{
    double z[NDIM];
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
        double acc = __dsub_rn(x[j], mu[j]);
#pragma unroll
        for (int k = 0; k < j; ++k) acc = fma(-L[j * NDIM + k], z[k], acc);
        z[j] = __ddiv_rn(acc, L[j * NDIM + j]);
        m = fma(z[j], z[j], m);
    }
    return fma(-0.5, m, negc);
}

// grid (E * nseg): workgroup b takes segment b % nseg of ensemble b / nseg
template <int NDIM>
__global__ __launch_bounds__(BR_THREADS) void k_bridge_logg(const LoggArgs a)
{
    constexpr int T = BR_THREADS, PITCH = NDIM | 1, LOADS = NDIM;   // a tile: T * NDIM doubles, NDIM per thread
    __shared__ double s_tile[T * PITCH];
    __shared__ double s_L[NDIM * NDIM];
    __shared__ double s_mu[NDIM];

    const int tid = threadIdx.x;
    const long long e = blockIdx.x / a.nseg, g = blockIdx.x - e * a.nseg;
    const long long r0 = g * a.seg_rows;
    const int R = (int)(a.N - r0 < a.seg_rows ? a.N - r0 : a.seg_rows);
    const int Wp = a.Wp;
    const double *__restrict__ base = a.chain + e * Wp * NDIM;      // walker 0 of the ensemble in sample 0
    const double *__restrict__ lp = a.logp + e * Wp;
    if (tid < NDIM * NDIM) s_L[tid] = a.chol[e * (NDIM * NDIM) + tid];
    if (tid < NDIM) s_mu[tid] = a.mean[e * NDIM + tid];
    const double negc = -a.cst[e];

    // what this thread loads of a tile: element i = tid + m * 256 of its T * NDIM, row i / NDIM, parameter i % NDIM
    int ld_k[LOADS], ld_w[LOADS], ld_row[LOADS], ld_at[LOADS];
    double x[LOADS];
#pragma unroll
    for (int m = 0; m < LOADS; ++m) {
        const int i = tid + m * BR_THREADS, row = i / NDIM, q = i - row * NDIM;
        ld_row[m] = row;
        ld_k[m] = row / Wp;
        ld_w[m] = (row - ld_k[m] * Wp) * NDIM + q;                  // in doubles from the ensemble's walker 0
        ld_at[m] = row * PITCH + q;
    }
    // the first row of the current tile: sample kb, walker wb; this thread's own row: sample kr, walker wr
    long long kb = r0 / Wp;
    int wb = (int)(r0 - kb * Wp);
    long long kr = (r0 + tid) / Wp;
    int wr = (int)(r0 + tid - kr * Wp);
    const int step_k = T / Wp, step_w = T - step_k * Wp;

    auto load = [&](int tb) {
#pragma unroll
        for (int m = 0; m < LOADS; ++m) {
            x[m] = 0.0;
            if (ld_row[m] < R - tb) {                               // (row tb + ld_row of the segment exists)
                long long k = kb + ld_k[m];
                int w = wb * NDIM + ld_w[m];                        // < 2 Wp NDIM < 2^31: check_chain bounds Wp for this
                if (w >= Wp * NDIM) { w -= Wp * NDIM; ++k; }
                x[m] = __builtin_nontemporal_load(base + k * a.cstride + w);
            }
        }
        kb += step_k;
        wb += step_w;
        if (wb >= Wp) { wb -= Wp; ++kb; }
    };

    load(0);
    for (int tb = 0; tb < R; tb += T) {
#pragma unroll
        for (int m = 0; m < LOADS; ++m) s_tile[ld_at[m]] = x[m];
        __syncthreads();
        if (tb + T < R) load(tb + T);                               // (uniform) in flight while this tile is taken
        if (tid < R - tb) {
            const double logg = br_logg_row<NDIM>(s_tile + tid * PITCH, s_L, s_mu, negc);
            const double v = __builtin_nontemporal_load(lp + kr * a.lstride + wr);
            a.l[e * a.N + r0 + tb + tid] = __dsub_rn(v, logg);
        }
        kr += step_k;
        wr += step_w;
        if (wr >= Wp) { wr -= Wp; ++kr; }
        __syncthreads();
    }
}

// -- draws of the proposal -------------------------------------------------------------------------------------------------
struct DrawArgs {
    const double *mean, *chol, *cst;
    long long n_draws, bpe;      // blocks per ensemble
    unsigned long long seed, first_draw, first_ensemble;
    double *theta, *logg;        // (E * n_draws, ndim), (E * n_draws)
};

// grid (E * bpe): block b takes draws [(b % bpe) * 256, ...) of ensemble b / bpe, one lane per draw
template <int NDIM>
__global__ __launch_bounds__(BR_THREADS) void k_bridge_draw(const DrawArgs a)
{
    constexpr int PAIRS = (NDIM + 1) / 2;
    __shared__ double s_L[NDIM * NDIM];
    __shared__ double s_mu[NDIM];
    const int tid = threadIdx.x;
    const long long e = blockIdx.x / a.bpe;
    const long long i = (blockIdx.x - e * a.bpe) * BR_THREADS + tid;
    if (tid < NDIM * NDIM) s_L[tid] = a.chol[e * (NDIM * NDIM) + tid];
    if (tid < NDIM) s_mu[tid] = a.mean[e * NDIM + tid];
    __syncthreads();
    if (i >= a.n_draws) return;
    const unsigned long long di = a.first_draw + (unsigned long long)i;
    const uint32_t c2 = (uint32_t)(a.first_ensemble + (unsigned long long)e);
    double z[2 * PAIRS];
#pragma unroll
    for (int p = 0; p < PAIRS; ++p) {
        const Philox4 o = philox4x32_10((uint32_t)di, (uint32_t)(di >> 32), c2, BR_DOMAIN | (uint32_t)p, (uint32_t)a.seed,
                                        (uint32_t)(a.seed >> 32));
        const double u0 = u53(o.v[0], o.v[1]), u1 = u53(o.v[2], o.v[3]);
        const double rad = sqrt(__dmul_rn(-2.0, log(__dsub_rn(1.0, u0))));
        double sn, cs;
        sincospi(__dmul_rn(2.0, u1), &sn, &cs);
        z[2 * p] = __dmul_rn(rad, cs);
        z[2 * p + 1] = __dmul_rn(rad, sn);
    }
    const long long row = e * a.n_draws + i;
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
        double t = s_mu[j];
#pragma unroll
        for (int k = 0; k <= j; ++k) t = fma(s_L[j * NDIM + k], z[k], t);
        a.theta[row * NDIM + j] = t;
        m = fma(z[j], z[j], m);
    }
    a.logg[row] = fma(-0.5, m, -a.cst[e]);
}

// -- the scaled terms ------------------------------------------------------------------------------------------------------
// grid (E * bpe): dst_a = exp(+-((src - sub) - lstar[e])), dst_l = src - sub (sub, dst_l: may be null)
__global__ __launch_bounds__(BR_THREADS) void k_bridge_scale(const double *__restrict__ lstar, const double *src,
                                                             const double *sub, long long N, long long bpe, int negate,
                                                             double *dst_l, double *dst_a)
{
    const long long e = blockIdx.x / bpe;
    const long long i = (blockIdx.x - e * bpe) * BR_THREADS + threadIdx.x;
    if (i >= N) return;
    const long long at = e * N + i;
    double l = src[at];
    if (sub) l = __dsub_rn(l, sub[at]);
    if (dst_l) dst_l[at] = l;
    const double t = __dsub_rn(l, lstar[e]);
    dst_a[at] = exp(negate ? -t : t);
}

// -- the iteration ---------------------------------------------------------------------------------------------------------
struct IterArgs {
    const double *a1, *a2, *s1;
    long long N1, N2, maxiter;
    double tol;
    double *r, *moments, *f2;    // (E), (E, 4), (E, N1) or null
    long long *iterations;       // (E)
};

// the slots of a workgroup: pairwise within each wave, 32, 16, ..., 1 apart, the four waves in ascending order; every
// thread gets the sum
__device__ __forceinline__ double br_block_sum(double v, double *s_w, int tid)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = __dadd_rn(v, __shfl_xor(v, s, 64));
    if ((tid & 63) == 0) s_w[tid >> 6] = v;
    __syncthreads();
    const double t = __dadd_rn(__dadd_rn(__dadd_rn(s_w[0], s_w[1]), s_w[2]), s_w[3]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ double br_f1(double s1, double s2r, double a1)
{
    return __ddiv_rn(1.0, __dadd_rn(s1, __dmul_rn(s2r, a1)));
}

__device__ __forceinline__ double br_f2(double s1, double s2r, double a2) { return __ddiv_rn(1.0, fma(s1, a2, s2r)); }

// grid (E), 256 threads
__global__ __launch_bounds__(BR_THREADS) void k_bridge_iterate(const IterArgs a)
{
    __shared__ double s_w[4];
    const int tid = threadIdx.x;
    const long long e = blockIdx.x, N1 = a.N1, N2 = a.N2;
    const double *__restrict__ a1 = a.a1 + e * N2;
    const double *__restrict__ a2 = a.a2 + e * N1;
    const double s1 = a.s1[e], s2 = __dsub_rn(1.0, s1);
    const double n1 = (double)N1, n2 = (double)N2;
    double r = 1.0;
    long long it = 0;
    for (;;) {                                                      // (every thread holds the same r: uniform)
        const double s2r = __dmul_rn(s2, r);
        double acc = 0.0;
#pragma unroll 4
        for (long long i = tid; i < N2; i += BR_THREADS) acc = __dadd_rn(acc, br_f1(s1, s2r, a1[i]));
        const double num = __ddiv_rn(br_block_sum(acc, s_w, tid), n2);
        acc = 0.0;
#pragma unroll 4
        for (long long j = tid; j < N1; j += BR_THREADS) acc = __dadd_rn(acc, br_f2(s1, s2r, a2[j]));
        const double den = __ddiv_rn(br_block_sum(acc, s_w, tid), n1);
        const double rn = __ddiv_rn(num, den);
        ++it;
        if (!(rn > 0.0 && rn < HUGE_VAL)) {                         // sums not finite, denominator 0, numerator 0
            r = __builtin_nan("");
            break;
        }
        const bool done = fabs(__dsub_rn(rn, r)) <= __dmul_rn(a.tol, rn);
        r = rn;
        if (done || it >= a.maxiter) break;
    }
    // the terms at the final r: their means, then the centred squares
    const double s2r = __dmul_rn(s2, r);
    double acc = 0.0;
#pragma unroll 4
    for (long long i = tid; i < N2; i += BR_THREADS) acc = __dadd_rn(acc, br_f1(s1, s2r, a1[i]));
    const double m1 = __ddiv_rn(br_block_sum(acc, s_w, tid), n2);
    acc = 0.0;
#pragma unroll 4
    for (long long j = tid; j < N1; j += BR_THREADS) {
        const double f = br_f2(s1, s2r, a2[j]);
        if (a.f2) a.f2[e * N1 + j] = f;
        acc = __dadd_rn(acc, f);
    }
    const double m2 = __ddiv_rn(br_block_sum(acc, s_w, tid), n1);
    acc = 0.0;
#pragma unroll 4
    for (long long i = tid; i < N2; i += BR_THREADS) {
        const double d = __dsub_rn(br_f1(s1, s2r, a1[i]), m1);
        acc = fma(d, d, acc);
    }
    const double v1 = __ddiv_rn(br_block_sum(acc, s_w, tid), n2);
    acc = 0.0;
#pragma unroll 4
    for (long long j = tid; j < N1; j += BR_THREADS) {
        const double d = __dsub_rn(br_f2(s1, s2r, a2[j]), m2);
        acc = fma(d, d, acc);
    }
    const double v2 = __ddiv_rn(br_block_sum(acc, s_w, tid), n1);
    if (tid == 0) {
        a.r[e] = r;
        a.iterations[e] = it;
        a.moments[4 * e] = m1;
        a.moments[4 * e + 1] = v1;
        a.moments[4 * e + 2] = m2;
        a.moments[4 * e + 3] = v2;
    }
}

// -- host ------------------------------------------------------------------------------------------------------------------
// blocks of 256 for n values of one ensemble
long long blocks_per_ensemble(long long n) { return (n + BR_THREADS - 1) / BR_THREADS; }

template <int NDIM>
struct LaunchLogg {
    static void run(dim3 grid, hipStream_t st, const LoggArgs &a)
    {
        hipLaunchKernelGGL(k_bridge_logg<NDIM>, grid, dim3(BR_THREADS), 0, st, a);
    }
};

template <int NDIM>
struct LaunchDraw {
    static void run(dim3 grid, hipStream_t st, const DrawArgs &a)
    {
        hipLaunchKernelGGL(k_bridge_draw<NDIM>, grid, dim3(BR_THREADS), 0, st, a);
    }
};

template <template <int> class Launch, typename Args>
int launch_ndim(int ndim, dim3 grid, hipStream_t st, const Args &args)
{
    if (ndim == 1) {                                                // (launch_by_ndim starts at 2)
        Launch<1>::run(grid, st, args);
        HIP_TRY(hipGetLastError());
        return BISIP_OK;
    }
    return launch_by_ndim<Launch>(ndim, grid, st, args);
}

}  // namespace

extern "C" {

int bisip_bridge_logg_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, const double *d_logp, int64_t logp_stride,
                          const double *d_mean, const double *d_chol, const double *d_const, double *d_l, void *stream)
{
    if (!d_chain || !d_logp || !d_mean || !d_chol || !d_const || !d_l) return fail(BISIP_EINVAL, "null argument");
    // the caps of bisip_chain_cov_dev: the kernel walks the rows of a segment as the covariance does
    BISIP_TRY(check_chain({n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim}, 1, GRID_MAX, GRID_MAX,
                          GRID_MAX / (2 * BISIP_MAX_NDIM)));
    if (logp_stride < n_ensembles * walkers_per_ensemble) return fail(BISIP_EINVAL, "logp_stride smaller than one sample");
    const long long N = n_samples * walkers_per_ensemble;
    const Segments p = logg_segments(N, n_ensembles);
    BISIP_TRY(check_segment_grid(p.nseg, n_ensembles));
    LoggArgs a{};
    a.chain = d_chain; a.logp = d_logp; a.mean = d_mean; a.chol = d_chol; a.cst = d_const;
    a.cstride = sample_stride; a.lstride = logp_stride; a.N = N; a.seg_rows = p.seg_rows; a.nseg = p.nseg;
    a.Wp = (int)walkers_per_ensemble; a.l = d_l;
    return launch_ndim<LaunchLogg>(ndim, dim3((unsigned)(n_ensembles * p.nseg)), (hipStream_t)stream, a);
}

int bisip_bridge_draw_dev(const double *d_mean, const double *d_chol, const double *d_const, int64_t n_ensembles, int ndim,
                          int64_t n_draws, uint64_t seed, uint64_t first_draw, int64_t first_ensemble, double *d_theta,
                          double *d_logg, void *stream)
{
    if (!d_mean || !d_chol || !d_const || !d_theta || !d_logg) return fail(BISIP_EINVAL, "null argument");
    BISIP_TRY(check_ndim(ndim));
    if (n_ensembles < 1 || n_ensembles > 0x7fffffffLL || n_draws < 1 || n_draws > (1LL << 40))
        return fail(BISIP_EINVAL, "bad shape: %lld draws of %lld ensembles", (long long)n_draws, (long long)n_ensembles);
    if (first_ensemble < 0 || first_ensemble + n_ensembles > 0x100000000LL)
        return fail(BISIP_EINVAL, "ensembles %lld ... do not fit the 32-bit counter word", (long long)first_ensemble);
    if (first_draw > UINT64_MAX - (uint64_t)n_draws) return fail(BISIP_EINVAL, "first_draw + n_draws exceeds 64 bits");
    const long long bpe = blocks_per_ensemble(n_draws);
    BISIP_TRY(check_grid(bpe, n_ensembles, LOUD, "%lld draws of %lld ensembles", (long long)n_draws, (long long)n_ensembles));
    DrawArgs a{};
    a.mean = d_mean; a.chol = d_chol; a.cst = d_const; a.n_draws = n_draws; a.bpe = bpe; a.seed = seed;
    a.first_draw = first_draw; a.first_ensemble = (unsigned long long)first_ensemble; a.theta = d_theta; a.logg = d_logg;
    return launch_ndim<LaunchDraw>(ndim, dim3((unsigned)(n_ensembles * bpe)), (hipStream_t)stream, a);
}

int bisip_bridge_scale_dev(const double *d_l1, int64_t n1, const double *d_logp2, const double *d_logg2, int64_t n2,
                           int64_t n_ensembles, const double *d_lstar, double *d_l2, double *d_a1, double *d_a2, void *stream)
{
    if (!d_l1 || !d_logp2 || !d_logg2 || !d_lstar || !d_a1 || !d_a2) return fail(BISIP_EINVAL, "null argument");
    if (n_ensembles < 1 || n_ensembles > 0x7fffffffLL || n1 < 1 || n2 < 1 || n1 > (1LL << 40) || n2 > (1LL << 40))
        return fail(BISIP_EINVAL, "bad shape: %lld and %lld values of %lld ensembles", (long long)n1, (long long)n2,
                    (long long)n_ensembles);
    const long long b1 = blocks_per_ensemble(n1), b2 = blocks_per_ensemble(n2);
    BISIP_TRY(check_grid(b1 > b2 ? b1 : b2, n_ensembles, LOUD, "%lld values of %lld ensembles", (long long)(n1 > n2 ? n1 : n2),
                         (long long)n_ensembles));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bridge_scale, dim3((unsigned)(n_ensembles * b2)), dim3(BR_THREADS), 0, st, d_lstar, d_logp2, d_logg2,
                       (long long)n2, b2, 1, d_l2, d_a1);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bridge_scale, dim3((unsigned)(n_ensembles * b1)), dim3(BR_THREADS), 0, st, d_lstar, d_l1,
                       (const double *)nullptr, (long long)n1, b1, 0, (double *)nullptr, d_a2);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int bisip_bridge_iterate_dev(const double *d_a1, int64_t n2, const double *d_a2, int64_t n1, int64_t n_ensembles,
                             const double *d_s1, double tol, int64_t maxiter, double *d_r, int64_t *d_iterations,
                             double *d_moments, double *d_f2, void *stream)
{
    if (!d_a1 || !d_a2 || !d_s1 || !d_r || !d_iterations || !d_moments) return fail(BISIP_EINVAL, "null argument");
    if (n_ensembles < 1 || n_ensembles > 0x7fffffffLL || n1 < 1 || n2 < 1 || n1 > (1LL << 40) || n2 > (1LL << 40))
        return fail(BISIP_EINVAL, "bad shape: %lld and %lld values of %lld ensembles", (long long)n1, (long long)n2,
                    (long long)n_ensembles);
    if (!(tol >= 0.0) || maxiter < 1) return fail(BISIP_EINVAL, "tol must be >= 0 and maxiter >= 1");
    IterArgs a{};
    a.a1 = d_a1; a.a2 = d_a2; a.s1 = d_s1; a.N1 = n1; a.N2 = n2; a.maxiter = maxiter; a.tol = tol;
    a.r = d_r; a.moments = d_moments; a.f2 = d_f2; a.iterations = (long long *)d_iterations;
    hipLaunchKernelGGL(k_bridge_iterate, dim3((unsigned)n_ensembles), dim3(BR_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

}  // extern "C"
