// chain_rhat.hip -- per-walker moments and the Gelman-Rubin potential scale reduction of a device-resident chain
// (bisip_chain_rhat_dev): the chain reduced along the STEP axis per walker, which nothing else here does.  The
// definitions are bisip_amd/convergence.py (walker_moments, gelman_rubin); convergence.ordered_rhat restates the order
// of every sum below in NumPy and gives the same bits.
//
// A half is the whole series (splits = 1, L = n) or its first and last L = n / 2 samples (splits = 2: half 0 is samples
// [0, L), half 1 is [n - L, n); the middle sample of an odd n is in neither).  A column j in [0, C), C = E * Wp * ndim, is
// one (ensemble, walker, parameter); consecutive lanes own consecutive columns, so a wave reads 512 contiguous bytes
// of every sample.  The chain is read once.
//
//   * Shifted sums.  c = the column's first sample of the half.  For every sample of the half, in ascending order,
//     d = x - c, S1 = S1 + d, S2 = S2 + d * d, both from 0.0; the product is rounded on its own (no fma).
//   * Segments.  rh_plan() cuts the L samples of a half into nseg segments of seg_len samples (the last one shorter):
//         want = max(1, 262144 / (splits * 256 * ceil(C / 256)));  seg_len = max(32, ceil(L / want));
//         nseg = ceil(L / seg_len)
//     -- a function of the shape alone.  Segment g sums its samples [g * seg_len, min(L, (g + 1) * seg_len)) as above, each
//     from 0.0 with the SAME shift c, and a column's segments are merged in ascending order: S = (...((s_0 + s_1) + s_2)
//     ...).  Eight samples of a lane are loaded before the first is added.
//   * mean = c + S1 / L;  var = (S2 - (S1 * S1) / L) / (L - 1), set to 0 where it is < 0 (a NaN stays).
//   * R-hat of (ensemble, parameter): the M = splits * Wp chains are numbered c = half * Wp + w.  m0 = the mean of
//     chain 0.  Chain c goes to partial c mod 64, in ascending c, each partial from 0.0:  V += var_c;  dm = mean_c - m0;
//     T1 += dm;  T2 += dm * dm (product rounded on its own).  The 64 partials of V, T1 and T2 are added pairwise 32, 16,
//     ..., 1 apart.  Wn = V / M;  Bn = (T2 - (T1 * T1) / M) / (M - 1), 0 where < 0;  rhat = sqrt((L - 1) / L + Bn / Wn)
//     with IEEE division and square root: NaN for 0 / 0, inf when only Wn is 0.
//
// Kernels.  Many small ensembles whose halves need one segment (E >= 256, splits * Wp * ndim <= 4096) take ONE kernel, a
// workgroup per ensemble that keeps the chain moments in LDS: no workspace.  Everything else: k_rhat_accumulate (a lane
// per (half, segment, column); with one segment it finishes the moments itself), k_rhat_merge when there are several
// segments, k_rhat_stage (a workgroup per ensemble, a wave per parameter).  The arithmetic is the same functions in both.
#include "chain.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int RH_THREADS = 256;
constexpr long long RH_LANES = 262144;        // lanes wanted before a half is cut into more segments
constexpr long long RH_SEG_MIN = 32;          // samples of a segment at least
constexpr long long RH_FUSED_ITEMS = 4096;    // splits * Wp * ndim whose means and variances fit 64 KiB of LDS
constexpr long long RH_FUSED_ENSEMBLES = 256; // a workgroup per ensemble fills the chip from here on

struct RhatPlan {
    long long L, start1, C, seg_len, nseg;
    bool fused;
};

RhatPlan rh_plan(long long n, long long E, long long Wp, int ndim, int splits)
{
    RhatPlan p{};
    p.L = splits == 2 ? n / 2 : n;
    p.start1 = n - p.L;
    p.C = E * Wp * ndim;
    const long long tiles = (p.C + RH_THREADS - 1) / RH_THREADS;
    long long want = RH_LANES / (splits * RH_THREADS * tiles);
    if (want < 1) want = 1;
    p.seg_len = (p.L + want - 1) / want;
    if (p.seg_len < RH_SEG_MIN) p.seg_len = RH_SEG_MIN;
    p.nseg = (p.L + p.seg_len - 1) / p.seg_len;
    p.fused = p.nseg == 1 && E >= RH_FUSED_ENSEMBLES && splits * Wp * ndim <= RH_FUSED_ITEMS;
    return p;
}

struct RhatArgs {
    const double *chain;
    long long stride, E, C, L, start1, seg_len, nseg;
    int Wp, ndim, splits;
    double *part;                // (2, splits, nseg, C): S1 then S2 of every segment (nseg > 1)
    double *mean, *var;          // (splits, C) each: the caller's or the workspace's; null: not stored
    double *rhat;                // (E, ndim) or null
};

// the shifted sums of samples [k0, k1) of a half whose first sample is at col
__device__ __forceinline__ void rh_sums(const double *__restrict__ col, long long stride, double c, long long k0,
                                        long long k1, double &S1, double &S2)
{
    double s1 = 0.0, s2 = 0.0;
    long long k = k0;
    for (; k + 8 <= k1; k += 8) {
        double x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = __builtin_nontemporal_load(col + (k + r) * stride);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const double d = __dsub_rn(x[r], c);
            s1 = __dadd_rn(s1, d);
            s2 = __dadd_rn(s2, __dmul_rn(d, d));
        }
    }
    for (; k < k1; ++k) {
        const double d = __dsub_rn(__builtin_nontemporal_load(col + k * stride), c);
        s1 = __dadd_rn(s1, d);
        s2 = __dadd_rn(s2, __dmul_rn(d, d));
    }
    S1 = s1;
    S2 = s2;
}

// (T2 - T1 * T1 / n) / (n - 1), 0 where negative; a NaN fails the comparison and stays
__device__ __forceinline__ double rh_variance(double T1, double T2, long long n)
{
    const double v = __ddiv_rn(__dsub_rn(T2, __ddiv_rn(__dmul_rn(T1, T1), (double)n)), (double)(n - 1));
    return v < 0.0 ? 0.0 : v;
}

__device__ __forceinline__ double rh_mean(double c, double S1, long long L) { return __dadd_rn(c, __ddiv_rn(S1, (double)L)); }

// R-hat of one (ensemble, parameter) by one wave; fm(c), fv(c): mean and variance of chain c
template <typename FM, typename FV>
__device__ __forceinline__ double rh_stage(int lane, long long M, long long L, FM &&fm, FV &&fv)
{
    const double m0 = fm(0);
    double V = 0.0, T1 = 0.0, T2 = 0.0;
    for (long long c = lane; c < M; c += 64) {
        const double dm = __dsub_rn(fm(c), m0);
        V = __dadd_rn(V, fv(c));
        T1 = __dadd_rn(T1, dm);
        T2 = __dadd_rn(T2, __dmul_rn(dm, dm));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        V = __dadd_rn(V, __shfl_xor(V, d, 64));
        T1 = __dadd_rn(T1, __shfl_xor(T1, d, 64));
        T2 = __dadd_rn(T2, __shfl_xor(T2, d, 64));
    }
    const double Wn = __ddiv_rn(V, (double)M), Bn = rh_variance(T1, T2, M);
    return __dsqrt_rn(__dadd_rn(__ddiv_rn((double)(L - 1), (double)L), __ddiv_rn(Bn, Wn)));
}

// grid (column tiles, segments, halves)
__global__ __launch_bounds__(RH_THREADS) void k_rhat_accumulate(const RhatArgs a)
{
    const long long j = (long long)blockIdx.x * RH_THREADS + threadIdx.x;
    if (j >= a.C) return;
    const long long g = blockIdx.y, half = blockIdx.z;
    const double *__restrict__ col = a.chain + (half ? a.start1 : 0) * a.stride + j;
    const double c = col[0];
    const long long k0 = g * a.seg_len, k1 = k0 + a.seg_len < a.L ? k0 + a.seg_len : a.L;
    double S1, S2;
    rh_sums(col, a.stride, c, k0, k1, S1, S2);
    if (a.nseg > 1) {                                           // (uniform)
        const long long at = (half * a.nseg + g) * a.C + j;
        a.part[at] = S1;
        a.part[a.splits * a.nseg * a.C + at] = S2;
        return;
    }
    if (a.mean) a.mean[half * a.C + j] = rh_mean(c, S1, a.L);
    if (a.var) a.var[half * a.C + j] = rh_variance(S1, S2, a.L);
}

// grid (column tiles, 1, halves): the segments of a column in ascending order
__global__ __launch_bounds__(RH_THREADS) void k_rhat_merge(const RhatArgs a)
{
    const long long j = (long long)blockIdx.x * RH_THREADS + threadIdx.x;
    if (j >= a.C) return;
    const long long half = blockIdx.z;
    const double *__restrict__ p1 = a.part + half * a.nseg * a.C + j;
    const double *__restrict__ p2 = p1 + a.splits * a.nseg * a.C;
    double S1 = p1[0], S2 = p2[0];
    for (long long g = 1; g < a.nseg; ++g) {
        S1 = __dadd_rn(S1, p1[g * a.C]);
        S2 = __dadd_rn(S2, p2[g * a.C]);
    }
    const double c = a.chain[(half ? a.start1 : 0) * a.stride + j];
    if (a.mean) a.mean[half * a.C + j] = rh_mean(c, S1, a.L);
    if (a.var) a.var[half * a.C + j] = rh_variance(S1, S2, a.L);
}

// a workgroup per ensemble, wave q takes parameter q (64 * ndim threads)
__global__ __launch_bounds__(64 * BISIP_MAX_NDIM) void k_rhat_stage(const RhatArgs a)
{
    const long long e = blockIdx.x;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long Wp = a.Wp, M = a.splits * Wp;
    auto at = [&](long long c) { const long long half = c / Wp, w = c - half * Wp; return half * a.C + (e * Wp + w) * a.ndim + q; };
    const double r = rh_stage(lane, M, a.L, [&](long long c) { return a.mean[at(c)]; }, [&](long long c) { return a.var[at(c)]; });
    if (lane == 0) a.rhat[e * a.ndim + q] = r;
}

// a workgroup per ensemble: its splits * Wp * ndim chain moments stay in LDS (one segment per half)
__global__ __launch_bounds__(1024) void k_rhat_fused(const RhatArgs a)
{
    extern __shared__ double s_mv[];                            // mean (items), var (items)
    const long long e = blockIdx.x;
    const int per = a.Wp * a.ndim, items = a.splits * per;
    for (int i = threadIdx.x; i < items; i += blockDim.x) {
        const int half = i / per, jj = i - half * per;
        const long long j = e * per + jj;
        const double *__restrict__ col = a.chain + (half ? a.start1 : 0) * a.stride + j;
        const double c = col[0];
        double S1, S2;
        rh_sums(col, a.stride, c, 0, a.L, S1, S2);
        const double m = rh_mean(c, S1, a.L), v = rh_variance(S1, S2, a.L);
        s_mv[i] = m;
        s_mv[items + i] = v;
        if (a.mean) a.mean[half * a.C + j] = m;
        if (a.var) a.var[half * a.C + j] = v;
    }
    if (!a.rhat) return;                                        // (uniform)
    __syncthreads();
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    if (q >= a.ndim) return;                                    // (whole waves)
    const double r = rh_stage(lane, a.splits * (long long)a.Wp, a.L, [&](long long c) { return s_mv[c * a.ndim + q]; },
                              [&](long long c) { return s_mv[items + c * a.ndim + q]; });
    if (lane == 0) a.rhat[e * a.ndim + q] = r;
}

// E: grid dimension x of the fused and the R-hat kernels; Wp: Wp * ndim and splits * Wp * ndim are ints in the kernels
// (2 * BISIP_MAX_NDIM columns per walker at most).  n has a rule of its own, which comes after the counts.
int check_rhat_shape(const ChainShape &s, int splits, Voice v)
{
    BISIP_TRY(check_ndim(s.ndim, 1, v));
    if (splits != 1 && splits != 2) return refuse(v, BISIP_EINVAL, "splits=%d: 1 or 2", splits);
    BISIP_TRY(check_counts({1, 0, s.E, s.Wp, s.ndim}, NO_CAP, GRID_MAX, GRID_MAX / (2 * BISIP_MAX_NDIM), v));
    if (s.n < 2 * splits) return refuse(v, BISIP_EINVAL, "n_samples=%lld: a chain needs 2 samples, a half too", (long long)s.n);
    if (splits * s.Wp < 2) return refuse(v, BISIP_EINVAL, "R-hat needs 2 chains");
    return BISIP_OK;
}

}  // namespace

extern "C" {

int64_t bisip_chain_rhat_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, int splits)
{
    if (check_rhat_shape({n_samples, 0, n_ensembles, walkers_per_ensemble, ndim}, splits, QUIET) != BISIP_OK) return -1;
    const RhatPlan p = rh_plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits);
    if ((p.C + RH_THREADS - 1) / RH_THREADS > 0x7fffffffLL) return -1;
    if (p.fused) return 0;
    // the segments' sums, and the chain moments for the R-hat stage when the caller does not take them
    return 8 * (2 * splits * p.C + (p.nseg > 1 ? 2 * splits * p.nseg * p.C : 0));
}

int bisip_chain_rhat_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                         int64_t walkers_per_ensemble, int ndim, int splits, double *d_mean, double *d_var, double *d_rhat,
                         void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_chain) return fail(BISIP_EINVAL, "null argument");
    if (!d_mean && !d_var && !d_rhat) return fail(BISIP_EINVAL, "none of mean, variance and R-hat asked for");
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_rhat_shape(s, splits, LOUD));
    BISIP_TRY(check_stride(s));
    const RhatPlan p = rh_plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits);
    const long long tiles = (p.C + RH_THREADS - 1) / RH_THREADS;
    BISIP_TRY(check_grid(tiles, 1, LOUD, "%lld columns", p.C));
    hipStream_t st = (hipStream_t)stream;
    RhatArgs a{};
    a.chain = d_chain; a.stride = sample_stride; a.E = n_ensembles; a.C = p.C; a.L = p.L; a.start1 = p.start1;
    a.seg_len = p.seg_len; a.nseg = p.nseg; a.Wp = (int)walkers_per_ensemble; a.ndim = ndim; a.splits = splits;
    a.mean = d_mean; a.var = d_var; a.rhat = d_rhat;

    if (p.fused) {
        const int items = splits * a.Wp * ndim, need = items > 64 * ndim ? items : 64 * ndim;
        const int threads = need >= 1024 ? 1024 : (need + 63) / 64 * 64;
        hipLaunchKernelGGL(k_rhat_fused, dim3((unsigned)n_ensembles), dim3(threads), (size_t)items * 16, st, a);
        HIP_TRY(hipGetLastError());
        return BISIP_OK;
    }

    BISIP_TRY(check_workspace(d_work, work_bytes, bisip_chain_rhat_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits)));
    double *w = (double *)d_work;
    if (d_rhat) {                                 // the R-hat stage reads the moments of every chain
        if (!a.mean) a.mean = w;
        if (!a.var) a.var = w + splits * p.C;
    }
    a.part = w + 2 * splits * p.C;
    hipLaunchKernelGGL(k_rhat_accumulate, dim3((unsigned)tiles, (unsigned)p.nseg, (unsigned)splits), dim3(RH_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (p.nseg > 1) {
        hipLaunchKernelGGL(k_rhat_merge, dim3((unsigned)tiles, 1, (unsigned)splits), dim3(RH_THREADS), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    if (d_rhat) {
        hipLaunchKernelGGL(k_rhat_stage, dim3((unsigned)n_ensembles), dim3(64 * ndim), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

}  // extern "C"
