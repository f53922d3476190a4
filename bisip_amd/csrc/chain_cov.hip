// chain_cov.hip -- the posterior covariance of every ensemble's used samples (bisip_chain_cov_dev) and the stored sample
// of largest log-probability (bisip_chain_best_sample_dev) of a device-resident chain.  The definitions are
// bisip_amd/covariance.py (flat_cov, best_sample); covariance.ordered_cov restates the order of every sum below in NumPy
// and gives the same bits.
//
// Rows.  Ensemble e owns N = n_samples * Wp rows of ndim doubles, numbered r = k * Wp + w (sample k, walker w): the order
// of get_chain(flat=True).  Both kernels cut the rows, not the samples, so that one ensemble of a million walkers and a
// few samples fills the chip as well as one of 32 walkers and 5000 samples.
//
// Covariance.
//   * Plan (cv_plan; covariance.plan): n_ensembles >= 256 -> one segment of N rows per ensemble, ONE kernel, no
//     workspace.  Else want = 2048 / n_ensembles, seg_rows = max(1024, ceil(N / want)), nseg = ceil(N / seg_rows).  (A
//     segment never exceeds 2^30 rows.)  A function of the shape alone.
//   * A workgroup of 256 threads takes one (ensemble, segment).  T = 256 row slots for ndim <= 8, T = 64 for ndim 9 ... 16
//     where the four waves share the triangle: wave q keeps the rows j = q, q + 4, q + 8, q + 12 of it (S_j and P_jk,
//     k >= j), 44 running sums at most, as one lane keeps all 8 + 36 at ndim 8.  The kernel is instantiated on ndim.
//   * Shifted sums.  c_j = parameter j of walker 0 of the ensemble's first used sample, the same in every segment.
//     d = x - c.  Row i of a segment (i from 0) goes to slot i mod T; a slot takes its rows in ascending order, each sum
//     from 0.0:  S_j = S_j + d_j;  P_jk = P_jk + d_j * d_k, the product rounded on its own (no fma).
//   * The T slots of a sum are added pairwise within each wave of 64 slots, 32, 16, ..., 1 apart; for T = 256 the four
//     waves' results are then added in ascending order ((w0 + w1) + w2) + w3.
//   * Segments are merged in ascending order S = (...((s_0 + s_1) + s_2) ...) by k_cov_merge (nseg > 1).
//   * mean_j = c_j + S_j / N;  cov_jk = (P_jk - (S_j * S_k) / N) / (N - 1) for j <= k, stored at [j, k] and [k, j]; a
//     diagonal entry < 0 becomes 0 (a NaN stays).
//   * Access.  A tile of T rows is T * ndim contiguous doubles wherever it lies inside a sample (a tile that crosses
//     samples is a few such runs): consecutive threads load consecutive doubles -- whole 128-byte lines per wave
//     instruction -- subtract c and store d to LDS with a row pitch of ndim | 1 doubles (odd: ds_read_b64 of one column by
//     64 rows touches every bank pair once).  The next tile's loads are in flight while this tile is summed.
//
// Best sample.  key (value with NaN read as -inf, index); a beats b when its value is larger, or equal with the lower
// index -- exact, so any order gives the same answer.  bs_plan: n_ensembles >= 256 -> one segment; else seg_rows =
// max(4096, ceil(N / (2048 / n_ensembles))).  k_best_scan: a workgroup per (ensemble, segment), thread t takes rows t,
// t + 256, ...; k_best_merge: a wave per ensemble over the segments' keys.  The winner's stored log-probability and its
// ndim doubles are copied as they are.
#include <climits>

#include "chain.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int CV_THREADS = 256;
constexpr long long CV_WGS = 2048;            // workgroups wanted of few ensembles
constexpr long long CV_SEG_MIN = 1024;        // rows of a covariance segment at least
constexpr long long BS_SEG_MIN = 4096;        // rows of a best-sample segment at least
constexpr long long CV_ONE_SEGMENT = 256;     // ensembles from which a workgroup per ensemble fills the chip
constexpr long long CV_SEG_MAX = 1LL << 30;   // rows of a segment at most: 32-bit row numbers inside it

struct RowPlan {
    long long N, seg_rows, nseg;
};

RowPlan row_plan(long long n, long long E, long long Wp, long long seg_min)
{
    RowPlan p{};
    p.N = n * Wp;
    if (E >= CV_ONE_SEGMENT) {
        p.seg_rows = p.N;
    } else {
        const long long want = CV_WGS / E;
        p.seg_rows = (p.N + want - 1) / want;
        if (p.seg_rows < seg_min) p.seg_rows = seg_min;
    }
    if (p.seg_rows > CV_SEG_MAX) p.seg_rows = CV_SEG_MAX;
    p.nseg = (p.N + p.seg_rows - 1) / p.seg_rows;
    return p;
}

RowPlan cv_plan(long long n, long long E, long long Wp) { return row_plan(n, E, Wp, CV_SEG_MIN); }
RowPlan bs_plan(long long n, long long E, long long Wp) { return row_plan(n, E, Wp, BS_SEG_MIN); }

struct CovArgs {
    const double *chain;
    long long stride, N, seg_rows, nseg;
    int Wp, ndim;
    double *mean, *cov;          // (E, ndim), (E, ndim, ndim); mean may be null
    double *part;                // (E, nseg, ndim + ndim (ndim + 1) / 2): S then P row by row (nseg > 1)
};

__host__ __device__ constexpr int cv_sums(int ndim) { return ndim + ndim * (ndim + 1) / 2; }
// where P_jk (j <= k) lies among the sums of one segment
__host__ __device__ constexpr int cv_at(int ndim, int j, int k) { return ndim + j * ndim - j * (j - 1) / 2 + (k - j); }

template <int NDIM>
struct CovShape {
    static constexpr int GROUPS = NDIM > 8 ? 4 : 1;                 // waves that share the triangle
    static constexpr int T = CV_THREADS / GROUPS;                  // row slots = rows of a tile
    static constexpr int PITCH = NDIM | 1;
    static constexpr int LOADS = (T * NDIM + CV_THREADS - 1) / CV_THREADS;
    static constexpr int JROWS = (NDIM + GROUPS - 1) / GROUPS;      // triangle rows of group 0, which has the most
    static constexpr int NACC = GROUPS == 1 ? cv_sums(NDIM) : JROWS + JROWS * NDIM - GROUPS * JROWS * (JROWS - 1) / 2;
};

// one row into the sums of group Q: triangle rows j = Q, Q + GROUPS, ...
template <int NDIM, int Q>
__device__ __forceinline__ void cv_row(const double *__restrict__ srow, double *acc)
{
    constexpr int G = CovShape<NDIM>::GROUPS;
    double d[NDIM];
#pragma unroll
    for (int k = Q; k < NDIM; ++k) d[k] = srow[k];
    int a = 0;
#pragma unroll
    for (int j = Q; j < NDIM; j += G) {
        acc[a] = __dadd_rn(acc[a], d[j]);
        ++a;
#pragma unroll
        for (int k = j; k < NDIM; ++k) {
            acc[a] = __dadd_rn(acc[a], __dmul_rn(d[j], d[k]));
            ++a;
        }
    }
}

// the 64 slots of a wave added pairwise; lane 0 stores group Q's sums where cv_at() says
template <int NDIM, int Q>
__device__ __forceinline__ void cv_flush(double *acc, int lane, double *__restrict__ dst)
{
    constexpr int G = CovShape<NDIM>::GROUPS;
    int a = 0;
#pragma unroll
    for (int j = Q; j < NDIM; j += G) {
#pragma unroll
        for (int k = j - 1; k < NDIM; ++k) {                        // k = j - 1 stands for S_j
            double v = acc[a++];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v = __dadd_rn(v, __shfl_xor(v, s, 64));
            if (lane == 0) dst[k < j ? j : cv_at(NDIM, j, k)] = v;
        }
    }
}

// entry [j, k] of the covariance from the sums of the whole ensemble
__device__ __forceinline__ double cv_entry(double Sa, double Sb, double P, long long N, bool diagonal)
{
    const double v = __ddiv_rn(__dsub_rn(P, __ddiv_rn(__dmul_rn(Sa, Sb), (double)N)), (double)(N - 1));
    return diagonal && v < 0.0 ? 0.0 : v;                           // (a NaN fails the comparison and stays)
}

// thread t finishes entry t of (ndim, ndim) and, t < ndim, the mean; S, P: the ensemble's sums as cv_at() orders them
__device__ __forceinline__ void cv_finish(const CovArgs &a, long long e, int t, const double *sums, const double *c)
{
    const int ndim = a.ndim;
    if (t < ndim * ndim) {
        const int j = t / ndim, k = t - j * ndim, lo = j < k ? j : k, hi = j < k ? k : j;
        a.cov[(e * ndim + j) * ndim + k] = cv_entry(sums[lo], sums[hi], sums[cv_at(ndim, lo, hi)], a.N, j == k);
    }
    if (a.mean && t < ndim) a.mean[e * ndim + t] = __dadd_rn(c[t], __ddiv_rn(sums[t], (double)a.N));
}

// grid (E * nseg): workgroup b takes segment b % nseg of ensemble b / nseg
template <int NDIM>
__global__ __launch_bounds__(CV_THREADS) void k_cov_accumulate(const CovArgs a)
{
    using SH = CovShape<NDIM>;
    constexpr int T = SH::T, PITCH = SH::PITCH, LOADS = SH::LOADS, NS = cv_sums(NDIM);
    __shared__ double s_tile[T * PITCH];
    __shared__ double s_c[NDIM];
    __shared__ double s_wave[SH::GROUPS == 1 ? 4 * NS : 1];
    __shared__ double s_sum[NS];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long e = blockIdx.x / a.nseg, g = blockIdx.x - e * a.nseg;
    const long long r0 = g * a.seg_rows;
    const int R = (int)(a.N - r0 < a.seg_rows ? a.N - r0 : a.seg_rows);
    const int Wp = a.Wp;
    const double *__restrict__ base = a.chain + e * Wp * NDIM;      // walker 0 of the ensemble in sample 0
    if (tid < NDIM) s_c[tid] = base[tid];
    __syncthreads();

    // what this thread loads of a tile: element i = tid + m * 256 of its T * NDIM, row i / NDIM, parameter i % NDIM
    int ld_k[LOADS], ld_w[LOADS], ld_row[LOADS], ld_at[LOADS];
    double ld_c[LOADS], x[LOADS];
#pragma unroll
    for (int m = 0; m < LOADS; ++m) {
        const int i = tid + m * CV_THREADS, row = i / NDIM, q = i - row * NDIM;
        ld_row[m] = i < T * NDIM ? row : INT_MAX;                   // (no such element: never inside the segment)
        ld_k[m] = row / Wp;
        ld_w[m] = row - ld_k[m] * Wp;
        ld_at[m] = row * PITCH + q;
        ld_c[m] = s_c[q];
        ld_w[m] = ld_w[m] * NDIM + q;                               // in doubles from the ensemble's walker 0
    }
    // the first row of the current tile: sample kb, walker wb
    long long kb = r0 / Wp;
    int wb = (int)(r0 - kb * Wp);
    const int step_k = T / Wp, step_w = T - step_k * Wp;

    auto load = [&](int tb) {
#pragma unroll
        for (int m = 0; m < LOADS; ++m) {
            x[m] = 0.0;
            if (ld_row[m] < R - tb) {                               // (row tb + ld_row of the segment exists)
                long long k = kb + ld_k[m];
                int w = wb * NDIM + ld_w[m];                        // < 2 Wp NDIM < 2^31: check_rows_shape bounds Wp for this
                if (w >= Wp * NDIM) { w -= Wp * NDIM; ++k; }
                x[m] = __builtin_nontemporal_load(base + k * a.stride + w);
            }
        }
        kb += step_k;
        wb += step_w;
        if (wb >= Wp) { wb -= Wp; ++kb; }
    };

    double acc[SH::NACC];
#pragma unroll
    for (int i = 0; i < SH::NACC; ++i) acc[i] = 0.0;
    const int slot = SH::GROUPS == 1 ? tid : lane;

    load(0);
    for (int tb = 0; tb < R; tb += T) {
#pragma unroll
        for (int m = 0; m < LOADS; ++m)
            if (ld_row[m] != INT_MAX) s_tile[ld_at[m]] = __dsub_rn(x[m], ld_c[m]);
        __syncthreads();
        if (tb + T < R) load(tb + T);                               // (uniform) in flight while this tile is summed
        if (slot < R - tb) {
            const double *srow = s_tile + slot * PITCH;
            if constexpr (SH::GROUPS == 1) {
                cv_row<NDIM, 0>(srow, acc);
            } else {
                switch (wave) {                                     // (uniform)
                case 0: cv_row<NDIM, 0>(srow, acc); break;
                case 1: cv_row<NDIM, 1>(srow, acc); break;
                case 2: cv_row<NDIM, 2>(srow, acc); break;
                default: cv_row<NDIM, 3>(srow, acc); break;
                }
            }
        }
        __syncthreads();
    }

    if constexpr (SH::GROUPS == 1) {
        cv_flush<NDIM, 0>(acc, lane, s_wave + wave * NS);
        __syncthreads();
        if (tid < NS)
            s_sum[tid] = __dadd_rn(__dadd_rn(__dadd_rn(s_wave[tid], s_wave[NS + tid]), s_wave[2 * NS + tid]), s_wave[3 * NS + tid]);
    } else {
        switch (wave) {
        case 0: cv_flush<NDIM, 0>(acc, lane, s_sum); break;
        case 1: cv_flush<NDIM, 1>(acc, lane, s_sum); break;
        case 2: cv_flush<NDIM, 2>(acc, lane, s_sum); break;
        default: cv_flush<NDIM, 3>(acc, lane, s_sum); break;
        }
    }
    __syncthreads();
    if (a.nseg > 1) {                                               // (uniform)
        if (tid < NS) a.part[(e * a.nseg + g) * NS + tid] = s_sum[tid];
        return;
    }
    cv_finish(a, e, tid, s_sum, s_c);
}

// grid (E), 256 threads: thread t adds the sums that entry t needs over the segments in ascending order
__global__ __launch_bounds__(CV_THREADS) void k_cov_merge(const CovArgs a)
{
    const long long e = blockIdx.x;
    const int t = threadIdx.x, ndim = a.ndim, NS = cv_sums(ndim);
    if (t >= ndim * ndim) return;
    const int j = t / ndim, k = t - j * ndim, lo = j < k ? j : k, hi = j < k ? k : j, at = cv_at(ndim, lo, hi);
    const double *__restrict__ p = a.part + e * a.nseg * NS;
    double Sa = p[lo], Sb = p[hi], P = p[at];
    for (long long g = 1; g < a.nseg; ++g) {
        Sa = __dadd_rn(Sa, p[g * NS + lo]);
        Sb = __dadd_rn(Sb, p[g * NS + hi]);
        P = __dadd_rn(P, p[g * NS + at]);
    }
    a.cov[(e * ndim + j) * ndim + k] = cv_entry(Sa, Sb, P, a.N, j == k);
    if (a.mean && j == k) a.mean[e * ndim + j] = __dadd_rn(a.chain[e * a.Wp * ndim + j], __ddiv_rn(Sa, (double)a.N));
}

template <int NDIM>
void cv_launch(const CovArgs &a, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL(k_cov_accumulate<NDIM>, dim3(blocks), dim3(CV_THREADS), 0, st, a);
}

// n, E: 32 bits; Wp: the kernel's element numbers within a sample reach 2 * Wp * ndim and are ints (w in its load)
int check_rows_shape(const ChainShape &s, Voice v)
{
    return check_counts(s, GRID_MAX, GRID_MAX, GRID_MAX / (2 * BISIP_MAX_NDIM), v);
}

int check_cov_shape(const ChainShape &s, Voice v)
{
    BISIP_TRY(check_ndim(s.ndim, 1, v));
    BISIP_TRY(check_rows_shape(s, v));
    if (s.n * s.Wp < 2)
        return refuse(v, BISIP_EINVAL, "a covariance needs 2 rows, got n_samples * walkers_per_ensemble = %lld", (long long)(s.n * s.Wp));
    return BISIP_OK;
}

// -- best sample ---------------------------------------------------------------------------------------------------------
struct BestArgs {
    const double *chain, *logp;
    long long cstride, lstride, N, seg_rows, nseg;
    int Wp, ndim;
    double *theta, *best;        // (E, ndim), (E)
    long long *index;            // (E)
    double *pval;                // (E, nseg) keys of the segments (nseg > 1)
    long long *pidx;
};

__device__ __forceinline__ bool bs_better(double v, long long i, double bv, long long bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ void bs_wave(double &v, long long &i)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s, 64);
        const long long oi = __shfl_xor(i, s, 64);
        if (bs_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// threads t < max(ndim, 1) of a workgroup: the outputs of ensemble e whose best row is idx
__device__ __forceinline__ void bs_finish(const BestArgs &a, long long e, int t, long long idx)
{
    const long long k = idx / a.Wp, w = e * a.Wp + (idx - k * a.Wp);
    if (t == 0) {
        if (a.index) a.index[e] = idx;
        if (a.best) a.best[e] = a.logp[k * a.lstride + w];
    }
    if (a.theta && t < a.ndim) a.theta[e * a.ndim + t] = a.chain[k * a.cstride + w * a.ndim + t];
}

// grid (E * nseg)
__global__ __launch_bounds__(CV_THREADS) void k_best_scan(const BestArgs a)
{
    __shared__ double s_v[4];
    __shared__ long long s_i[4];
    const int tid = threadIdx.x, Wp = a.Wp;
    const long long e = blockIdx.x / a.nseg, g = blockIdx.x - e * a.nseg;
    const long long r0 = g * a.seg_rows;
    const int R = (int)(a.N - r0 < a.seg_rows ? a.N - r0 : a.seg_rows);
    const double *__restrict__ lp = a.logp + e * Wp;
    long long k = (r0 + tid) / Wp;
    int w = (int)(r0 + tid - k * Wp);
    const int step_k = CV_THREADS / Wp, step_w = CV_THREADS - step_k * Wp;
    double bv = -HUGE_VAL;
    long long bi = LLONG_MAX;
#pragma unroll 4
    for (int r = tid; r < R; r += CV_THREADS) {
        double v = __builtin_nontemporal_load(lp + k * a.lstride + w);
        if (v != v) v = -HUGE_VAL;
        if (bs_better(v, r0 + r, bv, bi)) { bv = v; bi = r0 + r; }
        k += step_k;
        w += step_w;
        if (w >= Wp) { w -= Wp; ++k; }
    }
    bs_wave(bv, bi);
    if ((tid & 63) == 0) { s_v[tid >> 6] = bv; s_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; ++q)
            if (bs_better(s_v[q], s_i[q], bv, bi)) { bv = s_v[q]; bi = s_i[q]; }
        s_i[0] = bi;
        if (a.nseg > 1) { a.pval[e * a.nseg + g] = bv; a.pidx[e * a.nseg + g] = bi; }
    }
    if (a.nseg > 1) return;                                         // (uniform)
    __syncthreads();
    bs_finish(a, e, tid, s_i[0]);
}

// grid (E), one wave
__global__ __launch_bounds__(64) void k_best_merge(const BestArgs a)
{
    const long long e = blockIdx.x;
    const int lane = threadIdx.x;
    double bv = -HUGE_VAL;
    long long bi = LLONG_MAX;
    for (long long g = lane; g < a.nseg; g += 64) {
        const double v = a.pval[e * a.nseg + g];
        const long long i = a.pidx[e * a.nseg + g];
        if (bs_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    bs_wave(bv, bi);
    bs_finish(a, e, lane, bi);
}

}  // namespace

extern "C" {

int64_t bisip_chain_cov_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim)
{
    if (check_cov_shape({n_samples, 0, n_ensembles, walkers_per_ensemble, ndim}, QUIET) != BISIP_OK) return -1;
    const RowPlan p = cv_plan(n_samples, n_ensembles, walkers_per_ensemble);
    if (check_segment_grid(p.nseg, n_ensembles, QUIET) != BISIP_OK) return -1;
    return p.nseg > 1 ? 8 * n_ensembles * p.nseg * cv_sums(ndim) : 0;
}

int bisip_chain_cov_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                        int64_t walkers_per_ensemble, int ndim, double *d_mean, double *d_cov, void *d_work,
                        int64_t work_bytes, void *stream)
{
    if (!d_chain || !d_cov) return fail(BISIP_EINVAL, "null argument");
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_cov_shape(s, LOUD));
    BISIP_TRY(check_stride(s));
    const RowPlan p = cv_plan(n_samples, n_ensembles, walkers_per_ensemble);
    BISIP_TRY(check_segment_grid(p.nseg, n_ensembles));
    BISIP_TRY(check_workspace(d_work, work_bytes, p.nseg > 1 ? 8 * n_ensembles * p.nseg * cv_sums(ndim) : 0));
    hipStream_t st = (hipStream_t)stream;
    CovArgs a{};
    a.chain = d_chain; a.stride = sample_stride; a.N = p.N; a.seg_rows = p.seg_rows; a.nseg = p.nseg;
    a.Wp = (int)walkers_per_ensemble; a.ndim = ndim; a.mean = d_mean; a.cov = d_cov; a.part = (double *)d_work;
    const unsigned blocks = (unsigned)(n_ensembles * p.nseg);
    switch (ndim) {
    case 1: cv_launch<1>(a, blocks, st); break;
    case 2: cv_launch<2>(a, blocks, st); break;
    case 3: cv_launch<3>(a, blocks, st); break;
    case 4: cv_launch<4>(a, blocks, st); break;
    case 5: cv_launch<5>(a, blocks, st); break;
    case 6: cv_launch<6>(a, blocks, st); break;
    case 7: cv_launch<7>(a, blocks, st); break;
    case 8: cv_launch<8>(a, blocks, st); break;
    case 9: cv_launch<9>(a, blocks, st); break;
    case 10: cv_launch<10>(a, blocks, st); break;
    case 11: cv_launch<11>(a, blocks, st); break;
    case 12: cv_launch<12>(a, blocks, st); break;
    case 13: cv_launch<13>(a, blocks, st); break;
    case 14: cv_launch<14>(a, blocks, st); break;
    case 15: cv_launch<15>(a, blocks, st); break;
    default: cv_launch<16>(a, blocks, st); break;
    }
    HIP_TRY(hipGetLastError());
    if (p.nseg > 1) {
        hipLaunchKernelGGL(k_cov_merge, dim3((unsigned)n_ensembles), dim3(CV_THREADS), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

int64_t bisip_chain_best_sample_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble)
{
    if (check_rows_shape({n_samples, 0, n_ensembles, walkers_per_ensemble, 1}, QUIET) != BISIP_OK) return -1;
    const RowPlan p = bs_plan(n_samples, n_ensembles, walkers_per_ensemble);
    if (check_segment_grid(p.nseg, n_ensembles, QUIET) != BISIP_OK) return -1;
    return p.nseg > 1 ? 16 * n_ensembles * p.nseg : 0;
}

int bisip_chain_best_sample_dev(const double *d_chain, int64_t chain_stride, const double *d_logp, int64_t logp_stride,
                                int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                double *d_theta, double *d_best_logp, int64_t *d_index, void *d_work, int64_t work_bytes,
                                void *stream)
{
    if (!d_logp) return fail(BISIP_EINVAL, "null argument");
    if (!d_theta && !d_best_logp && !d_index) return fail(BISIP_EINVAL, "none of theta, log-probability and index asked for");
    if (d_theta && !d_chain) return fail(BISIP_EINVAL, "theta asked for without a chain");
    BISIP_TRY(check_ndim(ndim));
    BISIP_TRY(check_rows_shape({n_samples, chain_stride, n_ensembles, walkers_per_ensemble, ndim}, LOUD));
    // (two strides with names of their own; the caps on E and Wp keep both products within 64 bits)
    if (logp_stride < n_ensembles * walkers_per_ensemble)
        return fail(BISIP_EINVAL, "logp_stride smaller than one sample");
    if (d_chain && chain_stride < n_ensembles * walkers_per_ensemble * ndim)
        return fail(BISIP_EINVAL, "chain_stride smaller than one sample");
    const RowPlan p = bs_plan(n_samples, n_ensembles, walkers_per_ensemble);
    BISIP_TRY(check_segment_grid(p.nseg, n_ensembles));
    BISIP_TRY(check_workspace(d_work, work_bytes, p.nseg > 1 ? 16 * n_ensembles * p.nseg : 0));
    hipStream_t st = (hipStream_t)stream;
    BestArgs a{};
    a.chain = d_chain; a.logp = d_logp; a.cstride = chain_stride; a.lstride = logp_stride; a.N = p.N;
    a.seg_rows = p.seg_rows; a.nseg = p.nseg; a.Wp = (int)walkers_per_ensemble; a.ndim = ndim;
    a.theta = d_theta; a.best = d_best_logp; a.index = (long long *)d_index;
    a.pval = (double *)d_work; a.pidx = (long long *)d_work + n_ensembles * p.nseg;
    hipLaunchKernelGGL(k_best_scan, dim3((unsigned)(n_ensembles * p.nseg)), dim3(CV_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (p.nseg > 1) {
        hipLaunchKernelGGL(k_best_merge, dim3((unsigned)n_ensembles), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

}  // extern "C"
