// chain_trace.hip -- per-step walker statistics of a device-resident chain (bisip_chain_trace_dev): what the
// reference's plot_traces (src/bisip/plotlib.py:17-54) shows as one line per walker, reduced along the WALKER axis
// instead -- for every used sample, ensemble and parameter the percentiles and the mean of that step's Wp walkers.
//
//   * k_chain_trace_lds: one 256-lane workgroup per (sample, ensemble), or per (sample, G small ensembles).  The
//     contiguous Wp x ndim block is read from memory once, coalesced, and stored in LDS parameter-major as
//     order-preserving 64-bit keys (select_key.h): column c = (ensemble, parameter) at c * pitch, walker w at slot
//     w + (w >> 5).  Columns are padded to a power of two (npad >= 8) with the largest key.  pitch = (npad + npad / 32)
//     | 1 is odd: the ndim-strided transposing store of consecutive lanes lands on different banks; the extra slot per
//     32 keeps the strided reads of the sorting rounds off one bank.
//   * The mean comes from the same LDS copy before it is sorted, in the order trace_column_sum fixes.
//   * Every column is then SORTED by a bitonic network, all columns at once.  A thread takes 8 keys that differ in
//     three index bits into registers and does the three stages on those bits there, so the 36 stages of 256 keys cost
//     13 trips through LDS, not 36 (the first trip does the whole of the first three merges).  Any number of
//     percentiles then reads its two neighbours from the sorted column; numpy's _lerp between them, as
//     k_percentile_lerp / k_segmented_select.  A NaN sorts to one of the ends: the column's percentiles are NaN.
//     (Why a sort and not range narrowing on the keys: DESIGN.md, "Walker traces".)
//   * Ensembles beyond bisip_chain_trace_lds_walkers(ndim) go slab by slab through k_gather_columns_tiled (one column
//     per (sample, ensemble, parameter)), k_segmented_select and k_trace_column_mean: the same order statistics, the
//     same _lerp, the same summation order => the same doubles whichever path ran.
#include "chain.h"
#include "select_key.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int TR_MAX_P = 8;                   // percentiles per call
constexpr int TR_THREADS = 256;
constexpr size_t TR_LDS_BYTES = 65536;        // the static limit; a workgroup allocates only what its columns take
constexpr int TR_GROUP_KEYS = 2048;           // small ensembles share a workgroup up to this many padded keys
constexpr long long TR_SLAB_BYTES = 256LL << 20;    // gather path: columns of one slab of samples (or of one sample, if larger)

__host__ __device__ inline int tr_npad(long long wp)
{
    int n = 8;
    while (n < wp) n <<= 1;
    return n;
}
__host__ __device__ inline int tr_pitch(int npad) { return (npad + (npad >> 5)) | 1; }
__device__ __forceinline__ int tr_slot(int i) { return i + (i >> 5); }

// the largest (power of two) column the LDS kernel takes at this ndim
int lds_walkers(int ndim)
{
    int npad = 8;
    while ((size_t)ndim * tr_pitch(2 * npad) * 8 <= TR_LDS_BYTES) npad *= 2;
    return npad;
}

struct TraceArgs {
    const double *chain;
    long long n_samples, sample_stride, E;
    long long groups;            // workgroups per sample: ceil(E / G)
    int Wp, ndim, G;             // G ensembles per workgroup
    int npad, log_npad, pitch;
    int n_p;
    int lo[TR_MAX_P];            // lower order statistic of each percentile (kernarg segment: no upload, no wait)
    double t[TR_MAX_P];          // weight of the upper one
    double *pct;                 // (n_p, n_samples, E, ndim)
    double *mean;                // (n_samples, E, ndim) or null
};

// The sum of a column of n values as one wave takes it, the order both paths keep: lane l adds values l, l + 64, ... in
// turn onto 0.0, then lanes 32, 16, ..., 1 apart are added pairwise (wave_sum).  f(w) = value w.
template <typename F>
__device__ __forceinline__ double trace_column_sum(int lane, long long n, F &&f)
{
    double acc = 0.0;
    for (long long w = lane; w < n; w += 64) acc += f(w);
    return wave_sum(acc);
}

__device__ __forceinline__ void tr_ce(unsigned long long &x, unsigned long long &y, bool asc)
{
    const bool gt = x > y;
    const unsigned long long lo = gt ? y : x, hi = gt ? x : y;
    x = asc ? lo : hi;
    y = asc ? hi : lo;
}

// The first three merges of the network (sorted runs of 8, ascending where bit 3 of the index is clear) on the 8
// consecutive keys of a thread.
__device__ __forceinline__ void tr_sort8(unsigned long long *keys, int tid, int C, const TraceArgs &a)
{
    const int log_per = a.log_npad - 3, tasks = C << log_per;
    for (int task = tid; task < tasks; task += TR_THREADS) {
        const int c = task >> log_per, base = (task & ((1 << log_per) - 1)) << 3;
        unsigned long long *col = keys + c * a.pitch;
        unsigned long long x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = col[tr_slot(base + r)];
        tr_ce(x[0], x[1], true); tr_ce(x[2], x[3], false); tr_ce(x[4], x[5], true); tr_ce(x[6], x[7], false);
        tr_ce(x[0], x[2], true); tr_ce(x[1], x[3], true); tr_ce(x[4], x[6], false); tr_ce(x[5], x[7], false);
        tr_ce(x[0], x[1], true); tr_ce(x[2], x[3], true); tr_ce(x[4], x[5], false); tr_ce(x[6], x[7], false);
        const bool asc = (base & 8) == 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) tr_ce(x[r], x[r + 4], asc);
        tr_ce(x[0], x[2], asc); tr_ce(x[1], x[3], asc); tr_ce(x[4], x[6], asc); tr_ce(x[5], x[7], asc);
#pragma unroll
        for (int r = 0; r < 8; r += 2) tr_ce(x[r], x[r + 1], asc);
#pragma unroll
        for (int r = 0; r < 8; ++r) col[tr_slot(base + r)] = x[r];
    }
}

// Stages b_lo + NB - 1, ..., b_lo of the merge whose runs have k keys: a thread takes the 2^NB keys of a column whose
// indices differ in those bits.  Bit k of the index (above all of them) says which way its run is sorted.
template <int NB>
__device__ __forceinline__ void tr_round(unsigned long long *keys, int tid, int C, const TraceArgs &a, int b_lo, int k)
{
    constexpr int M = 1 << NB;
    const int log_per = a.log_npad - NB, tasks = C << log_per;
    for (int task = tid; task < tasks; task += TR_THREADS) {
        const int c = task >> log_per, tp = task & ((1 << log_per) - 1);
        const int base = ((tp >> b_lo) << (b_lo + NB)) | (tp & ((1 << b_lo) - 1));
        unsigned long long *col = keys + c * a.pitch;
        const bool asc = (base & k) == 0;
        unsigned long long x[M];
#pragma unroll
        for (int r = 0; r < M; ++r) x[r] = col[tr_slot(base | (r << b_lo))];
#pragma unroll
        for (int b = NB - 1; b >= 0; --b) {
#pragma unroll
            for (int r = 0; r < M; ++r)
                if (!(r & (1 << b))) tr_ce(x[r], x[r | (1 << b)], asc);
        }
#pragma unroll
        for (int r = 0; r < M; ++r) col[tr_slot(base | (r << b_lo))] = x[r];
    }
}

__global__ __launch_bounds__(TR_THREADS) void k_chain_trace_lds(const TraceArgs a)
{
    extern __shared__ unsigned long long s_keys[];        // (C, pitch)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = blockIdx.x / a.groups, g = blockIdx.x - s * a.groups;
    const long long e0 = g * a.G;
    const int Gb = (int)(a.E - e0 < a.G ? a.E - e0 : a.G);
    const int C = Gb * a.ndim, total = Gb * a.Wp * a.ndim;      // <= TR_LDS_BYTES / 8
    const double *__restrict__ src = a.chain + s * a.sample_stride + e0 * a.Wp * a.ndim;
    for (int i = tid; i < total; i += TR_THREADS) {
        const int row = i / a.ndim, q = i - row * a.ndim;
        const int eg = row / a.Wp, w = row - eg * a.Wp;
        s_keys[(eg * a.ndim + q) * a.pitch + tr_slot(w)] = select_key(__builtin_nontemporal_load(src + i));
    }
    const int extra = a.npad - a.Wp;
    for (int i = tid; i < C * extra; i += TR_THREADS) {
        const int c = i / extra, w = a.Wp + (i - c * extra);
        s_keys[c * a.pitch + tr_slot(w)] = ~0ull;
    }
    __syncthreads();
    const long long out0 = (s * a.E + e0) * a.ndim;              // (s, e0, 0); column c of the workgroup is out0 + c
    if (a.mean) {
        for (int c = wave; c < C; c += TR_THREADS / 64) {
            const unsigned long long *col = s_keys + c * a.pitch;
            const double sum = trace_column_sum(lane, a.Wp, [&](long long w) { return select_value(col[tr_slot((int)w)]); });
            if (lane == 0) a.mean[out0 + c] = sum / (double)a.Wp;
        }
    }
    if (a.n_p == 0) return;                                      // (uniform)
    __syncthreads();
    tr_sort8(s_keys, tid, C, a);
    __syncthreads();
    for (int m = 4; m <= a.log_npad; ++m) {                      // merge into runs of k = 2^m: stages m - 1 ... 0
        const int k = 1 << m;
        for (int hi = m - 1; hi >= 0;) {
            const int nb = hi + 1 < 3 ? hi + 1 : 3, b_lo = hi - nb + 1;
            if (nb == 3) tr_round<3>(s_keys, tid, C, a, b_lo, k);
            else if (nb == 2) tr_round<2>(s_keys, tid, C, a, b_lo, k);
            else tr_round<1>(s_keys, tid, C, a, b_lo, k);
            __syncthreads();
            hi = b_lo - 1;
        }
    }
    const long long k_stride = a.n_samples * a.E * a.ndim;
    for (int i = tid; i < C * a.n_p; i += TR_THREADS) {
        const int k = i / C, c = i - k * C;
        const unsigned long long *col = s_keys + c * a.pitch;
        const int lo = a.lo[k], hi = lo + 1 < a.Wp ? lo + 1 : a.Wp - 1;
        const bool has_nan = select_key_is_nan(col[0]) || select_key_is_nan(col[tr_slot(a.Wp - 1)]);
        const double x = select_value(col[tr_slot(lo)]), y = select_value(col[tr_slot(hi)]), t = a.t[k];
        const double d = y - x;
        // numpy.lib._function_base_impl._lerp, as k_percentile_lerp
        a.pct[k * k_stride + out0 + c] = has_nan ? __builtin_nan("") : (t >= 0.5 ? y - d * (1.0 - t) : x + d * t);
    }
}

// gather path: the mean of `columns` contiguous columns of n values, one wave per column, trace_column_sum's order
__global__ __launch_bounds__(TR_THREADS) void k_trace_column_mean(const double *__restrict__ cols, long long n, long long columns,
                                                                  double *__restrict__ out)
{
    const long long c = (long long)blockIdx.x * (TR_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= columns) return;                                    // (whole waves)
    const double *__restrict__ col = cols + c * n;
    const double sum = trace_column_sum(threadIdx.x & 63, n, [&](long long w) { return col[w]; });
    if ((threadIdx.x & 63) == 0) out[c] = sum / (double)n;
}

// samples per slab of the gather path; 0: one sample alone exceeds a grid
long long slab_samples(long long n, long long E, long long Wp, int ndim)
{
    const long long per_sample = E * Wp * ndim * 8;
    long long S = TR_SLAB_BYTES / per_sample;
    const long long by_columns = 0x7fffffffLL / (E * ndim), by_tiles = 0x7fffffffLL / (E * ((Wp + 63) / 64));
    if (S < 1) S = 1;
    if (S > by_columns) S = by_columns;
    if (S > by_tiles) S = by_tiles;
    return S < n ? S : n;
}

// Wp: an int in TraceArgs; E: 32 bits too; n is not capped here: each path holds its samples to one grid further down
int check_trace_shape(const ChainShape &s, int n_percentiles, Voice v)
{
    BISIP_TRY(check_ndim(s.ndim, 1, v));
    if (n_percentiles < 0 || n_percentiles > TR_MAX_P)
        return refuse(v, BISIP_EINVAL, "n_percentiles=%d: 0 ... %d per call", n_percentiles, TR_MAX_P);
    return check_counts(s, NO_CAP, GRID_MAX, GRID_MAX, v);
}

}  // namespace

extern "C" {

int bisip_chain_trace_lds_walkers(int ndim)
{
    if (ndim < 1 || ndim > BISIP_MAX_NDIM) return 0;
    return lds_walkers(ndim);
}

int64_t bisip_chain_trace_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                    int n_percentiles)
{
    if (check_trace_shape({n_samples, 0, n_ensembles, walkers_per_ensemble, ndim}, n_percentiles, QUIET) != BISIP_OK) return -1;
    if (walkers_per_ensemble <= lds_walkers(ndim)) return 0;
    const long long S = slab_samples(n_samples, n_ensembles, walkers_per_ensemble, ndim);
    if (S < 1) return -1;
    return S * n_ensembles * walkers_per_ensemble * ndim * 8;
}

int bisip_chain_trace_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, const double *percentiles, int n_percentiles,
                          double *d_pct, double *d_mean, void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_chain || (n_percentiles > 0 && (!percentiles || !d_pct))) return fail(BISIP_EINVAL, "null argument");
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_trace_shape(s, n_percentiles, LOUD));
    BISIP_TRY(check_stride(s));
    if (n_percentiles == 0 && !d_mean) return fail(BISIP_EINVAL, "neither percentiles nor the mean asked for");
    const long long E = n_ensembles, Wp = walkers_per_ensemble;
    std::vector<long long> lo(n_percentiles);
    std::vector<double> t(n_percentiles);
    int rc = percentile_ranks(Wp, percentiles, n_percentiles, lo, t);
    if (rc != BISIP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;

    if (Wp <= lds_walkers(ndim)) {
        TraceArgs a{};
        a.chain = d_chain; a.n_samples = n_samples; a.sample_stride = sample_stride; a.E = E;
        a.Wp = (int)Wp; a.ndim = ndim;
        a.npad = tr_npad(Wp); a.pitch = tr_pitch(a.npad);
        for (a.log_npad = 3; (1 << a.log_npad) < a.npad; ++a.log_npad) {}
        long long G = TR_GROUP_KEYS / ((long long)a.npad * ndim);
        G = G < 1 ? 1 : (G > E ? E : G);
        a.G = (int)G;
        a.groups = (E + G - 1) / G;
        a.n_p = n_percentiles;
        for (int k = 0; k < n_percentiles; ++k) { a.lo[k] = (int)lo[k]; a.t[k] = t[k]; }
        a.pct = d_pct; a.mean = d_mean;
        const size_t lds = (size_t)G * ndim * a.pitch * 8;
        if (lds > TR_LDS_BYTES) return fail(BISIP_EHIP, "trace columns of %zu bytes exceed the LDS of a workgroup", lds);
        BISIP_TRY(check_grid(a.groups, n_samples, LOUD, "%lld samples x %lld workgroups", (long long)n_samples, a.groups));
        hipLaunchKernelGGL(k_chain_trace_lds, dim3((unsigned)(n_samples * a.groups)), dim3(TR_THREADS), lds, st, a);
        HIP_TRY(hipGetLastError());
        return BISIP_OK;
    }

    const long long S = slab_samples(n_samples, E, Wp, ndim);
    if (S < 1) return fail(BISIP_EUNSUPPORTED, "one sample of %lld x %lld walkers exceeds one grid", E, Wp);
    const long long per_sample = E * Wp * ndim, out_per_sample = E * ndim;
    BISIP_TRY(check_workspace(d_work, work_bytes, S * per_sample * 8));
    double *cols = (double *)d_work;
    for (long long s0 = 0; s0 < n_samples; s0 += S) {
        const long long Sb = n_samples - s0 < S ? n_samples - s0 : S, columns = Sb * out_per_sample;
        rc = gather_columns_by_sample(d_chain + s0 * sample_stride, Sb, sample_stride, E, Wp, ndim, cols, st);
        if (rc != BISIP_OK) return rc;
        if (n_percentiles > 0) {
            rc = select_columns(cols, Wp, columns, n_percentiles, lo, t, d_pct + s0 * out_per_sample, st,
                                n_samples * out_per_sample);
            if (rc != BISIP_OK) return rc;
        }
        if (d_mean) {
            const unsigned blocks = (unsigned)((columns + TR_THREADS / 64 - 1) / (TR_THREADS / 64));
            hipLaunchKernelGGL(k_trace_column_mean, dim3(blocks), dim3(TR_THREADS), 0, st, (const double *)cols, Wp, columns,
                               d_mean + s0 * out_per_sample);
            HIP_TRY(hipGetLastError());
        }
    }
    return BISIP_OK;
}

}  // extern "C"
