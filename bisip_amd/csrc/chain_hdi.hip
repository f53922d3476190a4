// chain_hdi.hip -- highest-density intervals of a device-resident chain (bisip_chain_hdi_dev).
//
// The HDI of mass `mass` of a column of N values is the shortest interval that holds K = floor(mass * N) steps of the
// sorted column s: width[i] = s[i + K] - s[i], i = 0 ... M - 1 with M = N - K; a NaN width (inf - inf) is +inf; i* is the
// lowest i of smallest width; the interval is (s[i*], s[i* + K]); a column that holds a NaN gives (NaN, NaN) and i* = 0
// (include/bisip_hip.h; bisip_amd/interval.py holds the definition in NumPy).  Subtractions and comparisons of the same
// doubles: the result equals the definition's, bit for bit (up to the sign of a zero).
//
//   full path:  gather the columns (chain_columns.hip: gather_columns), sort them all with the segmented radix sort,
//               k_hdi_window over L = s, U = s + K.
//   tails path: only L = s[0 .. M-1] and U = s[K .. N-1] are ever read.  The order statistics a = s[M-1] and b = s[K] of
//               every column come from the selection kernel (select_columns, raw output); per window k_tails_compact
//               copies the values < a and > b of every column into two buffers of M, k_tails_fill completes them with the
//               threshold itself (equal doubles are interchangeable), the segmented sort orders the 2 x columns segments
//               of M and k_hdi_window reads the pairs.
// The path is a function of the shape and the windows alone (hdi_path below); BISIP_HDI_PATH=full|tails forces one.
#include "chain.h"

#include <cstdlib>

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int HDI_MAX_WINDOWS = 8;
constexpr int HDI_THREADS = 256;

// The tails path runs when every window's M = N - K is at most N / HDI_TAILS_SHARE and the columns have HDI_TAILS_MIN_N
// values at least.  Measured on an MI355X (benchmarks/interval_bench.py, medians of 5, the two paths alternating call by
// call; profiles/r05_interval_bench.jsonl), tails | full:
//   512 ensembles x 128,000 values x 7:  mass 0.95 (M = N / 20)             8.0 | 34.6 ms  (0.23)
//                                        masses 0.5, 0.9, 0.95 (M = N / 2)  50.0 | 35.5 ms  (1.41)
//   1 ensemble x 160,000 values x 7:     mass 0.95                          0.51 | 5.42 ms (0.09)
//                                        masses 0.5, 0.9, 0.95              4.05 | 5.45 ms (0.74)
// A window that keeps half of the column makes the tails the whole column, sorted after a selection and a compaction on
// top; at a twentieth the sort shrinks tenfold.  The share 1 / 8 lies between the measured points, nearer the one where the
// tails won by a factor of four; nothing between them was measured.  HDI_TAILS_MIN_N is not measured: below it the whole
// call is a handful of launches on either path (the tests drive both paths at every size).
constexpr long long HDI_TAILS_SHARE = 8;
constexpr long long HDI_TAILS_MIN_N = 4096;

struct WindowArgs {
    const double *lo;        // column c, window w: L = lo + c * col_stride, U = lo + hi_off[w] + c * col_stride
    long long col_stride, columns;
    long long n;             // values of a column
    long long K[HDI_MAX_WINDOWS], hi_off[HDI_MAX_WINDOWS];
    int n_windows;           // of this launch: blockIdx.y
    int w0;                  // its first window in the outputs
    const int *nan_flag;     // (columns,) or null: then NaNs are looked for at L[0] and U[M-1], where the sort puts them
    double *out;             // (windows, 2, columns)
    long long *index;        // (windows, columns) or null
};

// (width, i) < (bw, bi): smaller width, then smaller i
__device__ __forceinline__ bool hdi_better(double w, long long i, double bw, long long bi)
{
    return w < bw || (w == bw && i < bi);
}

// one workgroup per (column, window): lanes stride over i, the (width, i) pairs reduced by shuffles, then through LDS
__global__ __launch_bounds__(HDI_THREADS) void k_hdi_window(const WindowArgs a)
{
    __shared__ double sw[HDI_THREADS / 64];
    __shared__ long long si[HDI_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long col = blockIdx.x;
    const int w = blockIdx.y;
    const long long K = a.K[w], m = a.n - K;
    const double *__restrict__ L = a.lo + col * a.col_stride;
    const double *__restrict__ U = a.lo + a.hi_off[w] + col * a.col_stride;
    double bw = __builtin_inf();
    long long bi = 0x7fffffffffffffffLL;
    for (long long i = tid; i < m; i += HDI_THREADS) {
        double d = U[i] - L[i];
        if (d != d) d = __builtin_inf();          // inf - inf
        if (hdi_better(d, i, bw, bi)) { bw = d; bi = i; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ow = __shfl_xor(bw, s, 64);
        const long long oi = __shfl_xor(bi, s, 64);
        if (hdi_better(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
    if (lane == 0) { sw[wave] = bw; si[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < HDI_THREADS / 64; ++q)
            if (hdi_better(sw[q], si[q], bw, bi)) { bw = sw[q]; bi = si[q]; }
        // (m >= 1: lane 0 has seen i = 0, so bi < m)
        const double first = L[0], last = U[m - 1];
        const bool has_nan = a.nan_flag ? a.nan_flag[col] != 0 : (first != first || last != last);
        const long long o = (long long)(a.w0 + w) * 2 * a.columns + col;
        a.out[o] = has_nan ? __builtin_nan("") : L[bi];
        a.out[o + a.columns] = has_nan ? __builtin_nan("") : U[bi];
        if (a.index) a.index[(long long)(a.w0 + w) * a.columns + col] = has_nan ? 0 : bi;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// tails
// ---------------------------------------------------------------------------------------------------------------
constexpr int TL_VPT = 16;
constexpr int TL_CHUNK = HDI_THREADS * TL_VPT;

struct TailsArgs {
    const double *cols;       // (columns, n)
    long long n, columns, M, chunks;
    const double *thr_a;      // (columns,) s[M - 1]
    const double *thr_b;      // (columns,) s[K]
    double *tails;            // (2, columns, M): the M smallest, the M largest of every column
    unsigned *count;          // (2, columns): slots taken so far (zeroed before the launch)
    int *nan_flag;            // (columns,) (zeroed before the first launch)
};

// One workgroup per (column, chunk of TL_CHUNK values): counts its values < a and > b, reserves that many slots of the
// column's two buffers with one atomic each, writes them.  Every write index is checked against M: a NaN threshold makes
// every comparison false, and a column can never write past its buffer whatever its thresholds are.
__global__ __launch_bounds__(HDI_THREADS) void k_tails_compact(const TailsArgs a)
{
    __shared__ unsigned cnt[2], base[2];
    const int tid = threadIdx.x;
    const long long col = blockIdx.x / a.chunks, ch = blockIdx.x - col * a.chunks;
    const double *__restrict__ c = a.cols + col * a.n;
    const double ta = a.thr_a[col], tb = a.thr_b[col];
    const long long i0 = ch * TL_CHUNK + tid;
    double v[TL_VPT];
    unsigned below = 0, above = 0;
    bool nan = false;
    if (tid < 2) cnt[tid] = 0;
#pragma unroll
    for (int j = 0; j < TL_VPT; ++j) {
        const long long i = i0 + (long long)j * HDI_THREADS;
        const bool ok = i < a.n;
        v[j] = ok ? c[i] : 0.0;
        if (ok) {
            below += v[j] < ta;
            above += v[j] > tb;
            nan |= v[j] != v[j];
        }
    }
    __syncthreads();
    unsigned off_lo = below ? atomicAdd(&cnt[0], below) : 0u, off_hi = above ? atomicAdd(&cnt[1], above) : 0u;
    if (nan) a.nan_flag[col] = 1;
    __syncthreads();
    if (tid < 2) base[tid] = cnt[tid] ? atomicAdd(&a.count[tid * a.columns + col], cnt[tid]) : 0u;
    __syncthreads();
    double *__restrict__ dl = a.tails + col * a.M, *__restrict__ du = a.tails + (a.columns + col) * a.M;
    off_lo += base[0]; off_hi += base[1];
#pragma unroll
    for (int j = 0; j < TL_VPT; ++j) {
        const bool ok = i0 + (long long)j * HDI_THREADS < a.n;
        if (ok && v[j] < ta) { if ((long long)off_lo < a.M) dl[off_lo] = v[j]; ++off_lo; }
        if (ok && v[j] > tb) { if ((long long)off_hi < a.M) du[off_hi] = v[j]; ++off_hi; }
    }
}

// the slots the compaction left open take the threshold itself: the values equal to it
__global__ __launch_bounds__(HDI_THREADS) void k_tails_fill(const TailsArgs a)
{
    const long long idx = (long long)blockIdx.x * HDI_THREADS + threadIdx.x;
    if (idx >= 2 * a.columns * a.M) return;
    const long long seg = idx / a.M, j = idx - seg * a.M;
    if (j >= (long long)a.count[seg]) a.tails[idx] = seg < a.columns ? a.thr_a[seg] : a.thr_b[seg - a.columns];
}

enum HdiPath { HDI_FULL = 0, HDI_TAILS = 1 };

struct HdiPlan {
    long long n, columns, items;
    long long m_max;               // the largest M of the windows
    int path;
    size_t col_bytes, temp_bytes;  // one copy of the columns; the sort's scratch
    size_t thr_bytes, count_bytes, flag_bytes, tail_bytes;     // tails path
    size_t need;
};

// the shape rule, and what BISIP_HDI_PATH makes of it (read on every call)
int hdi_path(long long n, long long columns, long long m_max)
{
    int path = n >= HDI_TAILS_MIN_N && m_max * HDI_TAILS_SHARE <= n ? HDI_TAILS : HDI_FULL;
    if (2 * columns * m_max > 0x7fffffffLL) path = HDI_FULL;          // (the tails of one sort)
    const char *force = std::getenv("BISIP_HDI_PATH");
    if (force && !std::strcmp(force, "full")) path = HDI_FULL;
    if (force && !std::strcmp(force, "tails")) path = HDI_TAILS;
    return path;
}

// checks everything but pointers, the stride and the workspace; QUIET: the workspace function only reports < 0.  No
// count is capped as a bad shape: a chain beyond the 2^31 items of one sort is unsupported, after the windows are counted.
int make_plan(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, int n_windows,
              const int64_t *windows, HdiPlan &p, Voice v)
{
    BISIP_TRY(check_ndim(ndim, 1, v));
    BISIP_TRY(check_counts({n_samples, 0, n_ensembles, walkers_per_ensemble, ndim}, NO_CAP, NO_CAP, NO_CAP, v));
    if (n_windows < 1 || n_windows > HDI_MAX_WINDOWS)
        return refuse(v, BISIP_EINVAL, "n_windows=%d out of range (1 ... %d)", n_windows, HDI_MAX_WINDOWS);
    if (!windows) return refuse(v, BISIP_EINVAL, "null argument");
    if (n_samples > GRID_MAX || n_ensembles > GRID_MAX || walkers_per_ensemble > GRID_MAX ||     // (then the products fit)
        (p.n = n_samples * walkers_per_ensemble) > GRID_MAX || (p.columns = n_ensembles * ndim) > GRID_MAX ||
        p.n * p.columns > GRID_MAX)
        return refuse(v, BISIP_EUNSUPPORTED, "chain exceeds the 2^31 items of one sort");
    p.items = p.n * p.columns;
    p.m_max = 0;
    for (int w = 0; w < n_windows; ++w) {
        if (windows[w] < 1 || windows[w] > p.n - 1)
            return refuse(v, BISIP_EINVAL, "window %d of %lld steps outside [1, N - 1], N = %lld", w, (long long)windows[w], p.n);
        const long long m = p.n - windows[w];
        p.m_max = m > p.m_max ? m : p.m_max;
    }
    p.path = hdi_path(p.n, p.columns, p.m_max);
    p.col_bytes = align256((size_t)p.items * 8);
    p.thr_bytes = p.count_bytes = p.flag_bytes = p.tail_bytes = 0;
    if (p.path == HDI_FULL) {
        p.temp_bytes = sort_scratch_bound(p.items, p.columns);
        p.need = 2 * p.col_bytes + align256(p.temp_bytes);
    } else {
        if (2 * p.columns * p.m_max > GRID_MAX)
            return refuse(v, BISIP_EUNSUPPORTED, "tails of %lld values exceed the 2^31 items of one sort", 2 * p.columns * p.m_max);
        p.temp_bytes = sort_scratch_bound(2 * p.columns * p.m_max, 2 * p.columns);
        p.thr_bytes = align256((size_t)(2 * n_windows) * p.columns * 8);
        p.count_bytes = align256((size_t)2 * p.columns * 4);
        p.flag_bytes = align256((size_t)p.columns * 4);
        p.tail_bytes = align256((size_t)2 * p.columns * p.m_max * 8);
        p.need = p.col_bytes + p.thr_bytes + p.count_bytes + p.flag_bytes + 2 * p.tail_bytes + align256(p.temp_bytes);
    }
    return BISIP_OK;
}

}  // namespace

extern "C" {

int64_t bisip_chain_hdi_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                  int n_windows, const int64_t *windows)
{
    HdiPlan p{};
    if (make_plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, n_windows, windows, p, QUIET) != BISIP_OK) return -1;
    return (int64_t)p.need;
}

int bisip_chain_hdi_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                        int64_t walkers_per_ensemble, int ndim, const int64_t *windows, int n_windows, double *d_out,
                        int64_t *d_index, void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_chain || !windows || !d_out || !d_work) return fail(BISIP_EINVAL, "null argument");
    HdiPlan p{};
    BISIP_TRY(make_plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, n_windows, windows, p, LOUD));
    BISIP_TRY(check_stride({n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim}));
    BISIP_TRY(check_workspace(d_work, work_bytes, (int64_t)p.need));
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)d_work;
    double *cols = (double *)base;
    int rc = gather_columns(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, cols, st);
    if (rc != BISIP_OK) return rc;

    WindowArgs wa{};
    wa.columns = p.columns; wa.n = p.n; wa.out = d_out; wa.index = (long long *)d_index;
    if (p.path == HDI_FULL) {
        double *sorted = (double *)(base + p.col_bytes);
        rc = sort_segments(base + 2 * p.col_bytes, p.temp_bytes, cols, sorted, p.items, p.columns, p.n, st);
        if (rc != BISIP_OK) return rc;
        wa.lo = sorted; wa.col_stride = p.n; wa.n_windows = n_windows; wa.w0 = 0; wa.nan_flag = nullptr;
        for (int w = 0; w < n_windows; ++w) { wa.K[w] = windows[w]; wa.hi_off[w] = windows[w]; }
        hipLaunchKernelGGL(k_hdi_window, dim3((unsigned)p.columns, (unsigned)n_windows), dim3(HDI_THREADS), 0, st, wa);
        HIP_TRY(hipGetLastError());
        return BISIP_OK;
    }

    char *q = base + p.col_bytes;
    double *thr = (double *)q; q += p.thr_bytes;
    unsigned *count = (unsigned *)q; q += p.count_bytes;
    int *flag = (int *)q; q += p.flag_bytes;
    double *tails = (double *)q; q += p.tail_bytes;
    double *sorted = (double *)q; q += p.tail_bytes;
    void *d_temp = q;
    // a = s[M - 1] and b = s[K] of every column and window, the order statistics themselves
    std::vector<long long> lo(2 * n_windows);
    std::vector<double> t(2 * n_windows, 0.0);
    for (int w = 0; w < n_windows; ++w) { lo[2 * w] = p.n - windows[w] - 1; lo[2 * w + 1] = windows[w]; }
    rc = select_columns(cols, p.n, p.columns, 2 * n_windows, lo, t, thr, st, p.columns, true);
    if (rc != BISIP_OK) return rc;
    HIP_TRY(hipMemsetAsync(flag, 0, p.flag_bytes, st));
    for (int w = 0; w < n_windows; ++w) {
        TailsArgs ta{};
        ta.cols = cols; ta.n = p.n; ta.columns = p.columns; ta.M = p.n - windows[w];
        ta.chunks = (p.n + TL_CHUNK - 1) / TL_CHUNK;
        ta.thr_a = thr + (long long)(2 * w) * p.columns; ta.thr_b = thr + (long long)(2 * w + 1) * p.columns;
        ta.tails = tails; ta.count = count; ta.nan_flag = flag;
        HIP_TRY(hipMemsetAsync(count, 0, p.count_bytes, st));
        hipLaunchKernelGGL(k_tails_compact, dim3((unsigned)(p.columns * ta.chunks)), dim3(HDI_THREADS), 0, st, ta);
        HIP_TRY(hipGetLastError());
        const long long titems = 2 * p.columns * ta.M;
        hipLaunchKernelGGL(k_tails_fill, dim3((unsigned)((titems + HDI_THREADS - 1) / HDI_THREADS)), dim3(HDI_THREADS), 0, st, ta);
        HIP_TRY(hipGetLastError());
        rc = sort_segments(d_temp, p.temp_bytes, tails, sorted, titems, 2 * p.columns, ta.M, st);
        if (rc != BISIP_OK) return rc;
        wa.lo = sorted; wa.col_stride = ta.M; wa.n_windows = 1; wa.w0 = w; wa.nan_flag = flag;
        wa.K[0] = windows[w]; wa.hi_off[0] = p.columns * ta.M;
        hipLaunchKernelGGL(k_hdi_window, dim3((unsigned)p.columns, 1u), dim3(HDI_THREADS), 0, st, wa);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

}  // extern "C"
