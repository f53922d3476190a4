// chain_loo.hip -- PSIS-LOO of a device-resident chain: the squared standardised residuals q of every data point as columns
// (bisip_q_columns_dev) and, per column, the Pareto-smoothed leave-one-out sum and the Pareto shape of its upper tail
// (bisip_loo_columns_dev).  The definition is bisip_amd/loo.py (tail_length, gpd_fit, psis_loo_columns); loo.ordered_columns
// restates the order of every sum below in NumPy.
//
// A column holds the R values q of one data point, the log importance ratio of a row is q / 2, r(x) = exp((x - qmax) / 2).
//
//   1. select_columns (chain_columns.hip), raw: u = s[R - M - 1] and qmax = s[R - 1] of every column, M = tail_len.  A column
//      that holds a NaN gives NaN for both.
//   2. k_loo_compact, one workgroup per (column, chunk of 4096 values): the values > u go to the column's buffer of M slots
//      (one integer atomic per chunk reserves them: their order in the buffer is not fixed, the sort below removes it), a NaN
//      sets the column's flag, and the chunk's body sum  sum_{q <= u} r(q)  goes to a partial of its own: lane t of the 256
//      takes values t, t + 256, ... of the chunk in ascending order from 0.0 (a value of the tail adds 0.0), the lanes are
//      added pairwise within each wave, 32, 16, ..., 1 apart, the four waves then in ascending order.
//   3. k_loo_fill: the open slots take u itself; sort_segments orders every buffer: n_tail values of the tail in ascending
//      order behind M - n_tail copies of u.
//   4. k_loo_tail, one workgroup of 256 per column.  n = n_tail.  n <= 4: khat = +inf, nothing fitted.  Else
//      x_i = r(tail_i) - eu, eu = r(u), held in LDS when M <= LOO_LDS_CAP and else in the (dead) unsorted buffer of the
//      column: the same values either way.  m = 30 + floor(sqrt(n)) profile points b_j, j = 1 ... m: wave w takes j = w + 1,
//      w + 5, ...; lane l adds log1p(-b_j x_i) for i = l, l + 64, ... in ascending order, lanes pairwise 32 ... 1 apart;
//      k_j = sum / n, L_j = n ((log(-b_j / k_j) - k_j) - 1).  Thread j takes 1 / sum_i exp(L_i - L_j), i ascending; b = sum_j
//      b_j w_j, j ascending.  k: thread t adds log1p(-b x_i), i = t, t + 256, ... ascending, then the block tree (waves
//      pairwise, the four in ascending order); sigma = -k / b; khat = k n / (n + 10) + 5 / (n + 10); not finite: +inf and
//      nothing smoothed.  The smoothed weights w_i = min(eu + (sigma expm1(-khat log1p(-p_i))) / khat, 1), p_i = (i + 0.5) /
//      n, and the two sums  sum w_i  and  sum w_i / r_i  over the same block tree (unsmoothed: w_i = r_i and the second sum
//      is n).  The chunks' body sums are added in ascending order.
//      elpd_rel = (-qmax / 2 + log((R - n) + sum w / r)) - log(body + sum w).
//   exp, log, log1p and expm1 are the device library's; every other operation is one IEEE operation (-ffp-contract=off).
//   No floating-point atomics: the same call gives the same bits twice.  64-bit offsets throughout.
//
// Resource report (-Rpass-analysis=kernel-resource-usage, gfx950): 6 to 94 VGPRs, no AGPRs and no scratch in any kernel of
// the unit; the table stands before the kernels.
//
// The unit needs the context (the records of bisip_q_columns_dev) and so takes host.h through row_pass.h, as
// dispatch_fit.hip does; kernels.h and chain.h both define wave_sum, so what it uses of the column toolkit (chain.h,
// chain_columns.hip) is declared here instead of included.  The checks and align256 come from chain_check.h.
#include "chain_check.h"
#include "row_pass.h"

namespace bisip {
namespace host {
int select_columns(const double *cols, long long n, long long columns, int n_percentiles, const std::vector<long long> &lo,
                   const std::vector<double> &t, double *d_out, hipStream_t st, long long out_stride, bool raw);
size_t sort_scratch_bound(long long items, long long segments);
int sort_segments(void *d_temp, size_t temp, const double *in, double *out, long long items, long long segments, long long n,
                  hipStream_t st);
}  // namespace host
}  // namespace bisip

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int LOO_THREADS = 256;
constexpr int LOO_VPT = 16;
constexpr int LOO_CHUNK = LOO_THREADS * LOO_VPT;     // values of a compaction chunk
constexpr int LOO_LDS_CAP = 2048;                    // tails of up to this many values are fitted from LDS (16 KiB)
constexpr int LOO_MAX_M = 256;                       // profile points at most: m = 30 + floor(sqrt(n_tail))
constexpr long long LOO_MAX_TAIL = 227LL * 227 - 1;  // the longest tail with m <= LOO_MAX_M

// Resource report of the unit (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_q_columns       VGPRs  6, no AGPRs, no scratch, LDS 0,        8 waves / SIMD
//   k_loo_compact     VGPRs 52, no AGPRs, no scratch, LDS 40 B,     8 waves / SIMD
//   k_loo_fill        VGPRs 13, no AGPRs, no scratch, LDS 0,        8 waves / SIMD
//   k_loo_tail<true>  VGPRs 94, no AGPRs, no scratch, LDS 22,560 B, 5 waves / SIMD
//   k_loo_tail<false> VGPRs 94, no AGPRs, no scratch, LDS 6,176 B,  5 waves / SIMD

// ---------------------------------------------------------------------------------------------------------------
// responses -> q, in place
// ---------------------------------------------------------------------------------------------------------------
constexpr int QC_VPT = 8;

struct QArgs {
    double *cols;            // (n_spectra, 2N, rows): Re / Im columns in, q out
    long long rows, chunks;  // chunks of LOO_THREADS * QC_VPT rows of a column
    int N, rec;              // frequencies; doubles of a record
    const double *cb;        // records of the call's first spectrum
    long long cb_stride;
};

// one workgroup per (column, chunk): y and iv of the column come from its frequency's record (rec[0..3] = y_re, y_im,
// iv_re, iv_im), the bits of fq_q (dispatch_fit.hip)
__global__ __launch_bounds__(LOO_THREADS) void k_q_columns(const QArgs a)
{
    const long long col = blockIdx.x / a.chunks, ch = blockIdx.x - col * a.chunks;
    const long long e = col / (2 * a.N);
    const int c = (int)(col - e * 2 * a.N), part = c / a.N, j = c - part * a.N;
    const double *__restrict__ rec = a.cb + e * a.cb_stride + (long long)j * a.rec;
    const double y = rec[part], iv = rec[2 + part];
    double *__restrict__ z = a.cols + col * a.rows;
    const long long i0 = ch * (LOO_THREADS * QC_VPT) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < QC_VPT; ++k) {
        const long long i = i0 + (long long)k * LOO_THREADS;
        if (i < a.rows) {
            const double d = __dsub_rn(y, z[i]);
            z[i] = __dmul_rn(__dmul_rn(d, d), iv);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the column pass
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double loo_r(double x, double qmax) { return exp(0.5 * (x - qmax)); }

struct LooArgs {
    const double *cols;       // (columns, n)
    long long n, columns, M, chunks;
    const double *thr;        // (2, columns): u, then qmax
    double *tails;            // (columns, M): compacted, not ordered; k_loo_tail<false> keeps x there
    const double *sorted;     // (columns, M)
    unsigned *count;          // (columns,) slots taken (zeroed before the launch): n_tail
    int *nan_flag;            // (columns,) (zeroed before the launch)
    double *part;             // (columns, chunks) body sums
    double *elpd, *khat, *sigma;   // (columns,) each; any may be null
    long long *ntail;              // (columns,) or null
};

// the sum of x over the 256 threads, in every thread: pairwise within each wave, the four waves in ascending order
__device__ __forceinline__ double block_sum(double x, double *s_wave)
{
    x = wave_sum(x);
    __syncthreads();                                  // (s_wave may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// Every write index is checked against M: a NaN threshold makes every comparison false, and a column can never write
// past its buffer whatever its threshold is (the pattern of k_tails_compact, chain_hdi.hip, upper side only).
__global__ __launch_bounds__(LOO_THREADS) void k_loo_compact(const LooArgs a)
{
    __shared__ unsigned cnt, base;
    __shared__ double s_wave[4];
    const int tid = threadIdx.x;
    const long long col = blockIdx.x / a.chunks, ch = blockIdx.x - col * a.chunks;
    const double *__restrict__ c = a.cols + col * a.n;
    const double u = a.thr[col], qmax = a.thr[a.columns + col];
    const long long i0 = ch * LOO_CHUNK + tid;
    double v[LOO_VPT];
    unsigned above = 0;
    bool nan = false;
    double body = 0.0;
    if (tid == 0) cnt = 0;
#pragma unroll
    for (int j = 0; j < LOO_VPT; ++j) {
        const long long i = i0 + (long long)j * LOO_THREADS;
        const bool ok = i < a.n;
        v[j] = ok ? c[i] : 0.0;
        if (ok) {
            above += v[j] > u;
            nan |= v[j] != v[j];
            body += v[j] <= u ? loo_r(v[j], qmax) : 0.0;
        }
    }
    __syncthreads();
    unsigned off = above ? atomicAdd(&cnt, above) : 0u;
    if (nan) a.nan_flag[col] = 1;
    body = block_sum(body, s_wave);                   // (its barriers also order cnt)
    if (tid == 0) {
        base = cnt ? atomicAdd(&a.count[col], cnt) : 0u;
        a.part[col * a.chunks + ch] = body;
    }
    __syncthreads();
    double *__restrict__ dst = a.tails + col * a.M;
    off += base;
#pragma unroll
    for (int j = 0; j < LOO_VPT; ++j) {
        const bool ok = i0 + (long long)j * LOO_THREADS < a.n;
        if (ok && v[j] > u) { if ((long long)off < a.M) dst[off] = v[j]; ++off; }
    }
}

// the slots the compaction left open take the threshold itself
__global__ __launch_bounds__(LOO_THREADS) void k_loo_fill(const LooArgs a)
{
    const long long idx = (long long)blockIdx.x * LOO_THREADS + threadIdx.x;
    if (idx >= a.columns * a.M) return;
    const long long col = idx / a.M, j = idx - col * a.M;
    if (j >= (long long)a.count[col]) a.tails[idx] = a.thr[col];
}

template <bool LDS>
__global__ __launch_bounds__(LOO_THREADS) void k_loo_tail(const LooArgs a)
{
    __shared__ double s_x[LDS ? LOO_LDS_CAP : 1];
    __shared__ double s_b[LOO_MAX_M], s_L[LOO_MAX_M], s_bw[LOO_MAX_M];
    __shared__ double s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long col = blockIdx.x;
    if (a.nan_flag[col]) {                            // (the same in every thread)
        if (tid == 0) {
            if (a.elpd) a.elpd[col] = __builtin_nan("");
            if (a.khat) a.khat[col] = __builtin_nan("");
            if (a.sigma) a.sigma[col] = __builtin_nan("");
            if (a.ntail) a.ntail[col] = 0;
        }
        return;
    }
    const long long cnt = a.count[col];
    const int n = (int)(cnt < a.M ? cnt : a.M);
    const double nd = (double)n, R = (double)a.n;
    const double u = a.thr[col], qmax = a.thr[a.columns + col];
    const double eu = loo_r(u, qmax);
    const double *__restrict__ t = a.sorted + col * a.M + (a.M - n);
    double khat = __builtin_inf(), sigma = __builtin_nan("");
    bool smooth = false;
    if (n > 4) {
        double *x;
        if constexpr (LDS) x = s_x; else x = a.tails + col * a.M;
        for (int i = tid; i < n; i += LOO_THREADS) x[i] = loo_r(t[i], qmax) - eu;
        __syncthreads();
        const int m = 30 + (int)floor(__dsqrt_rn(nd));
        const double xq = x[(int)floor(nd / 4.0 + 0.5) - 1], xn = x[n - 1];
        for (int j = wave; j < m; j += LOO_THREADS / 64) {
            const double bj = 1.0 / xn + (1.0 - __dsqrt_rn((double)m / ((double)(j + 1) - 0.5))) / (3.0 * xq);
            double s = 0.0;
            for (int i = lane; i < n; i += 64) s += log1p(-bj * x[i]);
            s = wave_sum(s);
            const double kj = s / nd;
            if (lane == 0) { s_b[j] = bj; s_L[j] = nd * ((log(-bj / kj) - kj) - 1.0); }
        }
        __syncthreads();
        if (tid < m) {
            const double Lj = s_L[tid];
            double den = 0.0;
            for (int i = 0; i < m; ++i) den += exp(s_L[i] - Lj);
            s_bw[tid] = s_b[tid] * (1.0 / den);
        }
        __syncthreads();
        double b = 0.0;
        for (int j = 0; j < m; ++j) b += s_bw[j];
        double s = 0.0;
        for (int i = tid; i < n; i += LOO_THREADS) s += log1p(-b * x[i]);
        const double k = block_sum(s, s_wave) / nd;
        sigma = -k / b;
        khat = (k * nd) / (nd + 10.0) + 5.0 / (nd + 10.0);
        smooth = fabs(khat) < __builtin_inf();        // (false for a NaN)
        if (!smooth) { khat = __builtin_inf(); sigma = __builtin_nan(""); }
    }
    double sw = 0.0, swr = 0.0;
    for (int i = tid; i < n; i += LOO_THREADS) {
        const double r = loo_r(t[i], qmax);
        if (smooth) {
            const double p = ((double)i + 0.5) / nd;
            double w = eu + (sigma * expm1(-khat * log1p(-p))) / khat;
            if (w > 1.0) w = 1.0;                     // (a NaN stays, as np.minimum)
            sw += w;
            swr += w / r;
        } else {
            sw += r;
        }
    }
    sw = block_sum(sw, s_wave);
    swr = block_sum(swr, s_wave);
    if (tid == 0) {
        if (!smooth) swr = nd;
        double body = 0.0;
        const double *__restrict__ p = a.part + col * a.chunks;
        for (long long ch = 0; ch < a.chunks; ++ch) body += p[ch];
        if (a.elpd) a.elpd[col] = (-0.5 * qmax + log((R - nd) + swr)) - log(body + sw);
        if (a.khat) a.khat[col] = khat;
        if (a.sigma) a.sigma[col] = sigma;
        if (a.ntail) a.ntail[col] = n;
    }
}

struct LooPlan {
    long long chunks;
    size_t thr_bytes, count_bytes, flag_bytes, part_bytes, tail_bytes, temp_bytes, need;
};

// checks the shape; QUIET: the workspace function only reports < 0
int make_plan(int64_t n, int64_t columns, int64_t tail_len, LooPlan &p, Voice v)
{
    if (n < 2 || columns < 1) return refuse(v, BISIP_EINVAL, "bad shape: %lld columns of %lld values", (long long)columns, (long long)n);
    if (tail_len < 1 || tail_len > n - 1)
        return refuse(v, BISIP_EINVAL, "tail_len=%lld outside [1, n - 1], n = %lld", (long long)tail_len, (long long)n);
    if (tail_len > LOO_MAX_TAIL)
        return refuse(v, BISIP_EUNSUPPORTED, "tail_len=%lld: more than %d profile points", (long long)tail_len, LOO_MAX_M);
    if (columns > 0x7fffffffLL || columns * tail_len > 0x7fffffffLL)
        return refuse(v, BISIP_EUNSUPPORTED, "tails of %lld values exceed the 2^31 items of one sort", (long long)(columns * tail_len));
    p.chunks = (n + LOO_CHUNK - 1) / LOO_CHUNK;
    BISIP_TRY(check_grid(p.chunks, columns, v, "%lld chunks of %lld columns", p.chunks, (long long)columns));
    p.thr_bytes = align256((size_t)2 * columns * 8);
    p.count_bytes = align256((size_t)columns * 4);
    p.flag_bytes = align256((size_t)columns * 4);
    p.part_bytes = align256((size_t)columns * p.chunks * 8);
    p.tail_bytes = align256((size_t)columns * tail_len * 8);
    p.temp_bytes = sort_scratch_bound(columns * tail_len, columns);
    p.need = p.thr_bytes + p.count_bytes + p.flag_bytes + p.part_bytes + 2 * p.tail_bytes + align256(p.temp_bytes);
    return BISIP_OK;
}

}  // namespace

extern "C" {

int bisip_q_columns_dev(bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, double *d_cols, int64_t rows_per_spectrum,
                        void *stream)
{
    if (!c) return fail(BISIP_EINVAL, "null context");
    if (!d_cols) return fail(BISIP_EINVAL, "null argument");
    if (n_spectra < 1 || rows_per_spectrum < 1) return fail(BISIP_EINVAL, "bad shape");
    if (first_spectrum < 0 || first_spectrum + n_spectra > c->E)
        return fail(BISIP_EINVAL, "spectra [%lld, %lld) of %d", (long long)first_spectrum, (long long)(first_spectrum + n_spectra), c->E);
    if ((uintptr_t)d_cols % 8) return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    QArgs a{};
    a.cols = d_cols; a.rows = rows_per_spectrum;
    a.chunks = (rows_per_spectrum + LOO_THREADS * QC_VPT - 1) / (LOO_THREADS * QC_VPT);
    a.N = c->N; a.rec = (int)(c->cb_stride / c->N);
    a.cb = c->d_cb + first_spectrum * c->cb_stride; a.cb_stride = c->cb_stride;
    const long long columns = n_spectra * 2 * c->N;
    BISIP_TRY(check_grid(a.chunks, columns, LOUD, "%lld chunks of %lld columns", a.chunks, columns));
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_q_columns, dim3((unsigned)(columns * a.chunks)), dim3(LOO_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int64_t bisip_loo_columns_workspace(int64_t n, int64_t columns, int64_t tail_len)
{
    LooPlan p{};
    if (make_plan(n, columns, tail_len, p, QUIET) != BISIP_OK) return -1;
    return (int64_t)p.need;
}

int bisip_loo_columns_dev(const double *d_q, int64_t n, int64_t columns, int64_t tail_len, double *d_elpd_rel, double *d_khat,
                          double *d_sigma, int64_t *d_ntail, void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_q || !d_work) return fail(BISIP_EINVAL, "null argument");
    if (!d_elpd_rel && !d_khat && !d_sigma && !d_ntail) return fail(BISIP_EINVAL, "no output asked for");
    LooPlan p{};
    BISIP_TRY(make_plan(n, columns, tail_len, p, LOUD));
    BISIP_TRY(check_workspace(d_work, work_bytes, (int64_t)p.need));
    if (((uintptr_t)d_q % 8) || ((uintptr_t)d_work % 8) || ((uintptr_t)d_elpd_rel % 8) || ((uintptr_t)d_khat % 8) ||
        ((uintptr_t)d_sigma % 8) || ((uintptr_t)d_ntail % 8))
        return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)d_work;
    double *thr = (double *)w; w += p.thr_bytes;
    unsigned *count = (unsigned *)w; w += p.count_bytes;
    int *flag = (int *)w; w += p.flag_bytes;
    double *part = (double *)w; w += p.part_bytes;
    double *tails = (double *)w; w += p.tail_bytes;
    double *sorted = (double *)w; w += p.tail_bytes;
    void *d_temp = w;

    // u = s[n - tail_len - 1] and qmax = s[n - 1], the order statistics themselves
    const std::vector<long long> lo{n - tail_len - 1, n - 1};
    const std::vector<double> t{0.0, 0.0};
    int rc = select_columns(d_q, n, columns, 2, lo, t, thr, st, columns, true);
    if (rc != BISIP_OK) return rc;
    HIP_TRY(hipMemsetAsync(count, 0, p.count_bytes + p.flag_bytes, st));      // (count and flag lie side by side)

    LooArgs a{};
    a.cols = d_q; a.n = n; a.columns = columns; a.M = tail_len; a.chunks = p.chunks;
    a.thr = thr; a.tails = tails; a.sorted = sorted; a.count = count; a.nan_flag = flag; a.part = part;
    a.elpd = d_elpd_rel; a.khat = d_khat; a.sigma = d_sigma; a.ntail = (long long *)d_ntail;
    hipLaunchKernelGGL(k_loo_compact, dim3((unsigned)(columns * p.chunks)), dim3(LOO_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    const long long items = columns * tail_len;
    hipLaunchKernelGGL(k_loo_fill, dim3((unsigned)((items + LOO_THREADS - 1) / LOO_THREADS)), dim3(LOO_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    rc = sort_segments(d_temp, p.temp_bytes, tails, sorted, items, columns, tail_len, st);
    if (rc != BISIP_OK) return rc;
    if (tail_len <= LOO_LDS_CAP)
        hipLaunchKernelGGL(k_loo_tail<true>, dim3((unsigned)columns), dim3(LOO_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(k_loo_tail<false>, dim3((unsigned)columns), dim3(LOO_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

}  // extern "C"
