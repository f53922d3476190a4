// dispatch_predictive.hip -- posterior predictive checks of every spectrum over the used samples of a device-resident
// chain (bisip_predictive_check_dev).  The noise is Gaussian with known sigma, so a replicated standardised residual is
// standard normal whatever the sample is, and every check is the mean over the chain's rows of a closed-form function of
// the row's residuals: no random numbers.  Fused as dispatch_fit.hip: the chain is read where it lies, the model is
// evaluated in registers, no response and no residual is written to memory.  The definitions are
// bisip_amd/predictive.py (predictive_sums); predictive.ordered_predictive_sums restates the order of every sum below in
// NumPy: the same bits of chi2_mean and the same counts from the same responses, and the same order of pit, p_chi2 and
// p_max with glibc's functions in the place of the device library's.
//
// Rows, plan, row slots, wave order, segments: row_pass.h.  A slot adds every term to a sum that starts from 0.0; the
// segments are added by k_pred_finish, which divides by R.  Every term lies in [0, 1] or is >= 0: plain sums, no shift.
// Nothing is fused.
//
// Two passes over the chain, each evaluating the model (M::setup / eval_const, the bits of forward()):
//   * k_pred_rows, always: a row's frequencies in ascending order, one lane a row.  d and q: q_of_record (the bits of
//     fitquality.pointwise_q); T = sum of q, Re before Im of each frequency, from 0.0; qmax = max q; C = pairs of
//     adjacent frequencies, within Re and within Im, whose d < 0 differs.  A row with a parameter that is not finite or
//     whose T is not finite is BAD: it is counted per (spectrum, segment), takes no histogram bin, and k_pred_finish
//     makes every floating-point output of a spectrum with a bad row NaN.  A good row adds T, Q(N, T / 2) and
//     P(max of 2N |eps| >= sqrt(qmax)) to the three row sums and 1 to bin C of the workgroup's histogram in LDS (32-bit
//     integer atomics), which is added to the output (zeroed on the stream by the entry point) with 64-bit integer
//     atomics: any order gives the same counts.
//       Q(N, x) = exp(-x) sum_{k < N} x^k / k!, every term positive: x < N ascending from exp(-x) with factors x / k
//       (product, then quotient); x >= N descending from exp(((N - 1) log x - x) - log((N - 1)!)) with factors k / x;
//       a sum that rounds above 1 is 1.
//       p_max = -expm1(2N * log1p(-erfc(sqrt(qmax / 2)))).
//   * k_pred_points, when pit is asked for: h = sqrt(iv / 2), correctly rounded, once per point and tile (the halving is
//     exact: one rounding for sqrt(iv) / sqrt 2); a = d * h; Phi = erfc(-a) / 2: three roundings of erfc's argument.  One
//     double of state per point and lane, so the frequencies go in tiles of PC_JT = 8: 16 doubles of state per lane, the
//     chain is read again for every tile (from L2 / MALL after the first), and no output depends on the tiling.
// exp, log, log1p, expm1 and erfc are the device library's.  No floating-point atomics: the same bits on every call.
//
// Resource report (-Rpass-analysis=kernel-resource-usage, gfx950): no AGPRs and no scratch in any kernel of the unit.
//   k_pred_points: PolynomialDecomposition 116-126 VGPRs up to degree 5 (four waves per SIMD), 129-136 from degree 6 on
//     (three); Cole-Cole 140-168 with two to five modes (three waves) and 169 with one (two); Dias 149, Shin 142 (three).
//   k_pred_rows (exp, log, log1p, expm1, erfc and the two loops of Q inlined once): PolynomialDecomposition 147-163 up to
//     degree 3 (three waves), 169-193 from degree 4 on (two); Cole-Cole 178-251 (two); Dias 175 (two); Shin 168 (three).
//   k_pred_finish: 14 VGPRs.
#include "row_pass.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int PC_JT = 8;                      // frequencies per tile of the point pass: 2 * PC_JT doubles of state per lane
constexpr int PC_ROW_N_MAX = 700;             // above it exp(-x) underflows with x < N: the row outputs are refused

struct PcArgs : RowPass {
    double lgf;                  // log((N - 1)!)
    double *pit, *row;           // (n_spectra, 2, N), (n_spectra, 3); either may be null
    long long *hist;             // (n_spectra, 2N - 1); may be null
    double *part;                // (n_spectra, nseg, 2N + 4): the point sums, the three row sums, the count of bad rows
};

// Q(N, x), the regularised upper incomplete gamma function of an integer N >= 1
__device__ __forceinline__ double pc_chi2_sf(int N, double x, double lgf)
{
    double term, sum;
    if (x < (double)N) {
        term = sum = exp(-x);
#pragma unroll 1
        for (int k = 1; k < N; ++k) {
            term = __ddiv_rn(__dmul_rn(term, x), (double)k);
            sum = __dadd_rn(sum, term);
        }
    } else {
        term = sum = exp(__dsub_rn(__dsub_rn(__dmul_rn((double)(N - 1), log(x)), x), lgf));
#pragma unroll 1
        for (int k = N - 1; k >= 1; --k) {
            term = __ddiv_rn(__dmul_rn(term, (double)k), x);
            sum = __dadd_rn(sum, term);
        }
    }
    return sum > 1.0 ? 1.0 : sum;                                   // (N rounded terms can come out an ulp or so above 1)
}

__device__ __forceinline__ double pc_max_sf(double n_points, double qmax)
{
    const double e = erfc(__dsqrt_rn(__dmul_rn(0.5, qmax)));
    return -expm1(__dmul_rn(n_points, log1p(-e)));
}

// grid (n_spectra * nseg), (2N - 1) ints of dynamic LDS when the histogram is asked for: workgroup b takes segment
// b % nseg of spectrum b / nseg
template <class M>
__global__ __launch_bounds__(RM_THREADS) void k_pred_rows(const PcArgs a)
{
    constexpr int NDIM = M::NDIM;
    extern __shared__ int s_hist[];
    __shared__ double s_wave[4][3];
    __shared__ int s_bad;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, bins = 2 * N - 1;
    RowCursor<NDIM> at(a, blockIdx.x, tid);
    const long long e = at.e, g = at.g;
    const double *__restrict__ cb = at.cb;
    const bool want_hist = a.hist != nullptr, want_row = a.row != nullptr;    // (uniform)
    const double n_points = (double)(2 * N);

    if (want_hist)
        for (int c = tid; c < bins; c += RM_THREADS) s_hist[c] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();

    int n_bad = 0;
    double sT = 0.0, sQ = 0.0, sM = 0.0;
#pragma unroll 1
    for (int i = tid; i < at.R; i += RM_THREADS) {
        double th[NDIM];
        bool bad = load_row<NDIM>(at.row(), th);
        const typename M::Setup s = M::setup(th);
        double T = 0.0, qmax = 0.0;
        int C = 0;
        bool n0p = false, n1p = false;
#pragma unroll 1
        for (int j = 0; j < N; ++j) {
            const double *rec = cb + (long long)j * M::REC;
            double z0, z1, q0, q1, d0, d1;
            eval_const<M>(s, rec, z0, z1);
            q_of_record(rec, z0, z1, q0, q1, d0, d1);
            T = __dadd_rn(__dadd_rn(T, q0), q1);
            qmax = fmax(qmax, fmax(q0, q1));
            const bool n0 = d0 < 0.0, n1 = d1 < 0.0;
            if (j > 0) C += (int)(n0 != n0p) + (int)(n1 != n1p);
            n0p = n0;
            n1p = n1;
        }
        bad |= !(T < HUGE_VAL);                                     // (T >= 0, or NaN)
        double Q = 0.0, pm = 0.0;
        if (bad) {
            ++n_bad;
            T = Q = pm = __builtin_nan("");
        } else {
            if (want_hist) atomicAdd(&s_hist[C], 1);
            if (want_row) {
                Q = pc_chi2_sf(N, __dmul_rn(0.5, T), a.lgf);
                pm = pc_max_sf(n_points, qmax);
            }
        }
        sT = __dadd_rn(sT, T);
        sQ = __dadd_rn(sQ, Q);
        sM = __dadd_rn(sM, pm);
        at.next();
    }
    if (n_bad) atomicAdd(&s_bad, n_bad);
    sT = wave_sum(sT);
    sQ = wave_sum(sQ);
    sM = wave_sum(sM);
    if (lane == 0) {
        s_wave[wave][0] = sT;
        s_wave[wave][1] = sQ;
        s_wave[wave][2] = sM;
    }
    __syncthreads();
    double *__restrict__ p = a.part + (e * a.nseg + g) * (2 * N + 4) + 2 * N;
    if (tid < 3) p[tid] = waves_in_order(s_wave, tid);
    if (tid == 3) ((long long *)p)[3] = (long long)s_bad;
    if (want_hist) {
        long long *__restrict__ h = a.hist + e * bins;
        for (int c = tid; c < bins; c += RM_THREADS) {
            const int count = s_hist[c];
            if (count) atomicAdd((unsigned long long *)(h + c), (unsigned long long)count);
        }
    }
}

// grid (n_spectra * nseg): the sum of Phi over the segment's rows for every point, in tiles of PC_JT frequencies
template <class M>
__global__ __launch_bounds__(RM_THREADS) void k_pred_points(const PcArgs a)
{
    constexpr int NDIM = M::NDIM, JT = PC_JT, NV = 2 * JT;          // NV: states of a tile, part * JT + jj
    __shared__ double s_h[NV];
    __shared__ double s_wave[4][NV];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N;
    RowCursor<NDIM> at(a, blockIdx.x, tid);
    const double *__restrict__ cb = at.cb;
    double *__restrict__ p = a.part + (at.e * a.nseg + at.g) * (2 * N + 4);

    for (int j0 = 0; j0 < N; j0 += JT) {
        if (tid < NV) {                                             // h of this tile's points
            const int part = tid / JT, j = j0 + tid - part * JT;
            if (j < N) s_h[tid] = __dsqrt_rn(__dmul_rn(0.5, cb[(long long)j * M::REC + 2 + part]));
        }
        __syncthreads();
        double F[2][JT];
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) F[0][jj] = F[1][jj] = 0.0;
        at.rewind();
#pragma unroll 1
        for (int i = tid; i < at.R; i += RM_THREADS) {
            double th[NDIM];
            load_row<NDIM>(at.row(), th);                           // (a row that is not finite is k_pred_rows' to count)
            const typename M::Setup s = M::setup(th);
#pragma unroll
            for (int jj = 0; jj < JT; ++jj) {
                if (j0 + jj < N) {                                  // (uniform)
                    typedef const double __attribute__((address_space(4))) *const_ptr;
                    const double *rec = cb + (long long)(j0 + jj) * M::REC;
                    const const_ptr r = (const_ptr)rec;
                    double z0, z1;
                    eval_const<M>(s, rec, z0, z1);
                    const double a0 = __dmul_rn(__dsub_rn(r[0], z0), s_h[jj]);
                    const double a1 = __dmul_rn(__dsub_rn(r[1], z1), s_h[JT + jj]);
                    F[0][jj] = __dadd_rn(F[0][jj], __dmul_rn(0.5, erfc(-a0)));
                    F[1][jj] = __dadd_rn(F[1][jj], __dmul_rn(0.5, erfc(-a1)));
                }
            }
            at.next();
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const double x = wave_sum(F[v / JT][v % JT]);
            if (lane == 0) s_wave[wave][v] = x;
        }
        __syncthreads();
        if (tid < NV) {
            const int part = tid / JT, j = j0 + tid - part * JT;
            if (j < N) p[part * N + j] = waves_in_order(s_wave, tid);
        }
        __syncthreads();                                            // s_h and s_wave are rewritten by the next tile
    }
}

// grid (n_spectra, ceil((2N + 3) / 256)): thread t adds sum t of the segments in ascending order and divides by R; a
// spectrum with a bad row gets NaN
__global__ __launch_bounds__(RM_THREADS) void k_pred_finish(const PcArgs a)
{
    const long long e = blockIdx.x;
    const int t = blockIdx.y * RM_THREADS + threadIdx.x, N = a.N, width = 2 * N + 4;
    if (t >= 2 * N + 3) return;
    const bool point = t < 2 * N;
    if (point ? !a.pit : !a.row) return;
    const double *__restrict__ p = a.part + e * a.nseg * width;
    double s = p[t];
    long long bad = ((const long long *)p)[2 * N + 3];
    for (long long g = 1; g < a.nseg; ++g) {
        const double *__restrict__ pg = p + g * width;
        s = __dadd_rn(s, pg[t]);
        bad += ((const long long *)pg)[2 * N + 3];
    }
    const double v = bad ? __builtin_nan("") : __ddiv_rn(s, (double)a.R);
    if (point) a.pit[e * 2 * N + t] = v;
    else a.row[e * 3 + (t - 2 * N)] = v;
}

template <class M>
int launch_predictive(const PcArgs &a, unsigned blocks, hipStream_t st)
{
    const size_t lds = a.hist ? sizeof(int) * (size_t)(2 * a.N - 1) : 0;
    hipLaunchKernelGGL((k_pred_rows<M>), dim3(blocks), dim3(RM_THREADS), lds, st, a);
    HIP_TRY(hipGetLastError());
    if (a.pit) {
        hipLaunchKernelGGL((k_pred_points<M>), dim3(blocks), dim3(RM_THREADS), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

int dispatch_predictive(const bisip_ctx *c, const PcArgs &a, unsigned blocks, hipStream_t st)
{
    return with_model(c, "predictive-check", [&](auto m) { return launch_predictive<typename decltype(m)::type>(a, blocks, st); });
}

// bytes of the segments' sums; -1 when the grid does not exist
long long predictive_workspace(const bisip_ctx *c, const RmPlan &p, int64_t n_spectra)
{
    if (p.nseg > 0x7fffffffLL / n_spectra) return -1;
    return 8LL * n_spectra * p.nseg * (2LL * c->N + 4);
}

// log((N - 1)!) in long double, rounded once
double log_factorial(int n)
{
    long double s = 0.0L;
    for (int k = 2; k <= n; ++k) s += logl((long double)k);
    return (double)s;
}

}  // namespace

extern "C" {

int64_t bisip_predictive_check_workspace(bisip_ctx *c, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble)
{
    if (check_response_shape(c, n_samples, n_spectra, walkers_per_ensemble) != BISIP_OK) return -1;
    return predictive_workspace(c, rm_plan(n_samples, n_spectra, walkers_per_ensemble), n_spectra);
}

int bisip_predictive_check_dev(bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                               int64_t n_samples, int64_t sample_stride, int64_t walkers_per_ensemble, double *d_pit,
                               double *d_row, long long *d_sign_changes, void *d_work, int64_t work_bytes, void *stream)
{
    int rc = check_response_shape(c, n_samples, n_spectra, walkers_per_ensemble);
    if (rc != BISIP_OK) return rc;
    rc = check_row_buffers(c, first_spectrum, n_spectra, d_chain, sample_stride, walkers_per_ensemble,
                           {d_pit, d_row, d_sign_changes}, "pit nor row nor sign_changes", d_work);
    if (rc != BISIP_OK) return rc;
    if ((d_row || d_sign_changes) && c->N > PC_ROW_N_MAX)
        return fail(BISIP_EUNSUPPORTED, "the row outputs of N=%d frequencies (at most %d)", c->N, PC_ROW_N_MAX);
    RmPlan p;
    rc = plan_row_pass(c, n_samples, n_spectra, walkers_per_ensemble, predictive_workspace, d_work, work_bytes, p);
    if (rc != BISIP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    PcArgs a{};
    fill_row_pass(a, c, first_spectrum, d_chain, sample_stride, walkers_per_ensemble, p);
    a.lgf = log_factorial(c->N - 1);
    a.pit = d_pit; a.row = d_row; a.hist = d_sign_changes;
    a.part = (double *)d_work;
    if (d_sign_changes) HIP_TRY(hipMemsetAsync(d_sign_changes, 0, sizeof(long long) * (size_t)n_spectra * (2 * c->N - 1), st));
    rc = dispatch_predictive(c, a, (unsigned)(n_spectra * p.nseg), st);
    if (rc != BISIP_OK || !(d_pit || d_row)) return rc;
    return launch_per_point(k_pred_finish, n_spectra, 2 * c->N + 3, st, a);
}

}  // extern "C"
