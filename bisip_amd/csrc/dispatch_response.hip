// dispatch_response.hip -- mean and standard deviation of the MODEL RESPONSE over every spectrum's used samples of a
// device-resident chain (bisip_response_moments_dev), fused: the chain is read where it lies, the model is evaluated in
// registers and only 4N running sums per (spectrum, segment) exist -- no response is ever written to memory.  The
// definitions are bisip_amd/response.py (response_pa, response_moments); response.ordered_response_moments restates the
// order of every sum below in NumPy and gives the same bits from the same responses.
//
// Rows.  Spectrum e owns R = n_samples * Wp rows of NDIM doubles, numbered r = k * Wp + w (sample k, walker w): the order
// of get_chain(flat=True).  Row r lies at d_chain + k * sample_stride + (e * Wp + w) * NDIM, e counted from the first
// spectrum of the call.
//
//   * Plan (rm_plan; response.plan): n_spectra >= 256 -> one segment of R rows per spectrum, ONE kernel, no workspace.
//     Else want = 2048 / n_spectra, seg_rows = max(1024, ceil(R / want)), nseg = ceil(R / seg_rows).  (A segment never
//     exceeds 2^30 rows.)  A function of the shape alone.
//   * A workgroup of 256 threads takes one (spectrum, segment); thread t is row slot t.  Row i of a segment (i from 0)
//     goes to slot i mod 256; a slot takes its rows in ascending order.
//   * 4N sums per lane do not fit the registers at N = 32 ... 64, so the frequencies go in tiles of RM_JT = 8: a pass over
//     the segment's rows keeps S and P of 8 frequencies x 2 parts (32 doubles) per lane, evaluates M::setup once per row
//     and M::eval for the tile's frequencies.  The chain is read again for every tile (N / 8 times, from L2 / MALL after
//     the first); a frequency's sums never depend on the tiling.  Resource report (-Rpass-analysis=kernel-resource-usage):
//     138-237 VGPRs, two or three waves per SIMD, no scratch, for every model but the PA kernels of 4 and 5 Cole-Cole
//     modes (256 VGPRs, one wave); with 16 frequencies per tile every transcendental model's kernel takes 256 VGPRs, copies
//     registers through AGPRs and holds one wave.
//   * Shifted sums.  c = the response (part, frequency) of walker 0 of the spectrum's first used sample, the same in every
//     segment; x = the response of the row, in the representation asked for (PA: hypot and -atan2 of the device library,
//     as k_forward_columns); d = x - c;  S = S + d;  P = P + d * d, the product rounded on its own (no fma), each sum
//     from 0.0.  A row with a parameter that is not finite counts as x = NaN in every (part, frequency).
//   * The 256 slots of a sum are added pairwise within each wave of 64 slots, 32, 16, ..., 1 apart; the four waves'
//     results then in ascending order ((w0 + w1) + w2) + w3.
//   * Segments are merged in ascending order S = (...((s_0 + s_1) + s_2) ...) by k_response_merge (nseg > 1).
//   * mean = c + S / R;  var = (P - (S * S) / R) / R, < 0 becomes 0 (a NaN stays);  std = sqrt(var).
#include "response_plan.h"                    // RM_THREADS, rm_plan, check_response_shape: shared with dispatch_fit.hip

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int RM_JT = 8;                      // frequencies per tile: 4 * RM_JT running sums per lane

struct RmArgs {
    const double *chain;         // walker 0 of the call's first spectrum in the first used sample
    long long stride, R, seg_rows, nseg;
    int Wp, N;
    const double *cb;            // records of the call's first spectrum
    long long cb_stride;
    double *mean, *std;          // (n_spectra, 2, N) each; either may be null
    double *part;                // (n_spectra, nseg, 4N): S re, S im, P re, P im (nseg > 1)
    double *shift;               // (n_spectra, 2N): c, written by segment 0 (nseg > 1)
};

template <bool PA>
__device__ __forceinline__ void rm_represent(double &x0, double &x1)
{
    if constexpr (PA) {
        const double amp = hypot(x0, x1), mph = -atan2(x1, x0);
        x0 = amp;
        x1 = mph;
    }
}

__device__ __forceinline__ void rm_finish(const RmArgs &a, long long at, double c, double S, double P)
{
    const double R = (double)a.R;
    if (a.mean) a.mean[at] = __dadd_rn(c, __ddiv_rn(S, R));
    if (a.std) {
        double v = __ddiv_rn(__dsub_rn(P, __ddiv_rn(__dmul_rn(S, S), R)), R);
        if (v < 0.0) v = 0.0;                                       // (a NaN fails the comparison and stays)
        a.std[at] = __dsqrt_rn(v);
    }
}

// grid (n_spectra * nseg): workgroup b takes segment b % nseg of spectrum b / nseg
template <class M, bool PA>
__global__ __launch_bounds__(RM_THREADS) void k_response_moments(const RmArgs a)
{
    constexpr int NDIM = M::NDIM, JT = RM_JT;
    __shared__ double s_c[2 * JT];
    __shared__ double s_wave[4][4 * JT];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, Wp = a.Wp;
    const long long e = blockIdx.x / a.nseg, g = blockIdx.x - e * a.nseg;
    const long long r0 = g * a.seg_rows;
    const int R = (int)(a.R - r0 < a.seg_rows ? a.R - r0 : a.seg_rows);
    const double *__restrict__ base = a.chain + e * Wp * NDIM;      // walker 0 of the spectrum in the first used sample
    const double *__restrict__ cb = a.cb + e * a.cb_stride;

    double th0[NDIM];
#pragma unroll
    for (int q = 0; q < NDIM; ++q) th0[q] = base[q];
    const typename M::Setup s0 = M::setup(th0);

    // this thread's first row: sample k0, walker w0; from one of its rows to the next
    const long long k0 = (r0 + tid) / Wp;
    const int w0 = (int)(r0 + tid - k0 * Wp);
    const int step_k = RM_THREADS / Wp, step_w = RM_THREADS - step_k * Wp;

    for (int j0 = 0; j0 < N; j0 += JT) {
        if (tid < JT && j0 + tid < N) {                             // the shift of this tile's frequencies
            double c0, c1;
            M::eval(s0, cb + (long long)(j0 + tid) * M::REC + 4, c0, c1);
            rm_represent<PA>(c0, c1);
            s_c[tid] = c0;
            s_c[JT + tid] = c1;
        }
        __syncthreads();
        double S[2][JT], P[2][JT];
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) S[0][jj] = S[1][jj] = P[0][jj] = P[1][jj] = 0.0;
        long long k = k0;
        int w = w0;
#pragma unroll 1
        for (int i = tid; i < R; i += RM_THREADS) {
            const double *__restrict__ row = base + k * a.stride + (long long)w * NDIM;
            double th[NDIM];
            bool bad = false;
#pragma unroll
            for (int q = 0; q < NDIM; ++q) {
                th[q] = row[q];
                bad |= !(fabs(th[q]) < HUGE_VAL);                   // NaN or +-inf
            }
            const typename M::Setup s = M::setup(th);
#pragma unroll
            for (int jj = 0; jj < JT; ++jj) {
                if (j0 + jj < N) {                                  // (uniform)
                    double x0, x1;
                    eval_const<M>(s, cb + (long long)(j0 + jj) * M::REC, x0, x1);
                    rm_represent<PA>(x0, x1);
                    if (bad) x0 = x1 = __builtin_nan("");
                    const double d0 = __dsub_rn(x0, s_c[jj]), d1 = __dsub_rn(x1, s_c[JT + jj]);
                    S[0][jj] = __dadd_rn(S[0][jj], d0);
                    S[1][jj] = __dadd_rn(S[1][jj], d1);
                    P[0][jj] = __dadd_rn(P[0][jj], __dmul_rn(d0, d0));
                    P[1][jj] = __dadd_rn(P[1][jj], __dmul_rn(d1, d1));
                }
            }
            k += step_k;
            w += step_w;
            if (w >= Wp) { w -= Wp; ++k; }
        }
        // the 64 slots of a wave pairwise, then the four waves in ascending order
#pragma unroll
        for (int v = 0; v < 4 * JT; ++v) {
            const int jj = v % JT, what = v / JT;                   // what: S re, S im, P re, P im
            double x = what < 2 ? S[what][jj] : P[what - 2][jj];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) x = __dadd_rn(x, __shfl_xor(x, m, 64));
            if (lane == 0) s_wave[wave][v] = x;
        }
        __syncthreads();
        if (tid < 2 * JT) {
            const int part = tid / JT, jj = tid - part * JT, j = j0 + jj;
            if (j < N) {
                const int vS = part * JT + jj, vP = (2 + part) * JT + jj;
                const double Ss = __dadd_rn(__dadd_rn(__dadd_rn(s_wave[0][vS], s_wave[1][vS]), s_wave[2][vS]), s_wave[3][vS]);
                const double Ps = __dadd_rn(__dadd_rn(__dadd_rn(s_wave[0][vP], s_wave[1][vP]), s_wave[2][vP]), s_wave[3][vP]);
                if (a.nseg > 1) {
                    double *__restrict__ p = a.part + (e * a.nseg + g) * 4 * N;
                    p[part * N + j] = Ss;
                    p[(2 + part) * N + j] = Ps;
                    if (g == 0) a.shift[e * 2 * N + part * N + j] = s_c[tid];
                } else {
                    rm_finish(a, e * 2 * N + part * N + j, s_c[tid], Ss, Ps);
                }
            }
        }
        __syncthreads();                                            // s_c and s_wave are rewritten by the next tile
    }
}

// grid (n_spectra, ceil(2N / 256)): thread t adds the sums of entry t over the segments in ascending order
__global__ __launch_bounds__(RM_THREADS) void k_response_merge(const RmArgs a)
{
    const long long e = blockIdx.x;
    const int t = blockIdx.y * RM_THREADS + threadIdx.x, N = a.N;
    if (t >= 2 * N) return;
    const double *__restrict__ p = a.part + e * a.nseg * 4 * N;
    double S = p[t], P = p[2 * N + t];
    for (long long g = 1; g < a.nseg; ++g) {
        S = __dadd_rn(S, p[g * 4 * N + t]);
        P = __dadd_rn(P, p[g * 4 * N + 2 * N + t]);
    }
    rm_finish(a, e * 2 * N + t, a.shift[e * 2 * N + t], S, P);
}

template <class M>
int launch_response(const RmArgs &a, unsigned blocks, int kind, hipStream_t st)
{
    if (kind == BISIP_RESPONSE_PA) hipLaunchKernelGGL((k_response_moments<M, true>), dim3(blocks), dim3(RM_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_response_moments<M, false>), dim3(blocks), dim3(RM_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int dispatch_response(const bisip_ctx *c, const RmArgs &a, unsigned blocks, int kind, hipStream_t st)
{
    return with_model(c, "response-moments", [&](auto m) { return launch_response<typename decltype(m)::type>(a, blocks, kind, st); });
}

// bytes of the segments' sums and the shifts; 0 with one segment, -1 when the grid does not exist
long long response_workspace(const bisip_ctx *c, const RmPlan &p, int64_t n_spectra)
{
    if (p.nseg > 0x7fffffffLL / n_spectra) return -1;
    return p.nseg > 1 ? 8LL * n_spectra * (p.nseg * 4 + 2) * c->N : 0;
}

}  // namespace

extern "C" {

int64_t bisip_response_moments_workspace(bisip_ctx *c, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble)
{
    if (check_response_shape(c, n_samples, n_spectra, walkers_per_ensemble) != BISIP_OK) return -1;
    return response_workspace(c, rm_plan(n_samples, n_spectra, walkers_per_ensemble), n_spectra);
}

int bisip_response_moments_dev(bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                               int64_t n_samples, int64_t sample_stride, int64_t walkers_per_ensemble, int kind,
                               double *d_mean, double *d_std, void *d_work, int64_t work_bytes, void *stream)
{
    int rc = check_response_shape(c, n_samples, n_spectra, walkers_per_ensemble);
    if (rc != BISIP_OK) return rc;
    if (kind != BISIP_RESPONSE_RI && kind != BISIP_RESPONSE_PA) return fail(BISIP_EINVAL, "unknown response kind %d", kind);
    if (!d_chain) return fail(BISIP_EINVAL, "null argument");
    if (!d_mean && !d_std) return fail(BISIP_EINVAL, "neither mean nor std asked for");
    if (first_spectrum < 0 || first_spectrum + n_spectra > c->E)
        return fail(BISIP_EINVAL, "spectra [%lld, %lld) of %d", (long long)first_spectrum, (long long)(first_spectrum + n_spectra), c->E);
    if (sample_stride < n_spectra * walkers_per_ensemble * c->ndim)
        return fail(BISIP_EINVAL, "sample_stride smaller than one sample");
    if (((uintptr_t)d_chain % 8) || ((uintptr_t)d_mean % 8) || ((uintptr_t)d_std % 8) || ((uintptr_t)d_work % 8))
        return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    const RmPlan p = rm_plan(n_samples, n_spectra, walkers_per_ensemble);
    const long long need = response_workspace(c, p, n_spectra);
    if (need < 0)
        return fail(BISIP_EUNSUPPORTED, "%lld segments of %lld spectra exceed one grid", p.nseg, (long long)n_spectra);
    if (need && (!d_work || work_bytes < need))
        return fail(BISIP_EINVAL, "workspace of %lld bytes, need %lld", (long long)(d_work ? work_bytes : 0), need);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    RmArgs a{};
    a.chain = d_chain; a.stride = sample_stride; a.R = p.R; a.seg_rows = p.seg_rows; a.nseg = p.nseg;
    a.Wp = (int)walkers_per_ensemble; a.N = c->N;
    a.cb = c->d_cb + first_spectrum * c->cb_stride; a.cb_stride = c->cb_stride;
    a.mean = d_mean; a.std = d_std;
    a.part = (double *)d_work;
    a.shift = (double *)d_work + n_spectra * p.nseg * 4 * c->N;
    rc = dispatch_response(c, a, (unsigned)(n_spectra * p.nseg), kind, st);
    if (rc != BISIP_OK) return rc;
    if (p.nseg > 1) {
        hipLaunchKernelGGL(k_response_merge, dim3((unsigned)n_spectra, (unsigned)((2 * c->N + RM_THREADS - 1) / RM_THREADS)),
                           dim3(RM_THREADS), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

}  // extern "C"
