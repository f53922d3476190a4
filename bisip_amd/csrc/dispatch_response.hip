// dispatch_response.hip -- mean and standard deviation of the MODEL RESPONSE over every spectrum's used samples of a
// device-resident chain (bisip_response_moments_dev), fused: the chain is read where it lies, the model is evaluated in
// registers and only 4N running sums per (spectrum, segment) exist -- no response is ever written to memory.  The
// definitions are bisip_amd/response.py (response_pa, response_moments); response.ordered_response_moments restates the
// order of every sum below in NumPy and gives the same bits from the same responses.
//
// Rows, plan, row slots, wave order, segments: row_pass.h.  One segment: ONE kernel, no workspace.
//
//   * 4N sums per lane do not fit the registers at N = 32 ... 64, so the frequencies go in tiles of RM_JT = 8: a pass over
//     the segment's rows keeps S and P of 8 frequencies x 2 parts (32 doubles) per lane, evaluates M::setup once per row
//     and M::eval for the tile's frequencies.  The chain is read again for every tile (N / 8 times, from L2 / MALL after
//     the first); a frequency's sums never depend on the tiling.  Resource report (-Rpass-analysis=kernel-resource-usage):
//     RI 138-255 VGPRs (three waves per SIMD for PolynomialDecomposition up to degree 5, else two), PA 196-255 (two), no
//     AGPRs and no scratch, for every model but the PA kernels of 4 and 5 Cole-Cole modes (256 VGPRs + 16 and 36 AGPRs,
//     one wave); k_response_merge 20; with 16 frequencies per tile every transcendental model's kernel takes 256 VGPRs,
//     copies registers through AGPRs and holds one wave.
//   * Shifted sums.  c = the response (part, frequency) of walker 0 of the spectrum's first used sample, the same in every
//     segment; x = the response of the row, in the representation asked for (PA: hypot and -atan2 of the device library,
//     as k_forward_columns); d = x - c;  S = S + d;  P = P + d * d, the product rounded on its own (no fma), each sum
//     from 0.0.  A row with a parameter that is not finite counts as x = NaN in every (part, frequency).
//   * Segments are merged by k_response_merge (nseg > 1).
//   * mean = c + S / R;  var = (P - (S * S) / R) / R, < 0 becomes 0 (a NaN stays);  std = sqrt(var).
#include "row_pass.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int RM_JT = 8;                      // frequencies per tile: 4 * RM_JT running sums per lane

struct RmArgs : RowPass {
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
    const int N = a.N;
    RowCursor<NDIM> at(a, blockIdx.x, tid);
    const long long e = at.e, g = at.g;
    const double *__restrict__ cb = at.cb;

    double th0[NDIM];
#pragma unroll
    for (int q = 0; q < NDIM; ++q) th0[q] = at.base[q];
    const typename M::Setup s0 = M::setup(th0);

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
        at.rewind();
#pragma unroll 1
        for (int i = tid; i < at.R; i += RM_THREADS) {
            double th[NDIM];
            const bool bad = load_row<NDIM>(at.row(), th);
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
            at.next();
        }
#pragma unroll
        for (int v = 0; v < 4 * JT; ++v) {
            const int jj = v % JT, what = v / JT;                   // what: S re, S im, P re, P im
            const double x = wave_sum(what < 2 ? S[what][jj] : P[what - 2][jj]);
            if (lane == 0) s_wave[wave][v] = x;
        }
        __syncthreads();
        if (tid < 2 * JT) {
            const int part = tid / JT, jj = tid - part * JT, j = j0 + jj;
            if (j < N) {
                const double Ss = waves_in_order(s_wave, part * JT + jj), Ps = waves_in_order(s_wave, (2 + part) * JT + jj);
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
    rc = check_row_buffers(c, first_spectrum, n_spectra, d_chain, sample_stride, walkers_per_ensemble, {d_mean, d_std},
                           "mean nor std", d_work);
    if (rc != BISIP_OK) return rc;
    RmPlan p;
    rc = plan_row_pass(c, n_samples, n_spectra, walkers_per_ensemble, response_workspace, d_work, work_bytes, p);
    if (rc != BISIP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    RmArgs a{};
    fill_row_pass(a, c, first_spectrum, d_chain, sample_stride, walkers_per_ensemble, p);
    a.mean = d_mean; a.std = d_std;
    a.part = (double *)d_work;
    a.shift = (double *)d_work + n_spectra * p.nseg * 4 * c->N;
    rc = dispatch_response(c, a, (unsigned)(n_spectra * p.nseg), kind, st);
    if (rc != BISIP_OK || p.nseg == 1) return rc;
    return launch_per_point(k_response_merge, n_spectra, 2 * c->N, st, a);
}

}  // extern "C"
