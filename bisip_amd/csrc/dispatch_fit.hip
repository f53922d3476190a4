// dispatch_fit.hip -- per data point, over every spectrum's used samples of a device-resident chain, the mean and the
// variance of the squared standardised residual q = (y - Z)^2 / sigma^2 and the log of the mean of exp(-q / 2)
// (bisip_fit_quality_dev): what WAIC and the per-point misfit are made of.  Fused as dispatch_response.hip: the chain is
// read where it lies, the model is evaluated in registers and only a few running sums per (spectrum, segment, data point)
// exist -- no response and no q is ever written to memory.  The definitions are bisip_amd/fitquality.py (pointwise_q,
// fit_sums); fitquality.ordered_fit_sums restates the order of every sum below in NumPy: the same bits of mean_q and var_q
// from the same responses, and the same order of lmeh with NumPy's exp.
//
// Rows, plan, row slots, wave order, segments: row_pass.h.
//
//   * q = q_of_record of Z = M::eval, the bits of forward().  A row with a parameter that is not finite counts as q = NaN
//     at every point.
//   * Four states per (part, frequency) and lane -- S, P, m, s -- against the response kernel's two, so the frequencies go
//     in tiles of FQ_JT = 4: 32 doubles of state per lane, the chain is read again for every tile (from L2 / MALL after
//     the first), and no output depends on the tiling.  Resource report (-Rpass-analysis=kernel-resource-usage, gfx950):
//     162-247 VGPRs, no AGPRs, no scratch in any kernel of the unit; three waves per SIMD for PolynomialDecomposition of
//     degree 0 and 1, two for every other shape but five Cole-Cole modes (256 VGPRs + 4 AGPRs, one wave); k_fit_merge 50.
//   * mean_q, var_q: shifted sums.  c = q of walker 0 of the spectrum's first used sample, the same in every segment;
//     d = q - c;  S = S + d;  P = P + d * d, the product rounded on its own, each sum from 0.0.
//   * lmeh: a pair (m, s) per slot, m the smallest q so far and s = sum exp(-(q - m) / 2).  Empty: (+inf, 0).  A row q >= m:
//     s = s + exp(-(q - m) / 2).  A row q < m: s = s * exp(-(m - q) / 2) + 1, m = q (product and sum rounded on their own).
//     One exp (the device library's) per row.  Two pairs merge to m' = min(m_a, m_b); the side whose m is larger is scaled
//     by exp(-(m - m') / 2), the other (both, when the minima are equal) is not; s' = s_a + s_b.
//   * The pairs of the 256 slots and of the segments are merged in the order of the sums, the segments by k_fit_merge
//     (nseg > 1).
//   * mean_q = c + S / R;  var_q = (P - (S * S) / R) / (R - 1), < 0 becomes 0 (a NaN stays; R = 1 gives NaN);
//     lmeh = -m / 2 + log(s / R).
#include "row_pass.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int FQ_JT = 4;                      // frequencies per tile: 8 * FQ_JT doubles of state per lane

struct FqArgs : RowPass {
    double *mean_q, *var_q, *lmeh;   // (n_spectra, 2, N) each; any may be null
    double *part;                // (n_spectra, nseg, 8N): S, P, m, s of the 2N points each (nseg > 1)
    double *shift;               // (n_spectra, 2N): c, written by segment 0 (nseg > 1)
};

__device__ __forceinline__ double fq_scale(double d) { return exp(__dmul_rn(-0.5, d)); }

// (m, s) takes the row q
__device__ __forceinline__ void fq_row(double &m, double &s, double q)
{
    const bool lower = q < m;
    const double e = fq_scale(lower ? __dsub_rn(m, q) : __dsub_rn(q, m));
    s = lower ? __dadd_rn(__dmul_rn(s, e), 1.0) : __dadd_rn(s, e);   // (a NaN q fails the comparison and makes s NaN)
    if (lower) m = q;
}

// (m, s) = (m, s) merged with (mb, sb)
__device__ __forceinline__ void fq_merge(double &m, double &s, double mb, double sb)
{
    const bool a_hi = m > mb, b_hi = mb > m;
    const double e = fq_scale(a_hi ? __dsub_rn(m, mb) : __dsub_rn(mb, m));
    s = __dadd_rn(a_hi ? __dmul_rn(s, e) : s, b_hi ? __dmul_rn(sb, e) : sb);
    if (a_hi) m = mb;
}

__device__ __forceinline__ void fq_finish(const FqArgs &a, long long at, double c, double S, double P, double m, double s)
{
    const double R = (double)a.R;
    if (a.mean_q) a.mean_q[at] = __dadd_rn(c, __ddiv_rn(S, R));
    if (a.var_q) {
        double v = __ddiv_rn(__dsub_rn(P, __ddiv_rn(__dmul_rn(S, S), R)), __dsub_rn(R, 1.0));
        if (v < 0.0) v = 0.0;                                       // (a NaN fails the comparison and stays)
        a.var_q[at] = v;
    }
    if (a.lmeh) a.lmeh[at] = __dadd_rn(__dmul_rn(-0.5, m), log(__ddiv_rn(s, R)));
}

// grid (n_spectra * nseg): workgroup b takes segment b % nseg of spectrum b / nseg
template <class M>
__global__ __launch_bounds__(RM_THREADS) void k_fit_quality(const FqArgs a)
{
    constexpr int NDIM = M::NDIM, JT = FQ_JT, NV = 8 * JT;         // NV: states of a tile, what * 2 JT + part * JT + jj
    __shared__ double s_c[2 * JT];
    __shared__ double s_wave[4][NV];

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
        if (tid < JT && j0 + tid < N) {                             // the shift of this tile's points
            const double *rec = cb + (long long)(j0 + tid) * M::REC;
            double z0, z1, c0, c1;
            M::eval(s0, rec + 4, z0, z1);
            q_of_record(rec, z0, z1, c0, c1);
            s_c[tid] = c0;
            s_c[JT + tid] = c1;
        }
        __syncthreads();
        double S[2][JT], P[2][JT], Mn[2][JT], Sx[2][JT];
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) {
            S[0][jj] = S[1][jj] = P[0][jj] = P[1][jj] = Sx[0][jj] = Sx[1][jj] = 0.0;
            Mn[0][jj] = Mn[1][jj] = HUGE_VAL;
        }
        at.rewind();
#pragma unroll 1
        for (int i = tid; i < at.R; i += RM_THREADS) {
            double th[NDIM];
            const bool bad = load_row<NDIM>(at.row(), th);
            const typename M::Setup s = M::setup(th);
#pragma unroll
            for (int jj = 0; jj < JT; ++jj) {
                if (j0 + jj < N) {                                  // (uniform)
                    const double *rec = cb + (long long)(j0 + jj) * M::REC;
                    double z0, z1, q0, q1;
                    eval_const<M>(s, rec, z0, z1);
                    q_of_record(rec, z0, z1, q0, q1);
                    if (bad) q0 = q1 = __builtin_nan("");
                    const double d0 = __dsub_rn(q0, s_c[jj]), d1 = __dsub_rn(q1, s_c[JT + jj]);
                    S[0][jj] = __dadd_rn(S[0][jj], d0);
                    S[1][jj] = __dadd_rn(S[1][jj], d1);
                    P[0][jj] = __dadd_rn(P[0][jj], __dmul_rn(d0, d0));
                    P[1][jj] = __dadd_rn(P[1][jj], __dmul_rn(d1, d1));
                    fq_row(Mn[0][jj], Sx[0][jj], q0);
                    fq_row(Mn[1][jj], Sx[1][jj], q1);
                }
            }
            at.next();
        }
        // the pairs merged in the order of the sums: within a wave, then the four waves
#pragma unroll
        for (int v = 0; v < 2 * JT; ++v) {
            const int part = v / JT, jj = v % JT;
            const double xs = wave_sum(S[part][jj]), xp = wave_sum(P[part][jj]);
            double m = Mn[part][jj], s = Sx[part][jj];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double mb = __shfl_xor(m, d, 64), sb = __shfl_xor(s, d, 64);
                fq_merge(m, s, mb, sb);
            }
            if (lane == 0) {
                s_wave[wave][v] = xs;
                s_wave[wave][2 * JT + v] = xp;
                s_wave[wave][4 * JT + v] = m;
                s_wave[wave][6 * JT + v] = s;
            }
        }
        __syncthreads();
        if (tid < 2 * JT) {
            const int part = tid / JT, jj = tid - part * JT, j = j0 + jj;
            if (j < N) {
                const int vS = tid, vP = 2 * JT + tid, vM = 4 * JT + tid, vX = 6 * JT + tid;
                const double Ss = waves_in_order(s_wave, vS), Ps = waves_in_order(s_wave, vP);
                double m = s_wave[0][vM], s = s_wave[0][vX];
#pragma unroll
                for (int q = 1; q < 4; ++q) fq_merge(m, s, s_wave[q][vM], s_wave[q][vX]);
                if (a.nseg > 1) {
                    double *__restrict__ p = a.part + (e * a.nseg + g) * 8 * N;
                    p[part * N + j] = Ss;
                    p[(2 + part) * N + j] = Ps;
                    p[(4 + part) * N + j] = m;
                    p[(6 + part) * N + j] = s;
                    if (g == 0) a.shift[e * 2 * N + part * N + j] = s_c[tid];
                } else {
                    fq_finish(a, e * 2 * N + part * N + j, s_c[tid], Ss, Ps, m, s);
                }
            }
        }
        __syncthreads();                                            // s_c and s_wave are rewritten by the next tile
    }
}

// grid (n_spectra, ceil(2N / 256)): thread t merges the states of point t over the segments in ascending order
__global__ __launch_bounds__(RM_THREADS) void k_fit_merge(const FqArgs a)
{
    const long long e = blockIdx.x;
    const int t = blockIdx.y * RM_THREADS + threadIdx.x, N = a.N;
    if (t >= 2 * N) return;
    const double *__restrict__ p = a.part + e * a.nseg * 8 * N;
    double S = p[t], P = p[2 * N + t], m = p[4 * N + t], s = p[6 * N + t];
    for (long long g = 1; g < a.nseg; ++g) {
        const double *__restrict__ pg = p + g * 8 * N;
        S = __dadd_rn(S, pg[t]);
        P = __dadd_rn(P, pg[2 * N + t]);
        fq_merge(m, s, pg[4 * N + t], pg[6 * N + t]);
    }
    fq_finish(a, e * 2 * N + t, a.shift[e * 2 * N + t], S, P, m, s);
}

template <class M>
int launch_fit(const FqArgs &a, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL((k_fit_quality<M>), dim3(blocks), dim3(RM_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int dispatch_fit(const bisip_ctx *c, const FqArgs &a, unsigned blocks, hipStream_t st)
{
    return with_model(c, "fit-quality", [&](auto m) { return launch_fit<typename decltype(m)::type>(a, blocks, st); });
}

// bytes of the segments' states and the shifts; 0 with one segment, -1 when the grid does not exist
long long fit_workspace(const bisip_ctx *c, const RmPlan &p, int64_t n_spectra)
{
    if (p.nseg > 0x7fffffffLL / n_spectra) return -1;
    return p.nseg > 1 ? 8LL * n_spectra * (p.nseg * 8 + 2) * c->N : 0;
}

}  // namespace

extern "C" {

int64_t bisip_fit_quality_workspace(bisip_ctx *c, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble)
{
    if (check_response_shape(c, n_samples, n_spectra, walkers_per_ensemble) != BISIP_OK) return -1;
    return fit_workspace(c, rm_plan(n_samples, n_spectra, walkers_per_ensemble), n_spectra);
}

int bisip_fit_quality_dev(bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                          int64_t n_samples, int64_t sample_stride, int64_t walkers_per_ensemble, double *d_mean_q,
                          double *d_var_q, double *d_lmeh, void *d_work, int64_t work_bytes, void *stream)
{
    int rc = check_response_shape(c, n_samples, n_spectra, walkers_per_ensemble);
    if (rc != BISIP_OK) return rc;
    rc = check_row_buffers(c, first_spectrum, n_spectra, d_chain, sample_stride, walkers_per_ensemble,
                           {d_mean_q, d_var_q, d_lmeh}, "mean_q nor var_q nor lmeh", d_work);
    if (rc != BISIP_OK) return rc;
    RmPlan p;
    rc = plan_row_pass(c, n_samples, n_spectra, walkers_per_ensemble, fit_workspace, d_work, work_bytes, p);
    if (rc != BISIP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    FqArgs a{};
    fill_row_pass(a, c, first_spectrum, d_chain, sample_stride, walkers_per_ensemble, p);
    a.mean_q = d_mean_q; a.var_q = d_var_q; a.lmeh = d_lmeh;
    a.part = (double *)d_work;
    a.shift = (double *)d_work + n_spectra * p.nseg * 8 * c->N;
    rc = dispatch_fit(c, a, (unsigned)(n_spectra * p.nseg), st);
    if (rc != BISIP_OK || p.nseg == 1) return rc;
    return launch_per_point(k_fit_merge, n_spectra, 2 * c->N, st, a);
}

}  // extern "C"
