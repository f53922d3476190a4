// row_pass.h -- what the fused passes over a device-resident chain share (dispatch_response.hip, dispatch_fit.hip,
// dispatch_predictive.hip): each evaluates the model on every stored row where the chain lies and keeps only running sums.
// include/bisip_hip.h states the order of every sum; bisip_amd/response.py restates the plan (plan).
//
// Rows.  Spectrum e owns R = n_samples * Wp rows of NDIM doubles, numbered r = k * Wp + w (sample k, walker w): the order
// of get_chain(flat=True).  Row r lies at d_chain + k * sample_stride + (e * Wp + w) * NDIM, e counted from the first
// spectrum of the call.
//   * Plan (rm_plan): n_spectra >= 256 -> one segment of R rows per spectrum.  Else want = 2048 / n_spectra,
//     seg_rows = max(1024, ceil(R / want)), nseg = ceil(R / seg_rows).  (A segment never exceeds 2^30 rows.)  A function
//     of the shape alone.
//   * Slots.  A workgroup of 256 threads takes one (spectrum, segment): workgroup b of a grid of n_spectra * nseg takes
//     segment b % nseg of spectrum b / nseg; thread t is row slot t.  Row i of a segment (i from 0) goes to slot i mod 256;
//     a slot takes its rows in ascending order (RowCursor).  A kernel that holds its frequencies in tiles walks the
//     segment once per tile: the chain is read again (from L2 / MALL after the first), no sum depends on the tiling.
//   * A row with a parameter that is not finite (load_row) counts as NaN in whatever the pass sums.
//   * Wave order.  The 256 slots of a sum are added pairwise within each wave of 64 slots, 32, 16, ..., 1 apart (wave_sum);
//     the four waves' results then in ascending order ((w0 + w1) + w2) + w3 (waves_in_order).
//   * Segments are merged in ascending order (...((s_0 + s_1) + s_2) ...) by the unit's own kernel of one thread per
//     entry (launch_per_point), from a workspace of the unit's own layout.
#pragma once
#include <initializer_list>

#include "host.h"

namespace bisip {
namespace host {

constexpr int RM_THREADS = 256;               // row slots of a (spectrum, segment): one workgroup
constexpr long long RM_WGS = 2048;            // workgroups wanted of few spectra
constexpr long long RM_SEG_MIN = 1024;        // rows of a segment at least
constexpr long long RM_ONE_SEGMENT = 256;     // spectra from which a workgroup per spectrum fills the chip
constexpr long long RM_SEG_MAX = 1LL << 30;   // rows of a segment at most: 32-bit row numbers inside it

struct RmPlan {
    long long R, seg_rows, nseg;
};

inline RmPlan rm_plan(long long n, long long E, long long Wp)
{
    RmPlan p{};
    p.R = n * Wp;
    if (E >= RM_ONE_SEGMENT) {
        p.seg_rows = p.R;
    } else {
        const long long want = RM_WGS / E;
        p.seg_rows = (p.R + want - 1) / want;
        if (p.seg_rows < RM_SEG_MIN) p.seg_rows = RM_SEG_MIN;
    }
    if (p.seg_rows > RM_SEG_MAX) p.seg_rows = RM_SEG_MAX;
    p.nseg = (p.R + p.seg_rows - 1) / p.seg_rows;
    return p;
}

// what every kernel of a pass is told of the chain and the records; a unit's argument struct derives from it
struct RowPass {
    const double *chain;         // walker 0 of the call's first spectrum in the first used sample
    long long stride, R, seg_rows, nseg;
    int Wp, N;
    const double *cb;            // records of the call's first spectrum
    long long cb_stride;
};

// -- an entry point's checks, in the order they are reported in: check_response_shape, (the unit's own), check_row_buffers,
// (the unit's own), plan_row_pass ----------------------------------------------------------------------------------------
inline int check_response_shape(const bisip_ctx *c, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble)
{
    if (!c) return fail(BISIP_EINVAL, "null context");
    if (n_samples < 1 || n_samples > 0x7fffffffLL || n_spectra < 1 || n_spectra > c->E || walkers_per_ensemble < 1 ||
        walkers_per_ensemble > 0x7fffffffLL / (2 * BISIP_MAX_NDIM))
        return fail(BISIP_EINVAL, "bad chain shape");
    return BISIP_OK;
}

// the chain, the outputs (any may be null, not all: "neither <outs_named> asked for"), the spectra, the stride, alignment
inline int check_row_buffers(const bisip_ctx *c, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                             int64_t sample_stride, int64_t walkers_per_ensemble, std::initializer_list<const void *> outs,
                             const char *outs_named, const void *d_work)
{
    if (!d_chain) return fail(BISIP_EINVAL, "null argument");
    bool asked = false, aligned = !((uintptr_t)d_chain % 8) && !((uintptr_t)d_work % 8);
    for (const void *o : outs) {
        asked |= o != nullptr;
        aligned &= !((uintptr_t)o % 8);
    }
    if (!asked) return fail(BISIP_EINVAL, "neither %s asked for", outs_named);
    if (first_spectrum < 0 || first_spectrum + n_spectra > c->E)
        return fail(BISIP_EINVAL, "spectra [%lld, %lld) of %d", (long long)first_spectrum, (long long)(first_spectrum + n_spectra), c->E);
    if (sample_stride < n_spectra * walkers_per_ensemble * c->ndim)
        return fail(BISIP_EINVAL, "sample_stride smaller than one sample");
    if (!aligned) return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    return BISIP_OK;
}

// the plan of a shape that has passed check_response_shape, held against one grid and against the workspace the unit's own
// rule asks for (bytes; 0: none; -1: the grid does not exist); then the context's device is made current
inline int plan_row_pass(const bisip_ctx *c, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble,
                         long long (*workspace)(const bisip_ctx *, const RmPlan &, int64_t), const void *d_work,
                         int64_t work_bytes, RmPlan &p)
{
    p = rm_plan(n_samples, n_spectra, walkers_per_ensemble);
    const long long need = workspace(c, p, n_spectra);
    if (need < 0)
        return fail(BISIP_EUNSUPPORTED, "%lld segments of %lld spectra exceed one grid", p.nseg, (long long)n_spectra);
    if (need && (!d_work || work_bytes < need))
        return fail(BISIP_EINVAL, "workspace of %lld bytes, need %lld", (long long)(d_work ? work_bytes : 0), need);
    HIP_TRY(hipSetDevice(c->device));
    return BISIP_OK;
}

inline void fill_row_pass(RowPass &a, const bisip_ctx *c, int64_t first_spectrum, const double *d_chain, int64_t sample_stride,
                          int64_t walkers_per_ensemble, const RmPlan &p)
{
    a.chain = d_chain; a.stride = sample_stride; a.R = p.R; a.seg_rows = p.seg_rows; a.nseg = p.nseg;
    a.Wp = (int)walkers_per_ensemble; a.N = c->N;
    a.cb = c->d_cb + first_spectrum * c->cb_stride; a.cb_stride = c->cb_stride;
}

// grid (n_spectra, ceil(entries / 256)): a merge kernel's thread blockIdx.y * 256 + threadIdx.x takes one entry of a spectrum
template <class K, class A>
int launch_per_point(K kernel, int64_t n_spectra, int entries, hipStream_t st, const A &a)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_spectra, (unsigned)((entries + RM_THREADS - 1) / RM_THREADS)), dim3(RM_THREADS), 0,
                       st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

// -- device side ---------------------------------------------------------------------------------------------------------
// Where the workgroup and the thread stand: spectrum e, segment g of R rows, the spectrum's walker 0 in the first used
// sample (base) and its records (cb); row() is the slot's current row, from its first in the segment.  The loop stays
// the kernel's:  #pragma unroll 1  for (int i = tid; i < at.R; i += RM_THREADS) { ... at.row() ...; at.next(); }
template <int NDIM>
struct RowCursor {
    long long e, g;
    int R;
    const double *__restrict__ base;
    const double *__restrict__ cb;
    long long stride, k0, k;     // k, w: sample and walker of the current row; k0, w0: of the slot's first
    int Wp, w0, w, step_k, step_w;

    __device__ __forceinline__ RowCursor(const RowPass &a, unsigned block, int tid)
    {
        Wp = a.Wp;
        stride = a.stride;
        e = block / a.nseg;
        g = block - e * a.nseg;
        const long long r0 = g * a.seg_rows;
        R = (int)(a.R - r0 < a.seg_rows ? a.R - r0 : a.seg_rows);
        base = a.chain + e * Wp * NDIM;
        cb = a.cb + e * a.cb_stride;
        k = k0 = (r0 + tid) / Wp;
        w = w0 = (int)(r0 + tid - k0 * Wp);
        step_k = RM_THREADS / Wp;                                   // from one of the slot's rows to the next
        step_w = RM_THREADS - step_k * Wp;
    }
    __device__ __forceinline__ const double *row() const { return base + k * stride + (long long)w * NDIM; }
    __device__ __forceinline__ void next()
    {
        k += step_k;
        w += step_w;
        if (w >= Wp) { w -= Wp; ++k; }
    }
    __device__ __forceinline__ void rewind() { k = k0; w = w0; }
};

// th = the row's parameters; true when one of them is NaN or +-inf
template <int NDIM>
__device__ __forceinline__ bool load_row(const double *__restrict__ row, double (&th)[NDIM])
{
    bool bad = false;
#pragma unroll
    for (int q = 0; q < NDIM; ++q) {
        th[q] = row[q];
        bad |= !(fabs(th[q]) < HUGE_VAL);
    }
    return bad;
}

// (wave_sum is kernels.h's: the xor-shuffle sum 32 ... 1, one rounded addition each)
// entry v of the four waves' results s_wave[wave][v]
template <int NV>
__device__ __forceinline__ double waves_in_order(const double (&s_wave)[4][NV], int v)
{
    return __dadd_rn(__dadd_rn(__dadd_rn(s_wave[0][v], s_wave[1][v]), s_wave[2][v]), s_wave[3][v]);
}

// q = (y - Z)^2 / sigma^2 of both parts of one frequency from the response (z0, z1) and the record rec[0..3] = y_re, y_im,
// 1/s2_re, 1/s2_im:  d = y - Z;  t = d * d;  q = t * iv, each rounded on its own (no fma)
__device__ __forceinline__ void q_of_record(const double *rec, double z0, double z1, double &q0, double &q1, double &d0, double &d1)
{
    typedef const double __attribute__((address_space(4))) *const_ptr;   // scalar loads, as eval_const
    const const_ptr r = (const_ptr)rec;
    d0 = __dsub_rn(r[0], z0);
    d1 = __dsub_rn(r[1], z1);
    q0 = __dmul_rn(__dmul_rn(d0, d0), r[2]);
    q1 = __dmul_rn(__dmul_rn(d1, d1), r[3]);
}

__device__ __forceinline__ void q_of_record(const double *rec, double z0, double z1, double &q0, double &q1)
{
    double d0, d1;
    q_of_record(rec, z0, z1, q0, q1, d0, d1);
}

}  // namespace host
}  // namespace bisip
