// host.h -- what the translation units of libbisip_hip.so share: the layout of the QR-reduced tiers'
// operands, the walk over a chunk's half-steps and the draw kernels' launch shape, the context, the error plumbing and
// the dispatch entry points.  The kernels are templates, so every dispatch_*.hip instantiates only its own family and
// the units compile in parallel; the log-probability functor a sampler kernel takes is built from a context in one
// place for all of them (lp_build.h).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/bisip_hip.h"

namespace bisip {
namespace host {

// One spectrum's operands for one QR-reduced tier (0 plain, 1 compensated) as the kernels hold them: an entry of
// ReducedTier::image below, a kernel argument (fill_reduced), an element of the device array d_red -- all of them
// ReducedArgs<P, COMP> of kernels.h, to which the static_asserts beside fill_reduced tie this description for every
// degree.  In doubles, the compensated tier's low word of the triangle in front as floats, an even number of them
// (the doubles that follow stay aligned; the padding float is 0).  pack and unpack are the only functions that
// know the order of the fields.  Plain C++, no device: tests/native/sanitize_host.cpp runs them under the
// sanitizers (BISIP_HOST_LAYOUT_ONLY: this part of the header alone).
struct ReducedLayout {
    int n;                  // unknowns, P + 2
    size_t tri;             // entries of the packed upper triangle, row-major
    size_t lo_floats;       // tri, made even

    explicit constexpr ReducedLayout(int n_) : n(n_), tri((size_t)n_ * (n_ + 1) / 2), lo_floats((tri + 1) & ~(size_t)1) {}
    constexpr size_t doubles(int tier) const { return (tier == 1 ? lo_floats / 2 : 0) + tri + 3 * (size_t)n + 1; }

    // the triangle (and, tier 1, its low word) as full (n, n) matrices, the vectors, the scalar -> entry
    void pack(int tier, double *entry, const double *Rfull, const float *Rlo_full, const double *bhat, const double *e,
              const double *elo, double rest) const
    {
        if (tier == 1) {
            std::memset(entry, 0, lo_floats * sizeof(float));
            for (int i = 0, k = 0; i < n; ++i)
                for (int j = i; j < n; ++j, ++k) std::memcpy((char *)entry + k * sizeof(float), &Rlo_full[(size_t)i * n + j], sizeof(float));
            entry += lo_floats / 2;
        }
        for (int i = 0; i < n; ++i) entry = std::copy(Rfull + (size_t)i * n + i, Rfull + (size_t)i * n + n, entry);
        for (const double *v : {bhat, e, elo}) entry = std::copy(v, v + n, entry);
        *entry = rest;
    }

    // entry -> the packed triangle (and, tier 1, the tri floats of its low word), the vectors, the scalar
    void unpack(int tier, const double *entry, double *R, float *Rlo, double *bhat, double *e, double *elo, double *rest) const
    {
        if (tier == 1) {
            std::memcpy(Rlo, entry, tri * sizeof(float));
            entry += lo_floats / 2;
        }
        std::copy(entry, entry + tri, R);
        entry += tri;
        for (double *v : {bhat, e, elo}) { std::copy(entry, entry + n, v); entry += n; }
        *rest = *entry;
    }

    // a packed triangle (and its low word, if any) as the full (n, n) matrices the host emulation reads
    // (host_emulate.inc: reduced_chi2_kernel); zero below the diagonal
    void expand(const double *R, const float *Rlo, double *Rfull, float *Rlo_full) const
    {
        std::fill(Rfull, Rfull + (size_t)n * n, 0.0);
        if (Rlo) std::fill(Rlo_full, Rlo_full + (size_t)n * n, 0.0f);
        for (int i = 0, k = 0; i < n; ++i)
            for (int j = i; j < n; ++j, ++k) {
                Rfull[(size_t)i * n + j] = R[k];
                if (Rlo) Rlo_full[(size_t)i * n + j] = Rlo[k];
            }
    }
};

// A chunk of n_steps iterations, walked half-step by half-step, as every launch-per-half-step runner walks it
// (bisip_stretch_run_dev, the sharded runs, bisip_move_run_dev): where half h of iteration k finds its entries of the
// (n_steps, 2, nh) stream arrays, how many slots it has, and the chain rows it stores to.  Plain C++ as well.
struct ChunkWalk {
    int64_t W, ndim, n_steps, thin_by, nh;
    double *chain_row, *logp_row;     // row 0 of the chunk's stored chain (n_steps / thin_by, W, ndim) and (.., W), or null

    struct Half {
        int64_t off, n_slots;              // offset into the stream arrays; nh, or W / 2 in the smaller half
        double *chain_row, *logp_row;      // null unless the iteration is stored (and the chunk has the array)
    };

    ChunkWalk(int64_t W_, int64_t ndim_, int64_t n_steps_, int64_t thin_by_, double *chain_row_, double *logp_row_)
        : W(W_), ndim(ndim_), n_steps(n_steps_), thin_by(thin_by_), nh((W_ + 1) / 2), chain_row(chain_row_), logp_row(logp_row_) {}

    Half at(int64_t k, int h) const
    {
        const bool store = ((k + 1) % thin_by) == 0;   // the walkers of BOTH halves of a stored step
        const int64_t srow = k / thin_by;
        return Half{(k * 2 + h) * nh, h ? W / 2 : nh, (store && chain_row) ? chain_row + srow * W * ndim : nullptr,
                    (store && logp_row) ? logp_row + srow * W : nullptr};
    }
};

// The launch shape of a draw kernel (k_stretch_draw, k_move_draw) over `halves` half-steps of per_half slots each.
// GRID: x covers the slots of one half-step, (y, z) the half-steps -- the index arithmetic of a flat 64-bit grid was
// four 64-bit divisions per slot.  FLAT: one 32-bit index over everything (two 32-bit divisions), for ensembles too
// small to fill a workgroup per half-step.  The other two are refusals (launch_draw has their texts).  halves >= 1.
struct DrawGrid {
    enum Shape { FLAT, GRID, TOO_MANY_SLOTS, TOO_MANY_HALVES } shape;
    unsigned gx, gy, gz;
};

inline DrawGrid draw_grid(long long per_half, long long halves)
{
    if (per_half < 256 && per_half * halves + 256 <= 0xffffffffLL)
        return DrawGrid{DrawGrid::FLAT, (unsigned)((per_half * halves + 255) / 256), 1u, 1u};
    if ((per_half + 255) / 256 > 0x7fffffffLL) return DrawGrid{DrawGrid::TOO_MANY_SLOTS, 0u, 0u, 0u};
    const unsigned gy = (unsigned)(halves < 32768 ? halves : 32768);
    const long long gz = (halves + gy - 1) / gy;
    if (gz > 65535) return DrawGrid{DrawGrid::TOO_MANY_HALVES, 0u, 0u, 0u};
    return DrawGrid{DrawGrid::GRID, (unsigned)((per_half + 255) / 256), gy, (unsigned)gz};
}

}  // namespace host
}  // namespace bisip

#ifndef BISIP_HOST_LAYOUT_ONLY
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <type_traits>
#include <vector>

#include "errors.h"
#include "host_precompute.h"
#include "kernels.h"
#include "sampler_kernels.h"

namespace bisip {
namespace host {

constexpr int BLK_SMALL = 64;    // few walkers: spread them over more CUs
constexpr int BLK_LARGE = 256;
constexpr int BLK_STREAM = 128;  // HBM-bound reduced kernel: 128-lane workgroups stream ~3 % faster
                                 // than 256 (interleaved A/B, benchmarks/micro/reduced_variants.hip)
constexpr long long SMALL_W = 256LL * 256 * 2;  // below this, 64-lane workgroups
// From this polynomial degree on, the bulk launch of a lone spectrum's COMPENSATED reduced kernel reads its operands
// from memory through the scalar path, as a batch does, instead of taking them as kernel arguments: the triangle and
// its low words (99 scalars at degree 6, 171 at degree 9) no longer fit the scalar registers, and where kernel
// arguments are spilled into vector lanes (162 at degree 7), operands in memory are simply loaded again
// (measured at 2^23 walkers: +15 % at degree 6, +13 % at 7, +22 % at 8-9, +20 % at 10; equal at degree 5).
constexpr int REDUCED_COMP_MEMORY_OPERANDS_FROM = 6;
constexpr double BISIP_REDUCED_ERR_MAX = 1e-12;  // AUTO keeps the QR-reduced form below this estimate

// The model shapes that have kernels: the only lists of them (with_model and with_pd_degree below expand them)
#define PD_CASES(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
#define CC_CASES(X) X(1) X(2) X(3) X(4) X(5)
#define X(n) +1
static_assert(0 PD_CASES(X) == BISIP_MAX_POLY_DEG + 1, "PD_CASES lists the degrees 0 ... BISIP_MAX_POLY_DEG");
static_assert(0 CC_CASES(X) == BISIP_MAX_MODES, "CC_CASES lists the mode counts 1 ... BISIP_MAX_MODES");
#undef X

}  // namespace host
}  // namespace bisip

struct bisip_ctx {
    int device = 0, model_id = 0, N = 0, ndim = 0, variant = BISIP_VARIANT_AUTO;
    int P = 0, D = 0, S = 0;
    double c_exp = 1.0, lconst = 0.0;
    double auto_err_max = bisip::host::BISIP_REDUCED_ERR_MAX;   // AUTO keeps a QR-reduced tier whose estimate is below this
    bisip::Bounds bounds{};
    double lnw_min = 0.0, lnw_max = 0.0;   // over every frequency of every spectrum (bound_flags)
    bool grid_ok = false;                  // some spectrum's frequencies lie on a geometric grid (grid_step; BOUNDS_GRID; the loop is chosen per spectrum)
    int E = 1;                      // spectra in the context (batch of spectra: E > 1)
    double *d_cb = nullptr;        // records for k_forward (and k_logprob of CC/Dias/Shin): (E, N, REC)
    double *d_cb_lp = nullptr;     // PolynomialDecomposition: 1/sigma-weighted log-prob records (E, N, REC)
    double *d_cb_faithful = nullptr;
    double *d_lconst = nullptr;    // (E,)  batch; PolynomialDecomposition from degree 6 on
    long long cb_stride = 0;
    // QR-reduced form, two arithmetic tiers: [0] plain, [1] compensated (kernels.h:
    // logprob_row_reduced<P, COMP>); each has its own expansion point, and the compensated tier its own
    // operands (triangle, rest) from the QR carried out in binary128 (host_precompute.h: ReducedProblem)
    struct ReducedTier {
        double err = INFINITY;                  // worst estimated relative log-prob error over the spectra that RUN this tier; INFINITY: not estimated
        bool valid = false;                     // estimated for the current prior box (every spectrum that needs it)
        std::vector<double> image;              // (E,) entries of ReducedLayout, rewritten spectrum by spectrum: the one copy of the operands on the host
        void *d_red = nullptr;                  // the image on the device, where a kernel reads it from memory (reduced_image_on_device)
        std::vector<double> est;                // the estimate of every spectrum (tier 1: 0 where the spectrum does not run it)
        std::vector<unsigned char> done;        // per spectrum: estimated for the current box
    };
    ReducedTier red[2];
    // bisip_logprob measures the reduced kernel it ran on rows of its own batches (first call, then
    // every 2^n-th); a tier found wanting is closed to BISIP_VARIANT_AUTO until the box changes
    bool demoted[2] = {false, false};
    // A batch on BISIP_VARIANT_AUTO whose spectra do not all pass the plain tier launches the compensated
    // kernels with a tier per spectrum (BatchArgs::tier): tier_of[e] = 0 where the plain estimate of spectrum e
    // passes -- every spectrum runs what a context of its own would run, and only the others pay for the
    // compensated tier's operands and estimate.  mix_off: the guard closed the mix.
    std::vector<unsigned char> tier_of;
    unsigned char *d_tier = nullptr;
    bool mixed = false, mix_off = false;
    bool guard_on = true;
    int64_t guard_calls = 0, guard_checks = 0;
    double guard_worst = 0.0;
    int guard_escalations = 0;
    // per spectrum, for re-centring the reduced form when the prior box changes
    std::vector<bisip::ReducedProblem> reduced;
    // PolynomialDecomposition: host copies of what the compensated tier's binary128 operands are built from, on
    // demand (a spectrum that passes the plain tier never needs them)
    std::vector<double> h_w, h_zn, h_err, h_taus, h_log_taus;
    // workspace of the host-pointer entry points
    double *d_ws = nullptr;
    size_t ws_bytes = 0;
    double *d_gather = nullptr;    // sharded sampler: world slabs of ceil(slots/world) x (ndim+2)
    size_t gather_bytes = 0;
    double *d_packed = nullptr;    // big single ensembles: the chunk's state as one 64-byte row per walker (bisip_stretch_run_dev)
    size_t packed_bytes = 0;
    char *d_group = nullptr;       // multi-workgroup persistent sampler: 256 B of synchronisation words, then W rows of 64 B
    size_t group_bytes = 0;
    int64_t spectrum_offset = 0;   // batch: survey index of spectrum 0 (keys the Philox stream)
    // big host-buffer calls (bisip_logprob / bisip_forward): pinned double buffers, a second stream for the way
    // back, events per buffer (host_pipeline in bisip_hip.hip)
    char *h_pipe = nullptr;
    size_t pipe_bytes = 0;
    hipStream_t stream_back = nullptr;
    hipEvent_t pipe_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    char *h_pin = nullptr;         // pinned, device-mapped staging for small host-buffer calls
    char *d_pin = nullptr;         // its device-side address
    static constexpr size_t PIN_BYTES = 1 << 20;
    static constexpr size_t ZEROCOPY_BYTES = 64 << 10;
    hipStream_t stream = nullptr;
    const char *kernel_name = "";
};

namespace bisip {
namespace host {

int effective_variant(const bisip_ctx *c);
inline bool is_reduced(int v) { return v == BISIP_VARIANT_REDUCED || v == BISIP_VARIANT_REDUCED_COMP; }

// Which QR-reduced tier spectrum e runs now: 0 plain, 1 compensated, -1 neither (another formulation runs)
inline int running_tier(const bisip_ctx *c, size_t e)
{
    const int v = effective_variant(c);
    if (v == BISIP_VARIANT_REDUCED_COMP) return c->mixed ? c->tier_of[e] : 1;
    return v == BISIP_VARIANT_REDUCED ? 0 : -1;
}

// Does a tier's image go to the device (ReducedTier::d_red)?  Every tier of a batch; of a lone spectrum its
// compensated tier from degree REDUCED_COMP_MEMORY_OPERANDS_FROM on, where the bulk launch reads the operands from
// memory (dispatch_logprob.hip: launch_reduced).  For recenter_reduced, which uploads, and for build_context's
// constant that travels with the image (d_lconst); everybody else asks d_red.
inline bool reduced_image_on_device(const bisip_ctx *c, int tier)
{
    return c->E > 1 || (tier == 1 && c->P >= REDUCED_COMP_MEMORY_OPERANDS_FROM);
}

// ReducedLayout is the layout of ReducedArgs<P, COMP>, for every degree and both tiers
template <int P, bool COMP>
constexpr bool reduced_layout_is_the_kernels()
{
    using A = ReducedArgs<P, COMP>;
    using Plain = ReducedArgs<P, false>;
    constexpr ReducedLayout L(P + 2);
    static_assert(std::is_trivially_copyable<A>::value && alignof(A) == alignof(double) &&
                  sizeof(A) == sizeof(double) * L.doubles(COMP ? 1 : 0), "an entry is copied as bytes, doubles(tier) of them");
    // the plain struct is standard-layout: its offsets; the compensated one is the low word's floats, then the plain one
    static_assert(std::is_standard_layout<Plain>::value && offsetof(Plain, R) == 0 && offsetof(Plain, bhat) == 8 * L.tri &&
                  offsetof(Plain, e) == 8 * (L.tri + L.n) && offsetof(Plain, elo) == 8 * (L.tri + 2 * L.n) &&
                  offsetof(Plain, rest) == 8 * (L.tri + 3 * L.n), "order of the fields");
    static_assert(!COMP || (sizeof(ReducedLow<P, true>) == sizeof(float) * L.lo_floats &&
                            sizeof(A) == sizeof(ReducedLow<P, true>) + sizeof(Plain)), "the low word in front");
    return true;
}
#define X(p) static_assert(reduced_layout_is_the_kernels<p, false>() && reduced_layout_is_the_kernels<p, true>(), "ReducedLayout");
PD_CASES(X)
#undef X

// the kernel argument of a lone spectrum's launch: entry 0 of the image of the tier the kernel computes
template <int P, bool COMP>
inline void fill_reduced(const bisip_ctx *c, ReducedArgs<P, COMP> &r)
{
    std::memcpy(&r, c->red[COMP ? 1 : 0].image.data(), sizeof(r));
}

// A context's model shape as a template argument, for every host entry point that launches a model-templated kernel.
// with_model(c, what, f) returns f(ModelTag<M>{}), M = PDCollapsed<P>, ColeCole<D>, Dias or Shin;
// with_pd_degree(c, what, f) returns f(std::integral_constant<int, P>{}), for the PolynomialDecomposition formulations
// whose kernels are templated on the degree itself.  They know shapes, not policy: which formulation runs is the
// caller's business (effective_variant).  `what` names the kernel family in the error text.  build_context refuses
// every shape outside the lists, so the fall-throughs cannot be reached through the ABI: one code and one wording
// for all of them is no change of behaviour.
template <class M> struct ModelTag { using type = M; };

template <class F>
inline int with_pd_degree(const bisip_ctx *c, const char *what, F &&f)
{
    switch (c->P) {
#define X(p) case p: return f(std::integral_constant<int, p>{});
        PD_CASES(X)
#undef X
    }
    return fail(BISIP_EUNSUPPORTED, "no %s kernel for poly_deg=%d", what, c->P);
}

// a Cole-Cole mode count that comes without a context (a chain's, bisip_mode_order_dev): f(std::integral_constant<int, D>{})
template <class F>
inline int with_mode_count(int n_modes, const char *what, F &&f)
{
    switch (n_modes) {
#define X(d) case d: return f(std::integral_constant<int, d>{});
        CC_CASES(X)
#undef X
    }
    return fail(BISIP_EUNSUPPORTED, "no %s kernel for n_modes=%d", what, n_modes);
}

template <class F>
inline int with_model(const bisip_ctx *c, const char *what, F &&f)
{
    switch (c->model_id) {
    case BISIP_MODEL_POLYDECOMP:
        switch (c->P) {
#define X(p) case p: return f(ModelTag<PDCollapsed<p>>{});
            PD_CASES(X)
#undef X
        }
        return fail(BISIP_EUNSUPPORTED, "no %s kernel for poly_deg=%d", what, c->P);
    case BISIP_MODEL_COLECOLE:
        switch (c->D) {
#define X(d) case d: return f(ModelTag<ColeCole<d>>{});
            CC_CASES(X)
#undef X
        }
        return fail(BISIP_EUNSUPPORTED, "no %s kernel for n_modes=%d", what, c->D);
    case BISIP_MODEL_DIAS2000: return f(ModelTag<Dias>{});
    case BISIP_MODEL_SHIN2015: return f(ModelTag<Shin>{});
    }
    return fail(BISIP_EUNSUPPORTED, "no %s kernel for model_id=%d", what, c->model_id);
}

// a runtime flag as a template argument: f(std::bool_constant<b>{})
template <class F>
inline auto with_flag(bool b, F &&f)
{
    if (b) return f(std::bool_constant<true>{});
    return f(std::bool_constant<false>{});
}

LaunchArgs make_args(const bisip_ctx *c, const double *theta, double *out, int64_t W, const double *cb);
BatchArgs make_batch_args(const bisip_ctx *c, const double *theta, double *out, int64_t W);

// Lanes per walker for launches that cannot fill the chip with one lane per walker
// (dispatch_logprob.hip); the value never changes a result, only the wave count.
int lanes_per_walker(long long walkers);
// models whose frequency loop is too cheap to split over lanes
template <class M> struct CoopLimit { static constexpr long long value = 1LL << 40; };
// PDCollapsed spends 15 FMAs per frequency: passing the running sums between lanes costs as
// much as the residual it parallelises (measured 5.7 vs 5.2 us at 4096 walkers), so one lane.
template <int P> struct CoopLimit<PDCollapsed<P>> { static constexpr long long value = 0; };

// dispatch_logprob.hip / dispatch_forward.hip
int dispatch_logprob(const bisip_ctx *c, const double *theta, int64_t W, double *out, hipStream_t st);
int dispatch_forward(const bisip_ctx *c, const double *theta, int64_t W, double *Z, hipStream_t st, long long spectrum = -1,
                     long long count = 1);
int dispatch_forward_columns(const bisip_ctx *c, const double *theta, int64_t W, double *cols, hipStream_t st, long long spectrum,
                             long long count, int kind = BISIP_RESPONSE_RI);

// The refusals in front of every walk over a chunk (ChunkWalk).  own_range: the caller states W and the step range
// itself, in its own words (the Philox entry points, which bound both by the counter's 32-bit words).
inline int check_chunk(int64_t W, int64_t n_steps, int64_t thin_by, bool own_range = false)
{
    if (thin_by < 1 || n_steps % thin_by) return fail(BISIP_EINVAL, "n_steps=%lld must be a multiple of thin_by=%lld", (long long)n_steps, (long long)thin_by);
    if (!own_range && (W < 2 || n_steps < 0)) return fail(BISIP_EINVAL, "bad W=%lld or n_steps=%lld", (long long)W, (long long)n_steps);
    return BISIP_OK;
}

// what every draw kernel's arguments start with (sampler_kernels.h: DrawHead), but for the launch shape
inline DrawHead draw_head(const bisip_ctx *c, int64_t W, uint64_t seed, int64_t step0, int64_t n_steps, const int32_t *d_perm)
{
    DrawHead d;
    d.W = W; d.nh = (W + 1) / 2; d.n_steps = n_steps; d.step0 = step0; d.E = c->E; d.e0 = c->spectrum_offset;
    d.flat = 0;
    d.seed_lo = (unsigned int)(seed & 0xffffffffu); d.seed_hi = (unsigned int)(seed >> 32);
    d.perm = d_perm;
    return d;
}

// one launch of a draw kernel over arguments that begin with a DrawHead `s`, in the shape draw_grid chooses
template <class Args>
int launch_draw(long long per_half, long long halves, void (*kernel)(Args), Args d, hipStream_t st)
{
    const DrawGrid g = draw_grid(per_half, halves);
    if (g.shape == DrawGrid::TOO_MANY_SLOTS) return fail(BISIP_EINVAL, "too many slots per half-step");
    if (g.shape == DrawGrid::TOO_MANY_HALVES) return fail(BISIP_EINVAL, "n_steps=%lld too large for one draw (chunk the run)", halves / 2);
    d.s.flat = g.shape == DrawGrid::FLAT;
    hipLaunchKernelGGL(kernel, dim3(g.gx, g.gy, g.gz), dim3(256), 0, st, d);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

// dispatch_stretch.hip
enum StretchKind { STRETCH_HALF, STRETCH_EVAL, STRETCH_PERSIST, STRETCH_GROUP };

// what one stretch dispatch launches: a half-step / eval kernel over StretchArgs, or the
// persistent kernel over PersistArgs
struct StretchWork {
    StretchKind kind;
    const StretchArgs *half;
    const PersistArgs *persist;
};

StretchArgs to_device_args(const bisip_stretch_args *u);
int dispatch_stretch(const bisip_ctx *c, const StretchWork &a, long long Wp, hipStream_t st);
int dispatch_stretch_batch(const bisip_ctx *c, const StretchWork &a, long long Wp, hipStream_t st);   // dispatch_stretch_batch.hip
int dispatch_apply(const bisip_ctx *c, const StretchArgs &a, hipStream_t st);

}  // namespace host
}  // namespace bisip
#endif  // BISIP_HOST_LAYOUT_ONLY
