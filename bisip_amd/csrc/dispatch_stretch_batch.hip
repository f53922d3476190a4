// dispatch_stretch_batch.hip -- stretch-move launches for a batch of spectra (one context, E
// ensembles): half-step and persistent kernels over BatchGenericLP / BatchReducedLP.
#include "stretch_launch.h"

using namespace bisip;
using namespace bisip::host;

namespace {

template <class M, bool U, int L>
int stretch_generic_batch_l(const bisip_ctx *c, const StretchWork &a, long long Wp, hipStream_t st)
{
    BatchGenericLP<M, U, L> lp;
    lp.cb = c->d_cb_lp ? c->d_cb_lp : c->d_cb; lp.cb_stride = c->cb_stride; lp.Wp = Wp; lp.lconst = c->d_lconst; lp.N = c->N;
    lp.b = c->bounds;
    return launch_stretch(a, lp, st);
}

// u: every wave of 64 slots lies inside one spectrum (dispatch_stretch_batch), the kernels' U argument
template <class M>
int stretch_generic_batch(const bisip_ctx *c, const StretchWork &a, long long Wp, bool u, hipStream_t st)
{
    return with_flag(u, [&](auto uniform) {
        constexpr bool U = uniform;
        // a wave of 64/L slots must stay inside one spectrum for the uniform (scalar) operand path
        // (the persistent kernel's workgroup is one ensemble: always inside one spectrum)
        if constexpr (CoopLimit<M>::value > 0) {      // (models whose frequency loop is too cheap to split have one lane per slot: no other kernels exist)
            const int want = stretch_lanes(a);
            const bool whole = !U || a.kind == STRETCH_PERSIST;
            if (want == 4 && (whole || (Wp / 2) % 16 == 0)) return stretch_generic_batch_l<M, U, 4>(c, a, Wp, st);
            if (want >= 2 && (whole || (Wp / 2) % 32 == 0)) return stretch_generic_batch_l<M, U, 2>(c, a, Wp, st);
        }
        return stretch_generic_batch_l<M, U, 1>(c, a, Wp, st);
    });
}

template <int P, bool COMP>
int stretch_reduced_batch(const bisip_ctx *c, const StretchWork &a, long long Wp, bool u, hipStream_t st)
{
    return with_flag(u, [&](auto uniform) {
        BatchReducedLP<P, uniform, COMP> lp;
        lp.red = reinterpret_cast<const ReducedArgs<P, COMP> *>(c->red[COMP ? 1 : 0].d_red); lp.Wp = Wp; lp.lconst = c->d_lconst;
        lp.red_plain = reinterpret_cast<const ReducedArgs<P, false> *>(c->red[0].d_red);
        lp.tier = COMP && c->mixed ? c->d_tier : nullptr;
        lp.b = c->bounds;
        return launch_stretch(a, lp, st);
    });
}

}  // namespace

namespace bisip {
namespace host {

// batch of spectra: Wp walkers per spectrum; a wave of 64 slots stays inside one spectrum
// iff (Wp/2) % 64 == 0
int dispatch_stretch_batch(const bisip_ctx *c, const StretchWork &a, long long Wp, hipStream_t st)
{
    // in the persistent kernel a workgroup IS one ensemble, so the spectrum is always uniform
    const bool u = (Wp % 128) == 0 || a.kind == STRETCH_PERSIST;
    if (c->model_id == BISIP_MODEL_POLYDECOMP) {
        const int v = effective_variant(c);
        if (v == BISIP_VARIANT_REDUCED) return with_pd_degree(c, "batch stretch", [&](auto p) { return stretch_reduced_batch<p, false>(c, a, Wp, u, st); });
        if (v == BISIP_VARIANT_REDUCED_COMP) return with_pd_degree(c, "batch stretch", [&](auto p) { return stretch_reduced_batch<p, true>(c, a, Wp, u, st); });
    }
    return with_model(c, "batch stretch", [&](auto m) { return stretch_generic_batch<typename decltype(m)::type>(c, a, Wp, u, st); });
}

}  // namespace host
}  // namespace bisip
