// dispatch_moves_batch.hip -- differential-evolution and snooker half-steps for a batch of spectra (one context,
// E ensembles): k_move_half over BatchGenericLP / BatchReducedLP.
#include "move_launch.h"

using namespace bisip;
using namespace bisip::host;

namespace {

template <class M, bool U, int L>
int move_generic_batch_l(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, hipStream_t st)
{
    BatchGenericLP<M, U, L> lp;
    lp.cb = c->d_cb_lp ? c->d_cb_lp : c->d_cb; lp.cb_stride = c->cb_stride; lp.Wp = Wp; lp.lconst = c->d_lconst; lp.N = c->N;
    lp.b = c->bounds;
    return launch_move(a, kind, lp, st);
}

// u: every wave of 64 slots lies inside one spectrum (dispatch_move_batch), the kernels' U argument
template <class M>
int move_generic_batch(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, bool u, hipStream_t st)
{
    return with_flag(u, [&](auto uniform) {
        constexpr bool U = uniform;
        // a wave of 64/L slots must stay inside one spectrum for the uniform (scalar) operand path
        if constexpr (CoopLimit<M>::value > 0) {
            const int want = move_lanes(a);
            if (want == 4 && (!U || (Wp / 2) % 16 == 0)) return move_generic_batch_l<M, U, 4>(c, a, kind, Wp, st);
            if (want >= 2 && (!U || (Wp / 2) % 32 == 0)) return move_generic_batch_l<M, U, 2>(c, a, kind, Wp, st);
        }
        return move_generic_batch_l<M, U, 1>(c, a, kind, Wp, st);
    });
}

template <int P, bool COMP>
int move_reduced_batch(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, bool u, hipStream_t st)
{
    return with_flag(u, [&](auto uniform) {
        BatchReducedLP<P, uniform, COMP> lp;
        lp.red = reinterpret_cast<const ReducedArgs<P, COMP> *>(c->red[COMP ? 1 : 0].d_red); lp.Wp = Wp; lp.lconst = c->d_lconst;
        lp.red_plain = reinterpret_cast<const ReducedArgs<P, false> *>(c->red[0].d_red);
        lp.tier = COMP && c->mixed ? c->d_tier : nullptr;
        lp.b = c->bounds;
        return launch_move(a, kind, lp, st);
    });
}

}  // namespace

namespace bisip {
namespace host {

// Wp walkers per spectrum; a wave of 64 slots stays inside one spectrum iff (Wp/2) % 64 == 0
int dispatch_move_batch(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, hipStream_t st)
{
    const bool u = (Wp % 128) == 0;
    if (c->model_id == BISIP_MODEL_POLYDECOMP) {
        const int v = effective_variant(c);
        if (v == BISIP_VARIANT_FAITHFUL || v == BISIP_VARIANT_WAVE)
            return fail(BISIP_EUNSUPPORTED, "the device moves have no kernel for the faithful / wave "
                        "formulation: use variant auto, reduced or collapsed");
        if (v == BISIP_VARIANT_REDUCED) return with_pd_degree(c, "batch move", [&](auto p) { return move_reduced_batch<p, false>(c, a, kind, Wp, u, st); });
        if (v == BISIP_VARIANT_REDUCED_COMP) return with_pd_degree(c, "batch move", [&](auto p) { return move_reduced_batch<p, true>(c, a, kind, Wp, u, st); });
    }
    return with_model(c, "batch move", [&](auto m) { return move_generic_batch<typename decltype(m)::type>(c, a, kind, Wp, u, st); });
}

}  // namespace host
}  // namespace bisip
