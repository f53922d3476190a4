// lp_build.h -- the log-probability functor of a context, built in one place for every sampler kernel that takes one
// (the stretch move's and the other moves' dispatch units, lone spectrum and batch).  A builder turns the context's
// model shape, formulation and lane count into a functor type, fills the functor and hands it to f, which launches;
// a unit instantiates the builder it calls with its own f, so each still compiles its own kernels only.
#pragma once
#include "host.h"

namespace bisip {
namespace host {

// A lone spectrum: f(GenericLP<M, L>) or f(ReducedLP<P, COMP>).  `lanes` per slot are wanted; LMAX is the most the
// caller has kernels for (more than that, or lanes for a model whose frequency loop is not split, run as one).
// `what` names the kernel family in with_model's error text; no_kernel is the caller's refusal of the formulations
// that have no sampler kernel.
template <int LMAX, class F>
int with_lone_lp(const bisip_ctx *c, int lanes, const char *what, const char *no_kernel, F &&f)
{
    if (c->model_id == BISIP_MODEL_POLYDECOMP) {
        const int v = effective_variant(c);
        // the sampler kernels exist for the reduced and the collapsed formulation only; running
        // another one here would store log-probabilities that bisip_logprob does not reproduce
        // bit for bit, so say so
        if (v == BISIP_VARIANT_FAITHFUL || v == BISIP_VARIANT_WAVE) return fail(BISIP_EUNSUPPORTED, "%s", no_kernel);
        if (is_reduced(v))
            return with_pd_degree(c, what, [&](auto p) {
                constexpr int P = decltype(p)::value;
                return with_flag(v == BISIP_VARIANT_REDUCED_COMP, [&](auto comp) {
                    ReducedLP<P, decltype(comp)::value> lp;
                    fill_reduced<P, decltype(comp)::value>(c, lp.r);
                    lp.lconst = c->lconst;
                    lp.b = c->bounds;
                    return f(lp);
                });
            });
    }
    return with_model(c, what, [&](auto m) {
        using M = typename decltype(m)::type;
        auto go = [&](auto l) {
            GenericLP<M, decltype(l)::value> lp;
            lp.o = ModelOperands{c->d_cb_lp ? c->d_cb_lp : c->d_cb, c->N, c->lconst};
            lp.b = c->bounds;
            return f(lp);
        };
        if constexpr (CoopLimit<M>::value > 0) {      // (else one lane per slot: the other kernels are never instantiated)
            if constexpr (LMAX >= 8) if (lanes == 8) return go(std::integral_constant<int, 8>{});
            if (lanes == 4) return go(std::integral_constant<int, 4>{});
            if (lanes == 2) return go(std::integral_constant<int, 2>{});
        }
        return go(std::integral_constant<int, 1>{});
    });
}

// A batch of spectra, Wp walkers each: f(BatchGenericLP<M, U, L>) or f(BatchReducedLP<P, U, COMP>).  `whole`: the
// kernel's workgroup is one ensemble (the persistent kernel).  U, the uniform (scalar) operand path, needs every
// wave of 64 slots inside one spectrum: (Wp / 2) % 64 == 0, or whole.  With L lanes a slot a wave holds 64 / L slots,
// which must stay inside one spectrum as well, so fewer lanes than wanted run where Wp / 2 does not divide.
// (No refusal of the faithful / wave formulation: bisip_ctx_set_variant gives neither to a batch.)
template <class F>
int with_batch_lp(const bisip_ctx *c, long long Wp, int lanes, bool whole, const char *what, F &&f)
{
    return with_flag((Wp % 128) == 0 || whole, [&](auto uniform) {
        constexpr bool U = decltype(uniform)::value;
        const int v = c->model_id == BISIP_MODEL_POLYDECOMP ? effective_variant(c) : BISIP_VARIANT_AUTO;
        if (is_reduced(v))
            return with_pd_degree(c, what, [&](auto p) {
                constexpr int P = decltype(p)::value;
                return with_flag(v == BISIP_VARIANT_REDUCED_COMP, [&](auto comp) {
                    constexpr bool COMP = decltype(comp)::value;
                    BatchReducedLP<P, U, COMP> lp;
                    lp.red = reinterpret_cast<const ReducedArgs<P, COMP> *>(c->red[COMP ? 1 : 0].d_red); lp.Wp = Wp; lp.lconst = c->d_lconst;
                    lp.red_plain = reinterpret_cast<const ReducedArgs<P, false> *>(c->red[0].d_red);
                    lp.tier = COMP && c->mixed ? c->d_tier : nullptr;
                    lp.b = c->bounds;
                    return f(lp);
                });
            });
        return with_model(c, what, [&](auto m) {
            using M = typename decltype(m)::type;
            auto go = [&](auto l) {
                BatchGenericLP<M, U, decltype(l)::value> lp;
                lp.cb = c->d_cb_lp ? c->d_cb_lp : c->d_cb; lp.cb_stride = c->cb_stride; lp.Wp = Wp; lp.lconst = c->d_lconst; lp.N = c->N;
                lp.b = c->bounds;
                return f(lp);
            };
            if constexpr (CoopLimit<M>::value > 0) {      // (models whose frequency loop is too cheap to split have one lane per slot: no other kernels exist)
                const bool any = !U || whole;
                if (lanes == 4 && (any || (Wp / 2) % 16 == 0)) return go(std::integral_constant<int, 4>{});
                if (lanes >= 2 && (any || (Wp / 2) % 32 == 0)) return go(std::integral_constant<int, 2>{});
            }
            return go(std::integral_constant<int, 1>{});
        });
    });
}

}  // namespace host
}  // namespace bisip
