// dispatch_stretch.hip -- stretch-move launches, single spectrum: half-step / eval / apply /
// persistent (the batch-of-spectra instantiations live in dispatch_stretch_batch.hip).  The functor a launch takes
// comes from lp_build.h.
#include "stretch_launch.h"

using namespace bisip;
using namespace bisip::host;

namespace bisip {
namespace host {

StretchArgs to_device_args(const bisip_stretch_args *u)
{
    StretchArgs a;
    a.coords = u->coords; a.logp = u->logp;
    a.active = u->active; a.partner = u->partner;
    a.zz = u->zz; a.factor = u->factor; a.logu = u->logu;
    a.n_slots = u->n_slots; a.slot_lo = u->slot_lo; a.slot_hi = u->slot_hi;
    a.block = u->block; a.chain_row = u->chain_row; a.logp_row = u->logp_row;
    a.naccept = u->naccept; a.status = u->status;
    a.pad = u->pad;
    a.packed = nullptr;
    a.perm = nullptr; a.draw_W = 0; a.draw_a = 0.0; a.draw_ndim_m1 = 0.0;
    a.seed_lo = a.seed_hi = a.draw_step = a.draw_e = 0u; a.draw_h = 0;
    const long long world = u->world > 0 ? u->world : 1;
    a.base = u->n_slots / world;
    a.extra = u->n_slots % world;
    return a;
}

int dispatch_stretch(const bisip_ctx *c, const StretchWork &a, long long Wp, hipStream_t st)
{
    if (c->E > 1) {
        if (Wp < 2 || (Wp & 1)) return fail(BISIP_EINVAL, "batch context: walkers_per_spectrum must be even and >= 2, got %lld", Wp);
        return dispatch_stretch_batch(c, a, Wp, st);
    }
    return with_lone_lp<8>(c, stretch_lanes(a), "stretch",      // (eight lanes: the multi-workgroup sampler only)
                           "the device stretch move has no kernel for the faithful / wave "
                           "formulation: use variant auto, reduced or collapsed, or the host-loop sampler",
                           [&](const auto &lp) { return launch_stretch(a, lp, st); });
}

int dispatch_apply(const bisip_ctx *c, const StretchArgs &a, hipStream_t st)
{
    const unsigned grid = (unsigned)((a.n_slots + 63) / 64);
    switch (c->ndim) {
#define NDIM_CASE(n) case n: hipLaunchKernelGGL((k_stretch_apply<n>), dim3(grid), dim3(64), 0, st, a); break;
        NDIM_CASE(1) NDIM_CASE(2) NDIM_CASE(3) NDIM_CASE(4) NDIM_CASE(5) NDIM_CASE(6) NDIM_CASE(7) NDIM_CASE(8)
        NDIM_CASE(9) NDIM_CASE(10) NDIM_CASE(11) NDIM_CASE(12) NDIM_CASE(13) NDIM_CASE(14) NDIM_CASE(15) NDIM_CASE(16)
#undef NDIM_CASE
    default: return fail(BISIP_EUNSUPPORTED, "ndim=%d", c->ndim);
    }
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

}  // namespace host
}  // namespace bisip
