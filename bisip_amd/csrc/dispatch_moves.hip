// dispatch_moves.hip -- differential-evolution and snooker half-steps, single spectrum, and the entry points of
// the moves (draw / half / run); the batch-of-spectra instantiations live in dispatch_moves_batch.hip.  The functor a
// launch takes comes from lp_build.h.
#include "move_launch.h"

using namespace bisip;
using namespace bisip::host;

namespace {

MoveArgs to_move_args(const bisip_move_args *u)
{
    MoveArgs a;
    a.s = to_device_args(&u->stretch);
    a.s.active = u->active; a.s.partner = u->p0; a.s.logu = u->logu;
    a.s.zz = nullptr; a.s.factor = nullptr;
    a.p1 = u->p1; a.p2 = u->p2; a.gamma = u->gamma; a.gammas = u->snooker_gamma;
    return a;
}

// the checks of one half-step of move `kind` over a prepared bisip_move_args (W = walkers per ensemble)
int check_move(const bisip_ctx *c, const bisip_move_args *u, int kind, int64_t W)
{
    const bisip_stretch_args &s = u->stretch;
    if (s.n_slots < 0) return fail(BISIP_EINVAL, "n_slots < 0");
    if (!s.coords || !s.logp || !s.status) return fail(BISIP_EINVAL, "coords/logp/status must not be null");
    if (kind != BISIP_MOVE_DE && kind != BISIP_MOVE_SNOOKER) return fail(BISIP_EINVAL, "unknown move kind %d", kind);
    if (!u->active || !u->p0 || !u->p1 || !u->logu) return fail(BISIP_EINVAL, "null move stream");
    // the smaller half has W / 2 members
    if (kind == BISIP_MOVE_DE) {
        if (W / 2 < 2) return fail(BISIP_EINVAL, "the differential-evolution move needs two partners in the other half: %lld walkers, at least 4", (long long)W);
        if (!u->gamma) return fail(BISIP_EINVAL, "null move stream (gamma)");
    } else {
        if (W / 2 < 3) return fail(BISIP_EINVAL, "the snooker move needs three partners in the other half: %lld walkers, at least 6", (long long)W);
        if (!u->p2) return fail(BISIP_EINVAL, "null move stream (p2)");
        if (!(u->snooker_gamma == u->snooker_gamma)) return fail(BISIP_EINVAL, "snooker_gamma is NaN");
    }
    if (c->E > 1 && W != s.walkers_per_spectrum)
        return fail(BISIP_EINVAL, "batch context: W=%lld is not walkers_per_spectrum=%lld", (long long)W, (long long)s.walkers_per_spectrum);
    return BISIP_OK;
}

}  // namespace

namespace bisip {
namespace host {

int dispatch_move(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, hipStream_t st)
{
    if (c->E > 1) {
        if (Wp < 2 || (Wp & 1)) return fail(BISIP_EINVAL, "batch context: walkers_per_spectrum must be even and >= 2, got %lld", Wp);
        return dispatch_move_batch(c, a, kind, Wp, st);
    }
    return with_lone_lp<4>(c, move_lanes(a), "move",
                           "the device moves have no kernel for the faithful / wave "
                           "formulation: use variant auto, reduced or collapsed",
                           [&](const auto &lp) { return launch_move(a, kind, lp, st); });
}

}  // namespace host
}  // namespace bisip

extern "C" {

int bisip_move_draw_dev(bisip_ctx *c, int64_t W, uint64_t seed, int64_t step0, int64_t n_steps, const int32_t *d_perm,
                        double de_g0, double de_sigma, int32_t *d_active, int32_t *d_p0, int32_t *d_p1, int32_t *d_p2,
                        double *d_gamma, double *d_logu, void *stream)
{
    if (!c || !d_perm || !d_active || !d_p0 || !d_p1 || !d_p2 || !d_gamma || !d_logu) return fail(BISIP_EINVAL, "null argument");
    if (W < 4 || W > 0x7fffffffLL || n_steps < 0 || step0 < 0 || step0 + n_steps > 0xffffffffLL)
        return fail(BISIP_EINVAL, "bad W=%lld (at least 4) or step range [%lld, +%lld)", (long long)W, (long long)step0, (long long)n_steps);
    if (c->E > 1 && (W & 1)) return fail(BISIP_EINVAL, "batch context: walkers per spectrum must be even");
    if ((long long)c->E * W > 0x7fffffffLL) return fail(BISIP_EINVAL, "walker ids beyond 31 bits");
    if (n_steps == 0) return BISIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    MoveDrawArgs d;
    d.s = draw_head(c, W, seed, step0, n_steps, d_perm);
    d.g0 = de_g0; d.sigma = de_sigma;
    d.active = d_active; d.p0 = d_p0; d.p1 = d_p1; d.p2 = d_p2; d.gamma = d_gamma; d.logu = d_logu;
    return launch_draw(d.s.E * d.s.nh, 2 * n_steps, k_move_draw, d, (hipStream_t)stream);
}

int bisip_move_half_dev(bisip_ctx *c, const bisip_move_args *u, int kind, int64_t W, void *stream)
{
    if (!c || !u) return fail(BISIP_EINVAL, "null argument");
    if (kind == BISIP_MOVE_STRETCH) return bisip_stretch_half_dev(c, &u->stretch, stream);
    const int rc = check_move(c, u, kind, W);
    if (rc != BISIP_OK || u->stretch.n_slots == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return dispatch_move(c, to_move_args(u), kind, u->stretch.walkers_per_spectrum, (hipStream_t)stream);
}

int bisip_move_run_dev(bisip_ctx *c, const bisip_move_args *first, const int32_t *kinds, int64_t W, int64_t n_steps,
                       int64_t thin_by, void *stream)
{
    if (!c || !first || !kinds) return fail(BISIP_EINVAL, "null argument");
    if (const int rc = check_chunk(W, n_steps, thin_by)) return rc;
    // W is the total number of walkers (bisip_stretch_run_dev); the moves' refusals speak of one ensemble's
    const int64_t Wp = c->E > 1 ? first->stretch.walkers_per_spectrum : W;
    if (c->E > 1 && (Wp < 2 || (Wp & 1) || Wp * c->E != W))
        return fail(BISIP_EINVAL, "batch context: W=%lld is not %d spectra of walkers_per_spectrum=%lld", (long long)W, c->E, (long long)Wp);
    // every iteration is checked before the first is launched: a refused run leaves the ensemble as it was
    bool stretch = false;
    for (int64_t k = 0; k < n_steps; ++k) {
        if (kinds[k] == BISIP_MOVE_STRETCH) { stretch = true; continue; }
        const int rc = check_move(c, first, kinds[k], Wp);
        if (rc != BISIP_OK) return rc;
    }
    const bisip_stretch_args &f = first->stretch;
    if (!f.coords || !f.logp || !f.status) return fail(BISIP_EINVAL, "null buffer");
    if (stretch && (!f.active || !f.partner || !f.zz || !f.factor || !f.logu)) return fail(BISIP_EINVAL, "null stretch stream");
    HIP_TRY(hipSetDevice(c->device));
    const ChunkWalk walk(W, c->ndim, n_steps, thin_by, f.chain_row, f.logp_row);
    bisip_move_args u = *first;
    for (int64_t k = 0; k < n_steps; ++k) {
        for (int h = 0; h < 2; ++h) {
            const ChunkWalk::Half half = walk.at(k, h);
            const int64_t off = half.off;
            bisip_stretch_args &s = u.stretch;
            s.n_slots = half.n_slots; s.chain_row = half.chain_row; s.logp_row = half.logp_row;
            int rc;
            if (kinds[k] == BISIP_MOVE_STRETCH) {
                s.active = f.active + off; s.partner = f.partner + off;
                s.zz = f.zz + off; s.factor = f.factor + off; s.logu = f.logu + off;
                const StretchArgs a = to_device_args(&s);
                rc = dispatch_stretch(c, StretchWork{STRETCH_HALF, &a, nullptr}, s.walkers_per_spectrum, (hipStream_t)stream);
            } else {
                u.active = first->active + off; u.p0 = first->p0 + off; u.p1 = first->p1 + off;
                u.p2 = first->p2 ? first->p2 + off : nullptr;
                u.gamma = first->gamma ? first->gamma + off : nullptr; u.logu = first->logu + off;
                rc = dispatch_move(c, to_move_args(&u), kinds[k], s.walkers_per_spectrum, (hipStream_t)stream);
            }
            if (rc != BISIP_OK) return rc;
        }
    }
    return BISIP_OK;
}

}  // extern "C"
