// dispatch_moves_batch.hip -- differential-evolution and snooker half-steps for a batch of spectra (one context,
// E ensembles): k_move_half over BatchGenericLP / BatchReducedLP, which lp_build.h builds.
#include "move_launch.h"

using namespace bisip;
using namespace bisip::host;

namespace bisip {
namespace host {

// Wp walkers per spectrum
int dispatch_move_batch(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, hipStream_t st)
{
    return with_batch_lp(c, Wp, move_lanes(a), false, "batch move", [&](const auto &lp) { return launch_move(a, kind, lp, st); });
}

}  // namespace host
}  // namespace bisip
