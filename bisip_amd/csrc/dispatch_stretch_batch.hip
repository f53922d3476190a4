// dispatch_stretch_batch.hip -- stretch-move launches for a batch of spectra (one context, E
// ensembles): half-step and persistent kernels over BatchGenericLP / BatchReducedLP, which lp_build.h builds.
#include "stretch_launch.h"

using namespace bisip;
using namespace bisip::host;

namespace bisip {
namespace host {

// Wp walkers per spectrum
int dispatch_stretch_batch(const bisip_ctx *c, const StretchWork &a, long long Wp, hipStream_t st)
{
    // in the persistent kernel a workgroup IS one ensemble
    return with_batch_lp(c, Wp, stretch_lanes(a), a.kind == STRETCH_PERSIST, "batch stretch",
                         [&](const auto &lp) { return launch_stretch(a, lp, st); });
}

}  // namespace host
}  // namespace bisip
