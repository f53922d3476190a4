// response_plan.h -- how the fused passes over a device-resident chain (dispatch_response.hip, dispatch_fit.hip) cut a
// spectrum's rows into segments and spread them over row slots, and the chain-shape check both share.  A function of the
// shape alone; bisip_amd/response.py restates it (plan).
#pragma once
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

inline int check_response_shape(const bisip_ctx *c, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble)
{
    if (!c) return fail(BISIP_EINVAL, "null context");
    if (n_samples < 1 || n_samples > 0x7fffffffLL || n_spectra < 1 || n_spectra > c->E || walkers_per_ensemble < 1 ||
        walkers_per_ensemble > 0x7fffffffLL / (2 * BISIP_MAX_NDIM))
        return fail(BISIP_EINVAL, "bad chain shape");
    return BISIP_OK;
}

}  // namespace host
}  // namespace bisip
