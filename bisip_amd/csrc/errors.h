// errors.h -- the error plumbing of every translation unit of libbisip_hip.so: fail() records the text that
// bisip_last_error returns (bisip_hip.hip) and hands the code back; HIP_TRY turns a HIP error into BISIP_EHIP.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bisip_hip.h"

namespace bisip {
namespace host {

int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return ::bisip::host::fail(BISIP_EHIP, "%s failed: %s (%s:%d)", #expr,     \
                                       hipGetErrorString(e_), __FILE__, __LINE__);     \
    } while (0)

}  // namespace host
}  // namespace bisip
