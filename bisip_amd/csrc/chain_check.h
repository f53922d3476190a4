// chain_check.h -- the argument checks that the entry points of the chain_*.hip units share.  Host code only: everything
// here runs before a launch.  Each check owns one message text; an entry point calls the pieces in the order its rules
// are reported in, with its own caps, so that where two entries differ the difference is an argument at the call site.
// The ..._workspace functions pass QUIET: they get the code, and the text of bisip_last_error stays as it was.
// chain.h includes this header; a unit that cannot include chain.h (chain_modes.hip, chain_loo.hip: kernels.h defines
// wave_sum too) includes it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "errors.h"

// hands a check's refusal on to the caller of the entry point
#define BISIP_TRY(expr)                                                                \
    do {                                                                               \
        const int rc_ = (expr);                                                        \
        if (rc_ != BISIP_OK) return rc_;                                               \
    } while (0)

namespace bisip {
namespace host {

size_t align256(size_t x);                   // chain_columns.hip: the next multiple of 256 bytes

// the description of a device-resident chain that the entry points share, without the pointer: used sample k of walker w
// of ensemble e lies at d_chain + k * stride + (e * Wp + w) * ndim
struct ChainShape {
    int64_t n, stride, E, Wp;
    int ndim;
};

constexpr int64_t NO_CAP = INT64_MAX;
constexpr int64_t GRID_MAX = 0x7fffffffLL;   // workgroups of one grid dimension; also what a 32-bit index reaches

enum Voice { LOUD, QUIET };

template <class... A>
int refuse(Voice v, int code, const char *fmt, A... a)
{
    return v == QUIET ? code : fail(code, fmt, a...);
}

// least <= ndim <= BISIP_MAX_NDIM; least = 2 for a PolynomialDecomposition chain
inline int check_ndim(int ndim, int least = 1, Voice v = LOUD)
{
    if (ndim >= least && ndim <= BISIP_MAX_NDIM) return BISIP_OK;
    return refuse(v, BISIP_EINVAL, "ndim=%d out of range%s", ndim, least > 1 ? " (r0 and a_0 at least)" : "");
}

// every count at least 1 and at most the cap the entry gives (NO_CAP: none)
inline int check_counts(const ChainShape &s, int64_t n_cap, int64_t E_cap, int64_t Wp_cap, Voice v = LOUD)
{
    if (s.n >= 1 && s.n <= n_cap && s.E >= 1 && s.E <= E_cap && s.Wp >= 1 && s.Wp <= Wp_cap) return BISIP_OK;
    return refuse(v, BISIP_EINVAL, "bad chain shape");
}

// stride >= E * Wp * ndim of counts that are at least 1; a product beyond int64 is more than any stride
inline int check_stride(const ChainShape &s)
{
    int64_t row = 0;
    if (!__builtin_mul_overflow(s.E, s.Wp, &row) && !__builtin_mul_overflow(row, (int64_t)s.ndim, &row) && s.stride >= row)
        return BISIP_OK;
    return fail(BISIP_EINVAL, "sample_stride smaller than one sample");
}

// the three above in the order most entries report them in: ndim, the counts, the stride
inline int check_chain(const ChainShape &s, int least_ndim, int64_t n_cap, int64_t E_cap, int64_t Wp_cap)
{
    BISIP_TRY(check_ndim(s.ndim, least_ndim));
    BISIP_TRY(check_counts(s, n_cap, E_cap, Wp_cap));
    return check_stride(s);
}

// E * Wp rows of one sample within 32 bits, for the kernels that number them so (counts below 1 are not this rule's)
inline int check_rows(const ChainShape &s)
{
    int64_t rows = 0;
    if (s.E < 1 || s.Wp < 1) return BISIP_OK;
    if (__builtin_mul_overflow(s.E, s.Wp, &rows)) rows = INT64_MAX;
    if (rows <= GRID_MAX) return BISIP_OK;
    return fail(BISIP_EUNSUPPORTED, "%lld rows per sample exceed 2^31", (long long)rows);
}

// need bytes of workspace (0: none is looked at); a null workspace counts as one of 0 bytes
inline int check_workspace(const void *d_work, int64_t work_bytes, int64_t need)
{
    if (need <= 0 || (d_work && work_bytes >= need)) return BISIP_OK;
    return fail(BISIP_EINVAL, "workspace of %lld bytes, need %lld", (long long)(d_work ? work_bytes : 0), (long long)need);
}

// count * per workgroups (per >= 1) within one grid dimension; what, a...: the words and numbers of the refusal
template <class... A>
int check_grid(long long count, long long per, Voice v, const char *what, A... a)
{
    if (count <= GRID_MAX / per) return BISIP_OK;
    char fmt[128];
    std::snprintf(fmt, sizeof fmt, "%s exceed one grid", what);
    return refuse(v, BISIP_EUNSUPPORTED, fmt, a...);
}

// a workgroup per (ensemble, segment of its rows): chain_cov.hip and chain_bridge.hip
inline int check_segment_grid(long long nseg, long long E, Voice v = LOUD)
{
    return check_grid(nseg, E, v, "%lld segments of %lld ensembles", nseg, E);
}

}  // namespace host
}  // namespace bisip
