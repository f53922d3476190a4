// dispatch_forward.hip -- batched forward() launches.
#include "host.h"
#include <type_traits>

using namespace bisip;
using namespace bisip::host;

namespace {

// PolynomialDecomposition's forward is 17 instructions per frequency: whole rows through LDS (k_forward_rows) beat
// the 16-frequency tiles up to N = 32 (4.95 -> 5.3 TB/s of Z at N = 32).  The transcendental models keep the tiles
// there: all of a row's arithmetic in front of all of its stores costs them more than the longer runs gain (4.9 ->
// 4.1 TB/s, ColeCole<2>; 4.5 -> 3.8, Shin).
template <class M> struct cheap_eval : std::false_type {};
template <int P> struct cheap_eval<PDCollapsed<P>> : std::true_type {};

// spectrum >= 0: the rows belong to `count` consecutive spectra of a batch context, starting with that one,
// W / count rows each (bisip_forward_spectra_dev)
template <class M>
int launch_forward(const bisip_ctx *c, const double *theta, int64_t W, double *Z, hipStream_t st, long long spectrum = -1,
                   long long count = 1)
{
    LaunchArgs a = make_args(c, theta, Z, W, c->d_cb + (spectrum >= 0 ? spectrum * c->cb_stride : 0));
    if (c->E > 1 && spectrum < 0) { a.Wp = W / c->E; a.cb_stride = c->cb_stride; }   // batch: caller checked Wp % 64 == 0
    if (spectrum >= 0 && count > 1) { a.Wp = W / count; a.cb_stride = c->cb_stride; }   // caller checked (W / count) % 64 == 0
    // one single-wave workgroup per 64 walkers; the grid is not capped at the resident count
    // (a capped, looping grid measured 0-25 % slower depending on the box: benchmarks/micro/forward_variants.hip)
    const unsigned grid = (unsigned)((W + 63) / 64);
    const int N = c->N;
    const bool wide = (N % 2 == 0) && ((uintptr_t)Z % 16) == 0;   // 16-byte store pieces
    if ((N % 16 != 0 || cheap_eval<M>::value) && N <= 24) {
        if (wide) hipLaunchKernelGGL((k_forward_rows<M, 24, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_forward_rows<M, 24, false>), dim3(grid), dim3(64), 0, st, a);
    } else if ((N % 16 != 0 || cheap_eval<M>::value) && N <= 32) {
        if (wide) hipLaunchKernelGGL((k_forward_rows<M, 32, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_forward_rows<M, 32, false>), dim3(grid), dim3(64), 0, st, a);
    } else if (N % 16 == 0 && wide) hipLaunchKernelGGL((k_forward_tiled16<M>), dim3(grid), dim3(64), 0, st, a);
    else if (((uintptr_t)theta % 16) == 0) hipLaunchKernelGGL((k_forward_tiled<M, true>), dim3(grid), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_forward_tiled<M, false>), dim3(grid), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

// column-major output for `count` consecutive spectra starting with `spectrum`, W / count rows each
template <class M>
int launch_forward_columns(const bisip_ctx *c, const double *theta, int64_t W, double *cols, hipStream_t st, long long spectrum,
                           long long count, int kind)
{
    LaunchArgs a = make_args(c, theta, cols, W, c->d_cb + spectrum * c->cb_stride);
    a.Wp = W / count; a.cb_stride = c->cb_stride;
    if (kind == BISIP_RESPONSE_PA)
        hipLaunchKernelGGL((k_forward_columns<M, true>), dim3((unsigned)((W + 63) / 64)), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((k_forward_columns<M, false>), dim3((unsigned)((W + 63) / 64)), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

// a batch whose 64-walker blocks straddle spectra: one thread per (row, frequency)
template <class M>
int launch_forward_batch(const bisip_ctx *c, const double *theta, int64_t W, double *Z, hipStream_t st)
{
    const BatchArgs a = make_batch_args(c, theta, Z, W);
    const long long total = (long long)W * c->N;
    hipLaunchKernelGGL((k_forward_batch<M>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int dispatch_forward_batch(const bisip_ctx *c, const double *theta, int64_t W, double *Z, hipStream_t st)
{
    return with_model(c, "batch forward", [&](auto m) { return launch_forward_batch<typename decltype(m)::type>(c, theta, W, Z, st); });
}

}  // namespace

namespace bisip {
namespace host {

int dispatch_forward_columns(const bisip_ctx *c, const double *theta, int64_t W, double *cols, hipStream_t st, long long spectrum,
                             long long count, int kind)
{
    if (kind != BISIP_RESPONSE_RI && kind != BISIP_RESPONSE_PA) return fail(BISIP_EINVAL, "unknown response kind %d", kind);
    if (W == 0) return BISIP_OK;
    if (spectrum < 0 || count < 1 || spectrum + count > c->E) return fail(BISIP_EINVAL, "spectra [%lld, %lld) of %d", spectrum, spectrum + count, c->E);
    if (W % count) return fail(BISIP_EINVAL, "W=%lld rows do not divide over %lld spectra", (long long)W, count);
    if ((W + 63) / 64 > 0x7fffffffLL) return fail(BISIP_EINVAL, "W=%lld exceeds the launch grid limit", (long long)W);
    if (((uintptr_t)theta % 8) || ((uintptr_t)cols % 8)) return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    return with_model(c, "forward-columns", [&](auto m) { return launch_forward_columns<typename decltype(m)::type>(c, theta, W, cols, st, spectrum, count, kind); });
}

int dispatch_forward(const bisip_ctx *c, const double *theta, int64_t W, double *Z, hipStream_t st, long long spectrum,
                     long long count)
{
    if (W == 0) return BISIP_OK;
    if (spectrum >= 0 && (count < 1 || spectrum + count > c->E)) return fail(BISIP_EINVAL, "spectra [%lld, %lld) of %d", spectrum, spectrum + count, c->E);
    if (spectrum >= 0 && count > 1 && (W % count || (W / count) % 64))
        return fail(BISIP_EINVAL, "W=%lld rows over %lld spectra: each needs a multiple of 64 rows", (long long)W, count);
    if (((long long)W * c->N + 255) / 256 > 0x7fffffffLL)
        return fail(BISIP_EINVAL, "W=%lld exceeds the launch grid limit", (long long)W);
    if (((uintptr_t)theta % 8) || ((uintptr_t)Z % 8)) return fail(BISIP_EINVAL, "buffers must be 8-byte aligned");
    if (c->E > 1 && spectrum < 0) {
        if (W % c->E) return fail(BISIP_EINVAL, "W=%lld is not a multiple of n_spectra=%d", (long long)W, c->E);
        if ((W / c->E) % 64) return dispatch_forward_batch(c, theta, W, Z, st);
        // else 64-walker blocks never straddle two spectra: the tiled / whole-row kernels apply
    }
    return with_model(c, "forward", [&](auto m) { return launch_forward<typename decltype(m)::type>(c, theta, W, Z, st, spectrum, count); });
}

}  // namespace host
}  // namespace bisip
