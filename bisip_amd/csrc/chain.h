// chain.h -- what the chain_*.hip units share: the error plumbing and the argument checks (chain_check.h), the sum over a
// wave, the column toolkit and the one segmented sort (both in chain_columns.hip), and the launch of a kernel that is a
// template of ndim.  A unit that
// summarises a device-resident chain includes this header and nothing of the samplers' (host.h, kernels.h); the two
// units that take lag sums include it through chain_lags.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/bisip_hip.h"
#include "chain_check.h"

namespace bisip {

// the sum of x over the 64 lanes of a wave, in every lane: lanes 32, 16, ..., 1 apart are added pairwise
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

namespace host {

// the column toolkit: what the percentile entry points share with chain_trace.hip and chain_hdi.hip
int percentile_ranks(long long n, const double *percentiles, int n_percentiles, std::vector<long long> &lo, std::vector<double> &t);
int select_columns(const double *cols, long long n, long long columns, int n_percentiles, const std::vector<long long> &lo,
                   const std::vector<double> &t, double *d_out, hipStream_t st, long long out_stride = 0, bool raw = false);
int gather_columns(const double *d_chain, long long n_samples, long long sample_stride, long long E, long long Wp, int ndim,
                   double *cols, hipStream_t st);
int gather_columns_by_sample(const double *d_chain, long long n_samples, long long sample_stride, long long E, long long Wp,
                             int ndim, double *cols, hipStream_t st);

// the segmented radix sort of `segments` contiguous segments of n doubles each (items = segments * n < 2^31)
int sort_temp_bytes(long long items, long long segments, long long n, size_t *bytes);
size_t sort_scratch_bound(long long items, long long segments);
int sort_segments(void *d_temp, size_t temp, const double *in, double *out, long long items, long long segments, long long n,
                  hipStream_t st);

// Launch<ndim>::run(grid, st, args) for a kernel that is a template of ndim (chain_rtd.hip, chain_hist.hip)
template <template <int> class Launch, typename Args>
int launch_by_ndim(int ndim, dim3 grid, hipStream_t st, const Args &args)
{
    switch (ndim) {
    case 2: Launch<2>::run(grid, st, args); break;
    case 3: Launch<3>::run(grid, st, args); break;
    case 4: Launch<4>::run(grid, st, args); break;
    case 5: Launch<5>::run(grid, st, args); break;
    case 6: Launch<6>::run(grid, st, args); break;
    case 7: Launch<7>::run(grid, st, args); break;
    case 8: Launch<8>::run(grid, st, args); break;
    case 9: Launch<9>::run(grid, st, args); break;
    case 10: Launch<10>::run(grid, st, args); break;
    case 11: Launch<11>::run(grid, st, args); break;
    case 12: Launch<12>::run(grid, st, args); break;
    case 13: Launch<13>::run(grid, st, args); break;
    case 14: Launch<14>::run(grid, st, args); break;
    case 15: Launch<15>::run(grid, st, args); break;
    case 16: Launch<16>::run(grid, st, args); break;
    default: return fail(BISIP_EINVAL, "no kernel of ndim=%d", ndim);       // (the entry points check ndim first)
    }
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}
static_assert(BISIP_MAX_NDIM == 16, "launch_by_ndim covers ndim 2 ... 16");

}  // namespace host
}  // namespace bisip
