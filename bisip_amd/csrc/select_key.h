// select_key.h -- the order-preserving 64-bit image of a double that the selection kernels compare
// (chain_columns.hip: k_segmented_select; chain_hist.hip: k_chain_range; chain_trace.hip: k_chain_trace_lds).
#pragma once
#include <hip/hip_runtime.h>

namespace bisip {

__device__ __forceinline__ unsigned long long select_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);      // ascending keys <=> ascending doubles
}

__device__ __forceinline__ double select_value(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// keys of NaNs lie beyond those of the infinities at either end
__device__ __forceinline__ bool select_key_is_nan(unsigned long long k)
{
    return k > 0xfff0000000000000ull || k < 0x000fffffffffffffull;
}

}  // namespace bisip
