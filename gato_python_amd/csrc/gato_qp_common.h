// Device helpers of the box-QP kernels (gato_qp.hip, gato_polish.hip).  Internal header.
#pragma once
#include "gato_common.h"

namespace gato {
namespace {

template <typename T>
__device__ __forceinline__ T clip(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }

// |v| as the bit pattern of a non-negative double: ordered as the values, NaN above +inf, so an integer max is the max
template <typename T>
__device__ __forceinline__ unsigned long long mag_bits(T v) { return __builtin_bit_cast(unsigned long long, fabs((double)v)); }

__device__ __forceinline__ unsigned long long wave_max_bits(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ double slot_val(const unsigned long long *s, int f) { return __builtin_bit_cast(double, s[f]); }

}  // namespace
}  // namespace gato
