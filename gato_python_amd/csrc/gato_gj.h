// Register-resident Gauss-Jordan of the assembly (gato_assembly.hip), shared with the box-QP polish (gato_polish.hip) so that
// both invert Q_k and R_k with the same arithmetic.  Internal header.
#pragma once
#include "gato_common.h"

namespace gato {
namespace {

__device__ __forceinline__ float readlane_c(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double readlane_c(double v, int l)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// lane c < n holds column c of A, lane n + c holds column c of I; on return lane n + c holds column c of A^-1.
// Same arithmetic as invertMatrix (gato_utils.cuh:468-495): pivot row *= 1/pv, other rows -= col[r]/pv * row.
template <typename T, int n>
__device__ __forceinline__ void gj_inverse_reg(T (&col)[n])
{
#pragma unroll
    for (int p = 0; p < n; ++p) {
        const T pvinv = (T)1 / readlane_c(col[p], p);
        const T prow = col[p] * pvinv;                       // this lane's element of the scaled pivot row
#pragma unroll
        for (int r = 0; r < n; ++r) {
            if (r != p) {
                const T f = readlane_c(col[r], p);           // A[r][p], wave-uniform
                col[r] = gato::fmaT(-f, prow, col[r]);
            }
        }
        col[p] = prow;
    }
}

}  // namespace
}  // namespace gato
