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
//
// Issue order of one pivot step p (the operations and their operands are those of the plain double loop; only the order in
// which independent ones are issued differs, so every bit of the result is the same):
//  * the multipliers A[r][p] of a group of GATO_GJ_AHEAD rows are read into SGPR pairs of their own before the first FMA
//    of the group, so the FMAs issue back to back (a v_readlane feeding the very next VALU instruction costs wait states,
//    and one SGPR pair for every row serialises readlane -> wait -> FMA thirteen times per step);
//  * row p + 1 is updated FIRST: lane p + 1 then holds the next pivot, and its reciprocal - a chain of eleven dependent
//    fp64 instructions that needs nothing else of this step - is started there, in front of the other rows' FMAs.
// The sched_barrier behind a group's readlanes keeps the compiler from sinking them back to their FMAs; behind it the
// compiler places v_div_scale / v_rcp after the first four FMAs and the rest of the chain among the others.  (Pinning one FMA
// behind every instruction of the chain by hand measured the same: DESIGN_LOG.md 3.3.)  n > GATO_GJ_AHEAD + 1 takes two
// groups per step (32 x 32 in fp64 would otherwise hold 62 SGPRs of multipliers).
#ifndef GATO_GJ_AHEAD
#define GATO_GJ_AHEAD 16
#endif
template <typename T, int n>
__device__ __forceinline__ void gj_inverse_reg(T (&col)[n])
{
    constexpr int G = GATO_GJ_AHEAD;
    T pvinv = (T)1 / readlane_c(col[0], 0);
#pragma unroll
    for (int p = 0; p < n; ++p) {
        const T prow = col[p] * pvinv;                       // this lane's element of the scaled pivot row
        // rows in issue order: p + 1, then the others ascending (o -> row index)
        auto row_at = [p](int o) { return p + 1 < n ? (o == 0 ? p + 1 : (o - 1 < p ? o - 1 : o + 1)) : o; };
#pragma unroll
        for (int o0 = 0; o0 < n - 1; o0 += G) {
            T f[G];
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (o0 + j < n - 1) f[j] = readlane_c(col[row_at(o0 + j)], p);   // A[r][p], wave-uniform
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (o0 + j < n - 1) {
                    const int r = row_at(o0 + j);
                    col[r] = gato::fmaT(-f[j], prow, col[r]);
                    if (o0 + j == 0 && p + 1 < n) pvinv = (T)1 / readlane_c(col[p + 1], p + 1);   // next step's 1 / pivot
                }
            }
        }
        col[p] = prow;
    }
}

}  // namespace
}  // namespace gato
