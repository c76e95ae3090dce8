// The change of variables of a stage-cost cross term, written once for the units that apply it:
// gato_cross.hip, gato_cross_csr.hip, gato_tangent_cross.hip, gato_qp_cross.hip (and the dispatch of gato_grad.hip's cross
// entry).  Internal header.  W_k is C x S column-major, M_k and B^_k S x C column-major, everything else as in gato_cross.hip.
#pragma once
#include "gato_solver.h"
#include "gato_gj.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

// g'_x,i = g_x,i - sum_c W[c, i] g_u,c on t: one chain of fused multiply-adds over the ascending c
template <typename T, int S, int C>
__device__ __forceinline__ T cross_fold_g(const T *sW, const T *gu, T t, int i)
{
    for (int c = 0; c < C; ++c) t = fmaT(-sW[c + i * C], gu[c], t);
    return t;
}

// u_j = v_j - sum_s W[j, s] x_s on t: one chain of fused multiply-adds over the ascending s
template <typename T, int S, int C>
__device__ __forceinline__ T cross_unfold_u(const T *sW, const T *x, T t, int j)
{
    for (int s = 0; s < S; ++s) t = fmaT(-sW[j + s * C], x[s], t);
    return t;
}

// One full knot (k < K - 1) from its blocks in LDS to the work area, by a workgroup of NT threads (whole waves) whose staging
// stores a barrier has already made visible: (R + rho I)^-1 by the assembly's Gauss-Jordan on wave 0, W = Rinv M^T,
// Q'' = Q - M W, A^' = A^ - B^ W, R and B^ as they are, g'_x = g_x - W^T g_u.  sW [S C] and sRi [C C] are scratch; the knot's
// [Q | R], [A^ | B^], W_k and g'_k go to Gp + gb, Cp + cb, W + mb and gp + v0 (base and offset apart, as the kernels held them
// before: pointers offset by the caller cost a VGPR in three instantiations).  Every output element has one writer and one
// chain of fused multiply-adds over the ascending inner index, so the bits do not depend on NT.  The caller's next write to
// the LDS blocks needs a barrier first.
template <typename T, int S, int C, int NT>
__device__ __forceinline__ void cross_transform_knot(const T *sQ, const T *sR, const T *sA, const T *sB, const T *sM, const T *sg,
                                                     T *sW, T *sRi, T rho, int tid, T *Gp, size_t gb, T *Cp, size_t cb, T *W, size_t mb,
                                                     T *gp, size_t v0)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SC = S * C;
    static_assert(NT % 64 == 0, "whole waves");
    const int lane = NT == 64 ? tid : tid & 63, wave = NT == 64 ? 0 : tid >> 6;
    if (wave == 0) {                                                         // (R_k + rho I)^-1 by the assembly's Gauss-Jordan, one wave
        T col[C];
#pragma unroll
        for (int r = 0; r < C; ++r) {
            T e = (T)(lane - C == r);
            if (lane < C) {
                e = sR[lane * C + r];
                if (lane == r) e += rho;
            }
            col[r] = e;
        }
        gj_inverse_reg<T, C>(col);
        if (lane >= C && lane < 2 * C) {
#pragma unroll
            for (int r = 0; r < C; ++r) sRi[(lane - C) * C + r] = col[r];
        }
    }
    __syncthreads();
    for (int e = tid; e < SC; e += NT) {                                     // W = Rinv M^T: W[c][s] = sum_j Rinv[c][j] M[s][j]
        const int c = e % C, s = e / C;
        T t = (T)0;
        for (int j = 0; j < C; ++j) t = fmaT(sRi[c + j * C], sM[s + j * S], t);
        sW[e] = t;
        W[mb + e] = t;
    }
    __syncthreads();
    for (int e = tid; e < SS; e += NT) {                                     // Q'' = Q - M W and A^' = A^ - B^ W
        const int i = e % S, j = e / S;
        T q = sQ[e], t = sA[e];
        for (int c = 0; c < C; ++c) {
            const T w = sW[c + j * C];
            q = fmaT(-sM[i + c * S], w, q);
            t = fmaT(-sB[i + c * S], w, t);
        }
        Gp[gb + e] = q;
        Cp[cb + e] = t;
    }
    for (int e = tid; e < CC; e += NT) Gp[gb + SS + e] = sR[e];              // R and B^ unchanged
    for (int e = tid; e < SC; e += NT) Cp[cb + SS + e] = sB[e];
    if (tid < n) {                                                           // g'_x = g_x - W^T g_u, g'_u = g_u
        T t = sg[tid];
        if (tid < S) t = cross_fold_g<T, S, C>(sW, sg + S, t, tid);
        gp[v0 + tid] = t;
    }
}

}  // namespace
}  // namespace gato

// The launcher's instantiation for the solver's (dtype, S, C), every compiled shape in both precisions, in a function with
// `d` (Dims) and `dtype` in scope: GATO_CROSS_LAUNCH(T, S_, C_), defined around each use, is the call.  prefix: what the
// refusal of a shape that is not compiled begins with.
#define GATO_CROSS_CASE(S_, C_) \
    if (d.S == S_ && d.C == C_) return dtype == GATO_F32 ? GATO_CROSS_LAUNCH(float, S_, C_) : GATO_CROSS_LAUNCH(double, S_, C_);
#define GATO_CROSS_DISPATCH(prefix)                                                                                    \
    do {                                                                                                               \
        GATO_SHAPES(GATO_CROSS_CASE)                                                                                   \
        set_error(prefix ": (STATE_SIZE=%d, CONTROL_SIZE=%d) is not a compiled shape", d.S, d.C);                      \
        return GATO_ESHAPE;                                                                                            \
    } while (0)
