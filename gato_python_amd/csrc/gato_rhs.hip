// gamma = c - C G^-1 g for new right-hand sides over the blocks of the most recent assembly (gato_solve_rhs): the re-solve's
// only stage in front of the PCG.  Nothing here writes a matrix buffer.
#include "gato_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;

// One wave per knot (grid.x strides over the knots, grid.y = system).  The knot's blocks go into LDS once and every
// right-hand side of the system reuses them, so the matrix bytes are read once per knot whatever R is.  Per knot
// (schur_kernel's definition, gato_assembly.hip):
//   gamma_0 = c_0 - Q_0^-1 q_0
//   gamma_k = c_k - Q_k^-1 q_k - phi_k q_{k-1} - B_{k-1} R_{k-1}^-1 r_{k-1},   phi_k = A_{k-1} Q_{k-1}^-1 = -S[k].left
// phi_k is taken from S[k].left (bit for bit what the assembly computed) instead of A_{k-1} and Q_{k-1}^-1 again; BR = B R^-1
// is formed once per knot with plain FMAs.  The lanes cover (row, right-hand side) pairs: S R rows per knot.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void rhs_gamma_kernel(const T *__restrict__ Ginv, const T *__restrict__ Cd,
                                                         const T *__restrict__ Sbd, const T *__restrict__ g,
                                                         const T *__restrict__ c, T *__restrict__ gamma, int K, int R,
                                                         BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SC = S * C;
    __shared__ T sQi[SS], sPhi[SS], sB[SC], sRi[CC], sBR[SC];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    Ginv += sys * bs.g; Cd += sys * bs.c; Sbd += sys * bs.bd;
    g += sys * R * bs.n; c += sys * R * bs.sk; gamma += sys * R * bs.sk;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        __syncthreads();                                                     // the previous knot's readers are done
        const T *Qi = Ginv + (size_t)k * (SS + CC);
        for (int i = lane; i < SS; i += WAVE) sQi[i] = Qi[i];
        if (k > 0) {
            const T *Sl = Sbd + (size_t)k * 3 * SS, *B = Cd + (size_t)(k - 1) * (SS + SC) + SS;
            const T *Ri = Ginv + (size_t)(k - 1) * (SS + CC) + SS;
            for (int i = lane; i < SS; i += WAVE) sPhi[i] = -Sl[i];
            for (int i = lane; i < SC; i += WAVE) sB[i] = B[i];
            for (int i = lane; i < CC; i += WAVE) sRi[i] = Ri[i];
            __syncthreads();
            for (int e = lane; e < SC; e += WAVE) {                          // BR (S x C, column-major)
                const int r = e % S, j = e / S;
                T acc = (T)0;
#pragma unroll
                for (int l = 0; l < C; ++l) acc = gato::fmaT(sB[r + l * S], sRi[l + j * C], acc);
                sBR[e] = acc;
            }
        }
        __syncthreads();
        for (int e = lane; e < S * R; e += WAVE) {
            const int i = e % S, rr = e / S;
            const T *gr = g + (size_t)rr * bs.n, *cr = c + (size_t)rr * bs.sk;
            const T *qk = gr + (size_t)k * n;
            T t = (T)0;
#pragma unroll
            for (int cc = 0; cc < S; ++cc) t = gato::fmaT(sQi[i + cc * S], qk[cc], t);     // Q_k^-1 q_k
            T out;
            if (k == 0) {
                out = cr[i] - t;
            } else {
                const T *qm = gr + (size_t)(k - 1) * n, *rm = qm + S;
                T p = (T)0, b = (T)0;
#pragma unroll
                for (int cc = 0; cc < S; ++cc) p = gato::fmaT(sPhi[i + cc * S], qm[cc], p);  // phi_k q_{k-1}
#pragma unroll
                for (int cc = 0; cc < C; ++cc) b = gato::fmaT(sBR[i + cc * S], rm[cc], b);   // BR r_{k-1}
                T gt = t - cr[(size_t)k * S + i];
                gt += b + p;
                out = -gt;
            }
            gamma[(size_t)rr * bs.sk + (size_t)k * S + i] = out;
        }
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_rhs_gamma(const Dims &d, int R, const T *Ginv, const T *Cd, const T *Sbd, const T *g, const T *c, T *gamma,
                     hipStream_t st)
{
    if (R < 1 || d.B < 1 || d.B > 65535) {
        set_error("rhs_gamma: R = %d, B = %d", R, d.B);
        return GATO_EINVAL;
    }
    const int gx = d.K < 8192 ? d.K : 8192;
    hipLaunchKernelGGL((rhs_gamma_kernel<T, S, C>), dim3(gx, d.B), dim3(WAVE), 0, st, Ginv, Cd, Sbd, g, c, gamma, d.K, R,
                       batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

#define X(S_, C_)                                                                                                   \
    template int launch_rhs_gamma<float, S_, C_>(const Dims &, int, const float *, const float *, const float *,  \
                                                 const float *, const float *, float *, hipStream_t);             \
    template int launch_rhs_gamma<double, S_, C_>(const Dims &, int, const double *, const double *, const double *, \
                                                  const double *, const double *, double *, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
