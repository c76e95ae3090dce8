// A state-control cross term in the stage cost: G_k = [[Q_k, M_k], [M_k^T, R_k]] for k < K - 1, M_k S x C.
// The change of variables u_k = v_k - W_k x_k, W_k = (R_k + rho I)^-1 M_k^T, makes the problem block diagonal in (x, v):
//   Q''_k = Q_k - M_k W_k   (the solver adds rho to its diagonal itself),   R_k unchanged,
//   A^'_k = A^_k - B^_k W_k,  B^_k unchanged   (A^ = -A, B^ = -B: the raw values of C_dense),
//   g'_x,k = g_x,k - W_k^T g_u,k,  g'_u,k = g_u,k;   c and lambda unchanged;   the last knot has no M.
// cross_prepare_kernel writes the transformed blocks and W into the solver's work area, cross_rhs_kernel transforms further
// right-hand sides from the stored W, cross_finish_kernel maps a solution back (u = v - W x, in place) and grad_cross_kernel
// forms M_bar from (dz, a).  Nothing here touches an existing kernel: the transformed problem runs through the unchanged whole
// solve and re-solve.
// The per-knot kernels: one wave per knot, grid.x strides over the knots, grid.y = system, operands staged in LDS.  Every output
// element has one writer and one chain of fused multiply-adds over the ascending inner index: no atomics, and the bits do not
// depend on the launch geometry.
#include "gato_cross_device.h"
#include "gato_grad_elem.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NT = 256;

// Layouts: M and W per system [(K-1) S C]; M_k S x C column-major (as B_k in C_dense), W_k C x S column-major.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void cross_prepare_kernel(CrossArgs a, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SC = S * C, SN = S * n;
    __shared__ T sQ[SS], sA[SS], sM[SC], sB[SC], sW[SC], sR[CC], sRi[CC], sg[n];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y, ms = (size_t)(K - 1) * SC;
    const T *G = (const T *)a.G + sys * bs.g, *Cd = (const T *)a.Cd + sys * bs.c, *M = (const T *)a.M + sys * ms;
    const T *g = (const T *)a.g + sys * bs.n;
    T *Gp = (T *)a.Gp + sys * bs.g, *Cp = (T *)a.Cp + sys * bs.c, *W = (T *)a.W + sys * ms, *gp = (T *)a.gp + sys * bs.n;
    const T rho = (T)a.rho;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const size_t gb = (size_t)k * (SS + CC), v0 = (size_t)k * n;
        if (k == K - 1) {                                                    // the last knot has no M: Q and g_x as they are
            for (int e = lane; e < SS; e += WAVE) Gp[gb + e] = G[gb + e];
            if (lane < S) gp[v0 + lane] = g[v0 + lane];
            continue;
        }
        const size_t cb = (size_t)k * SN, mb = (size_t)k * SC;
        __syncthreads();                                                     // the previous knot's readers are done
        for (int e = lane; e < SS; e += WAVE) { sQ[e] = G[gb + e]; sA[e] = Cd[cb + e]; }
        for (int e = lane; e < SC; e += WAVE) { sM[e] = M[mb + e]; sB[e] = Cd[cb + SS + e]; }
        for (int e = lane; e < CC; e += WAVE) sR[e] = G[gb + SS + e];
        if (lane < n) sg[lane] = g[v0 + lane];
        __syncthreads();
        cross_transform_knot<T, S, C, WAVE>(sQ, sR, sA, sB, sM, sg, sW, sRi, rho, lane, Gp, gb, Cp, cb, W, mb, gp, v0);
    }
}

// g' of R right-hand sides per system from the stored W: g, gp [B][R][N]
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void cross_rhs_kernel(const T *__restrict__ Wd, const T *__restrict__ g, T *__restrict__ gp, int K,
                                                         int R, BatchStride bs)
{
    constexpr int n = S + C, SC = S * C;
    __shared__ T sW[SC], sg[n];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *W = Wd + sys * (size_t)(K - 1) * SC;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const size_t v0 = (size_t)k * n;
        const bool full = k < K - 1;
        __syncthreads();                                                     // the previous knot's readers are done
        if (full)
            for (int e = lane; e < SC; e += WAVE) sW[e] = W[(size_t)k * SC + e];
        for (int r = 0; r < R; ++r) {
            const size_t o = (sys * R + r) * bs.n + v0;
            if (lane < (full ? n : S)) sg[lane] = g[o + lane];
            __syncthreads();
            if (lane < (full ? n : S)) {
                T t = sg[lane];
                if (full && lane < S) t = cross_fold_g<T, S, C>(sW, sg + S, t, lane);
                gp[o + lane] = t;
            }
            __syncthreads();                                                 // sg is free for the next right-hand side
        }
    }
}

// u_k <- v_k - W_k x_k of R solutions per system, in place on dz [B][R][N]; x and lambda are not written
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void cross_finish_kernel(const T *__restrict__ Wd, T *__restrict__ dz, int K, int R, BatchStride bs)
{
    constexpr int n = S + C, SC = S * C;
    __shared__ T sW[SC], sx[S];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *W = Wd + sys * (size_t)(K - 1) * SC;
    for (int k = blockIdx.x; k < K - 1; k += gridDim.x) {
        const size_t v0 = (size_t)k * n;
        __syncthreads();                                                     // the previous knot's readers are done
        for (int e = lane; e < SC; e += WAVE) sW[e] = W[(size_t)k * SC + e];
        for (int r = 0; r < R; ++r) {
            const size_t o = (sys * R + r) * bs.n + v0;
            if (lane < S) sx[lane] = dz[o + lane];
            __syncthreads();
            if (lane < C) dz[o + S + lane] = cross_unfold_u<T, S, C>(sW, sx, dz[o + S + lane], lane);
            __syncthreads();                                                 // sx is free for the next solution
        }
    }
}

// M_bar_k = -(a_x,k dz_u,k^T + dz_x,k a_u,k^T) in M's layout, M_k and M_k^T perturbed together: grad_M_elem (gato_grad_elem.h,
// contraction off), which the CSR gradient of a cross entry evaluates too.  Thread = output entry over [B][(K-1) S C].
template <typename T, int S, int C>
__global__ __launch_bounds__(NT) void grad_cross_kernel(const T *__restrict__ dz, const T *__restrict__ a, T *__restrict__ Mbar,
                                                        size_t per, size_t total, BatchStride bs)
{
#pragma clang fp contract(off)
    constexpr int SC = S * C;
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const size_t sys = e / per, r = e - sys * per;
    const size_t k = r / SC;
    Mbar[e] = grad_M_elem<T, S, C>(dz + sys * bs.n, a + sys * bs.n, k, (int)(r - k * SC));
}

template <typename T, int S, int C>
int launch_prepare(const Dims &d, const CrossArgs &a, hipStream_t st)
{
    return launch_per_knot("cross_prepare", cross_prepare_kernel<T, S, C>, d, st, a, d.K, batch_stride(d));
}

template <typename T, int S, int C>
int launch_rhs(const Dims &d, int R, const void *W, const void *g, void *gp, hipStream_t st)
{
    return launch_per_knot("cross_rhs", cross_rhs_kernel<T, S, C>, d, st, (const T *)W, (const T *)g, (T *)gp, d.K, R, batch_stride(d));
}

template <typename T, int S, int C>
int launch_finish(const Dims &d, int R, const void *W, void *dz, hipStream_t st)
{
    if (d.K < 2) return GATO_OK;
    if (d.B < 1 || d.B > 65535) { set_error("cross_finish: B = %d", d.B); return GATO_EINVAL; }
    hipLaunchKernelGGL((cross_finish_kernel<T, S, C>), dim3(knot_grid(d.K - 1), d.B), dim3(WAVE), 0, st, (const T *)W, (T *)dz, d.K, R,
                       batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

template <typename T, int S, int C>
int launch_grad(const Dims &d, const void *dz, const void *a, void *Mbar, hipStream_t st)
{
    const size_t per = (size_t)(d.K - 1) * S * C, total = per * d.B, blocks = (total + NT - 1) / NT;
    if (blocks == 0) return GATO_OK;
    if (blocks > 0x7fffffff) { set_error("kkt_grad_cross: %zu elements are beyond one launch", total); return GATO_EINVAL; }
    hipLaunchKernelGGL((grad_cross_kernel<T, S, C>), dim3((unsigned)blocks), dim3(NT), 0, st, (const T *)dz, (const T *)a, (T *)Mbar,
                       per, total, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

}  // namespace
}  // namespace gato

int cross_prepare(const Dims &d, int dtype, const CrossArgs &a, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_prepare<T, S_, C_>(d, a, st)
    GATO_CROSS_DISPATCH("cross term");
#undef GATO_CROSS_LAUNCH
}

int cross_rhs(const Dims &d, int dtype, int R, const void *W, const void *g, void *gp, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_rhs<T, S_, C_>(d, R, W, g, gp, st)
    GATO_CROSS_DISPATCH("cross term");
#undef GATO_CROSS_LAUNCH
}

int cross_finish(const Dims &d, int dtype, int R, const void *W, void *dz, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_finish<T, S_, C_>(d, R, W, dz, st)
    GATO_CROSS_DISPATCH("cross term");
#undef GATO_CROSS_LAUNCH
}

int cross_grad(const Dims &d, int dtype, const void *dz, const void *a, void *Mbar, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_grad<T, S_, C_>(d, dz, a, Mbar, st)
    GATO_CROSS_DISPATCH("cross term");
#undef GATO_CROSS_LAUNCH
}
