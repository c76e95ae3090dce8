// Right-hand side of the tangent (forward-mode) system of a plain KKT solve with a state-control cross term in the stage cost
// (gato_kkt_tangent_rhs_cross).  With x = dz, lambda the point of the cross solve in the original
// variables, a dot an input tangent and G_k = [[Q_k, M_k], [M_k^T, R_k]] (k < K - 1; the last knot has no M):
//   t_g = g. - G. x - C.^T lambda,  (G. x)_x,k = Q._k x_k + M._k u_k,  (G. x)_u,k = M._k^T x_k + R._k u_k;   t_c = c. - C. x
//   g'_x,k = t_g,x,k - W_k^T t_g,u,k,  g'_u = t_g,u     (the transform of cross_rhs_kernel, from the solver's stored W_k)
// M. is used as given: M_k and M_k^T are perturbed together, the convention of grad_cross_kernel's M_bar.  W has no tangent: it is
// part of how the inverse is applied, not of what is differentiated.
// One wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i of the knot; the R directions loop inside
// the wave over what LDS holds once for all of them (x of knots k-1 and k, lambda_k+1, W_k).  Wave k writes t_g / g' of knot k and
// t_c of block row k: every output element has one writer, no atomics, and every sum is one chain of fused multiply-adds over the
// ascending index - row i of G. x is the Q. (R.) products and then the M. (M.^T) products on the same chain.
// No act, no bounds, no weights: kkt_tangent_rhs_kernel's act blocks fill LDS, this kernel has none and stages the tangent
// blocks of one direction instead (STAGE), with whole-wave contiguous loads.  M._k and C._k are read along a row by the lanes
// of a column, so their staged copies have a leading dimension of S + 1 (LDS banks).  STAGE = false reads the blocks where they
// lie, as kkt_tangent_rhs_kernel does; the bits are the same.
#include "gato_cross_device.h"

namespace gato {
namespace {

constexpr int WAVE = 64;

template <typename T, int S, int C, bool STAGE>
__global__ __launch_bounds__(WAVE) void cross_tangent_rhs_kernel(CrossTangentArgs a, int K, int R, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SC = S * C, SN = S * n;
    constexpr int LD = STAGE ? S + 1 : S;                                     // leading dimension of M._k and C._k as they are read
    __shared__ T sG[STAGE ? SS + CC : 1], sM[STAGE ? LD * C : 1], sCp[STAGE ? SN : 1], sCk[STAGE ? LD * n : 1];
    __shared__ T sW[SC], sXp[n], sXk[n], sLn[S], sTu[C];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y, ms = (size_t)(K - 1) * SC;
    const T *x = (const T *)a.x + sys * bs.n, *lam = (const T *)a.lam + sys * bs.sk;
    const T *W = (const T *)a.W + sys * ms;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const bool full = k < K - 1;
        const int nk = full ? n : S;
        const size_t v0 = (size_t)k * n;
        __syncthreads();                                                     // the previous knot's readers are done
        if (full && a.gp)
            for (int e = lane; e < SC; e += WAVE) sW[e] = W[(size_t)k * SC + e];
        if (lane < nk) sXk[lane] = x[v0 + lane];
        if (k > 0 && lane < n) sXp[lane] = x[v0 - n + lane];                 // knot k-1 is always a full knot
        if (full && lane < S) sLn[lane] = lam[(size_t)(k + 1) * S + lane];
        for (int r = 0; r < R; ++r) {
            const size_t dir = sys * R + r;
            const T *Gd = a.G_dot ? (const T *)a.G_dot + dir * bs.g + (size_t)k * (SS + CC) : nullptr;
            const T *Md = a.M_dot && full ? (const T *)a.M_dot + dir * ms + (size_t)k * SC : nullptr;
            const T *Cdk = a.C_dot && full ? (const T *)a.C_dot + dir * bs.c + (size_t)k * SN : nullptr;
            const T *Cdp = a.C_dot && k > 0 ? (const T *)a.C_dot + dir * bs.c + (size_t)(k - 1) * SN : nullptr;
            if (STAGE) {
                __syncthreads();                                             // the previous direction's readers are done
                if (Gd) {
                    for (int e = lane; e < (full ? SS + CC : SS); e += WAVE) sG[e] = Gd[e];
                    Gd = sG;
                }
                if (Md) {
                    for (int e = lane; e < SC; e += WAVE) sM[e % S + (e / S) * LD] = Md[e];
                    Md = sM;
                }
                if (Cdp) {
                    for (int e = lane; e < SN; e += WAVE) sCp[e] = Cdp[e];
                    Cdp = sCp;
                }
                if (Cdk) {
                    for (int e = lane; e < SN; e += WAVE) sCk[e % S + (e / S) * LD] = Cdk[e];
                    Cdk = sCk;
                }
            }
            __syncthreads();
            T t = (T)0;
            if (lane < nk) {
                const int i = lane;
                if (a.g_dot) t = ((const T *)a.g_dot)[dir * bs.n + v0 + i];
                if (Gd || Md) {                                              // (G. x)_i: the block's own products, then M.'s
                    T hx = (T)0;
                    if (i < S) {
                        if (Gd) {
#pragma unroll 4
                            for (int j = 0; j < S; ++j) hx = fmaT(Gd[i + j * S], sXk[j], hx);
                        }
                        if (Md) {
#pragma unroll 4
                            for (int c = 0; c < C; ++c) hx = fmaT(Md[i + c * LD], sXk[S + c], hx);
                        }
                    } else {
                        const int j = i - S;
                        if (Gd) {
#pragma unroll 4
                            for (int c = 0; c < C; ++c) hx = fmaT(Gd[SS + j + c * C], sXk[S + c], hx);
                        }
                        if (Md) {
#pragma unroll 4
                            for (int s = 0; s < S; ++s) hx = fmaT(Md[s + j * LD], sXk[s], hx);
                        }
                    }
                    t -= hx;
                }
                if (Cdk) {                                                   // (C.^T lambda)_i
                    T ctl = (T)0;
#pragma unroll 4
                    for (int s = 0; s < S; ++s) ctl = fmaT(Cdk[s + i * LD], sLn[s], ctl);
                    t -= ctl;
                }
                if (a.tg) ((T *)a.tg)[dir * bs.n + v0 + i] = t;
            }
            if (lane < S) {                                                  // block row k of c. - C. x
                const int i = lane;
                T tc = a.c_dot ? ((const T *)a.c_dot)[dir * bs.sk + (size_t)k * S + i] : (T)0;
                if (Cdp) {
                    T cx = (T)0;
#pragma unroll 4
                    for (int j = 0; j < n; ++j) cx = fmaT(Cdp[i + j * S], sXp[j], cx);
                    tc -= cx;
                }
                ((T *)a.tc)[dir * bs.sk + (size_t)k * S + i] = tc;
            }
            if (a.gp) {                                                      // g'_x = t_g,x - W^T t_g,u on the values just formed
                if (full) {
                    if (lane >= S && lane < n) sTu[lane - S] = t;
                    __syncthreads();
                    if (lane < S) t = cross_fold_g<T, S, C>(sW, sTu, t, lane);
                }
                if (lane < nk) ((T *)a.gp)[dir * bs.n + v0 + lane] = t;
            }
        }
    }
}

template <typename T, int S, int C>
int launch_tangent(const Dims &d, int R, const CrossTangentArgs &a, bool in_place, hipStream_t st)
{
    if (in_place) return launch_per_knot("kkt_tangent_rhs_cross", cross_tangent_rhs_kernel<T, S, C, false>, d, st, a, d.K, R, batch_stride(d));
    return launch_per_knot("kkt_tangent_rhs_cross", cross_tangent_rhs_kernel<T, S, C, true>, d, st, a, d.K, R, batch_stride(d));
}

}  // namespace
}  // namespace gato

int cross_tangent_rhs(const Dims &d, int dtype, int R, const CrossTangentArgs &a, bool in_place, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_tangent<T, S_, C_>(d, R, a, in_place, st)
    GATO_CROSS_DISPATCH("kkt_tangent_rhs_cross");
#undef GATO_CROSS_LAUNCH
}
