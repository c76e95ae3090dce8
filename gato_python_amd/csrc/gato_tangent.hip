// Right-hand side of the tangent (forward-mode) system of a KKT solve or a converged box-QP point (gato_kkt_tangent_rhs,
// DESIGN.md section 3.13).  With x, lambda the returned point, a dot an input tangent and A the hard-active set:
//   1. t_g = g. - G. x - C.^T lambda,  t_c = c. - C. x                 (C's identity blocks carry no tangent, rho drops out)
//   2. soft-active i: t_g,i += w._i (b_i - x_i) + w_i b._i;  saturated i: t_g,i -= sign(act_i) m._i
//   3. t_g -= G b._A,  t_c -= C b._A  (b._A = b. on A, 0 elsewhere; C's identity blocks included): the shift of
//      polish_prepare_kernel applied to b. instead of b.  Rows of t_g on A hold what the sums give: Ginv' ignores them.
// [x.'; lambda.] = gato_solve_rhs(t_g, t_c) on the point's assembly is the tangent off A; on A it is b. itself.
// One wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i of the knot; the R directions loop
// inside the wave over what LDS holds once for all of them.  Wave k writes t_g of knot k and t_c of block row k: every output
// element has one writer, no atomics, a fixed order of the sums.  Nothing here reads or writes the assembly.
#include "gato_common.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;

// what a variable is in the reduced system of its act
enum { V_FREE = 0, V_HARD = 1, V_SOFT = 2, V_SAT = 3 };

template <typename T, int S, int C, int W>
__global__ __launch_bounds__(WAVE) void kkt_tangent_rhs_kernel(TangentArgs a, int K, int R, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SN = S * n;
    __shared__ T sQ[SS], sR[CC], sCp[SN], sCk[SN];     // with an act only: the blocks of step 3
    __shared__ T sXp[n], sXk[n], sLn[S], sZ[S];        // x of knots k-1 and k, lambda_k+1, zeros (the identity block's tangent)
    __shared__ T sWk[n], sBk[n];                       // W only: knot k's w_i and b_i on the soft-active set
    __shared__ int sKind[2][n], sUp[2][n];             // knots k-1 (0) and k (1): V_* and act > 0
    __shared__ T sD[2][n];                             // per direction: b._A of knots k-1 and k
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const bool has_act = a.act != nullptr;
    const signed char *act = has_act ? a.act + sys * bs.n : nullptr;
    const T *w = has_act ? sys_weights<T, W>(a.w, sys, bs) : nullptr;
    const bool caps = W == BOUNDS_CAPPED && (a.cap || a.m_dot);
    const T *G = has_act ? (const T *)a.G + sys * bs.g : nullptr, *Cd = has_act ? (const T *)a.Cd + sys * bs.c : nullptr;
    const T *x = (const T *)a.x + sys * bs.n, *lam = (const T *)a.lam + sys * bs.sk;
    const T *lo = (const T *)a.lo, *hi = (const T *)a.hi;                      // read on the soft-active set only
    if (lane < S) sZ[lane] = (T)0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int nk = k < K - 1 ? n : S;
        const bool next = k < K - 1;
        const size_t v0 = (size_t)k * n;
        __syncthreads();                                                     // the previous knot's readers are done
        if (has_act) {
            const T *Gk = G + (size_t)k * (SS + CC);
            for (int e = lane; e < SS; e += WAVE) sQ[e] = Gk[e];
            if (next) {
                for (int e = lane; e < CC; e += WAVE) sR[e] = Gk[SS + e];
                for (int e = lane; e < SN; e += WAVE) sCk[e] = Cd[(size_t)k * SN + e];
            }
            if (k > 0)
                for (int e = lane; e < SN; e += WAVE) sCp[e] = Cd[(size_t)(k - 1) * SN + e];
        }
        if (lane < n) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kk = k - 1 + h;
                int kind = V_FREE, up = 0;
                T wi = (T)0, b = (T)0;
                if (has_act && kk >= 0 && lane < (kk < K - 1 ? n : S)) {
                    const size_t v = (size_t)kk * n + lane;
                    const signed char ai = act[v];
                    up = ai > 0;
                    if (soft_active(ai, w, v)) {
                        kind = caps && saturated(ai) ? V_SAT : V_SOFT;
                        if (h == 1 && kind == V_SOFT) {
                            wi = w[v];
                            b = bound_of(ai, lo[sys * bs.n + v], hi[sys * bs.n + v]);
                        }
                    } else if (ai != 0) kind = V_HARD;
                }
                sKind[h][lane] = kind;
                sUp[h][lane] = up;
                if (W && h == 1) { sWk[lane] = wi; sBk[lane] = b; }
            }
            if (lane < nk) sXk[lane] = x[v0 + lane];
            if (k > 0) sXp[lane] = x[v0 - n + lane];                          // knot k-1 is always a full knot
        }
        if (lane < S && next) sLn[lane] = lam[(size_t)(k + 1) * S + lane];
        for (int r = 0; r < R; ++r) {
            const size_t dir = sys * R + r;
            const T *lo_d = a.lo_dot ? (const T *)a.lo_dot + dir * bs.n : nullptr;
            const T *hi_d = a.hi_dot ? (const T *)a.hi_dot + dir * bs.n : nullptr;
            if (has_act) {
                __syncthreads();                                             // the previous direction's readers of sD are done
                if (lane < n) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        T bd = (T)0;
                        if (sKind[h][lane] == V_HARD) {
                            const T *src = sUp[h][lane] ? hi_d : lo_d;
                            if (src) bd = src[(size_t)(k - 1 + h) * n + lane];
                        }
                        sD[h][lane] = bd;
                    }
                }
            }
            __syncthreads();
            const T *Gd = a.G_dot ? (const T *)a.G_dot + dir * bs.g + (size_t)k * (SS + CC) : nullptr;
            const T *Cdk = a.C_dot && next ? (const T *)a.C_dot + dir * bs.c + (size_t)k * SN : nullptr;
            const T *Cdp = a.C_dot && k > 0 ? (const T *)a.C_dot + dir * bs.c + (size_t)(k - 1) * SN : nullptr;
            if (lane < nk) {
                const int i = lane;
                const size_t v = v0 + i;
                T t = a.g_dot ? ((const T *)a.g_dot)[dir * bs.n + v] : (T)0;
                T hx, ctl;
                if (Gd) {                                                    // (G. x)_i: the tangent blocks are read in place
                    row_products<T, S, C>(i, false, Gd, Gd + SS, sCk, sXk, sZ, sZ, (T)0, hx, ctl);
                    t -= hx;
                }
                if (Cdk) {                                                   // (C.^T lambda)_i: only ctl is used, no G product is kept
                    row_products<T, S, C>(i, true, sQ, sR, Cdk, sXk, sZ, sLn, (T)0, hx, ctl);
                    t -= ctl;
                }
                if (W && has_act) {
                    const int kind = sKind[1][i];
                    if (kind == V_SOFT) {
                        const T *src = sUp[1][i] ? hi_d : lo_d;
                        if (a.w_dot) t = fmaT(((const T *)a.w_dot)[dir * bs.n + v], sBk[i] - sXk[i], t);
                        if (src) t = fmaT(sWk[i], src[v], t);
                    } else if (W == BOUNDS_CAPPED && kind == V_SAT && a.m_dot) {
                        const T md = ((const T *)a.m_dot)[dir * bs.n + v];
                        t -= sUp[1][i] ? md : -md;
                    }
                }
                if (has_act) {                                               // (G b._A)_i
                    row_products<T, S, C>(i, false, sQ, sR, sCk, sD[1], sZ, sZ, (T)0, hx, ctl);
                    t -= hx;
                }
                ((T *)a.tg)[dir * bs.n + v] = t;
            }
            if (lane < S) {                                                  // block row k of c. - C. x - C b._A
                const int i = lane;
                T t = a.c_dot ? ((const T *)a.c_dot)[dir * bs.sk + (size_t)k * S + i] : (T)0;
                if (Cdp) {
                    T cx = (T)0;
#pragma unroll 4
                    for (int j = 0; j < n; ++j) cx = fmaT(Cdp[i + j * S], sXp[j], cx);
                    t -= cx;
                }
                if (has_act) {
                    T cb = sD[1][i];
                    if (k > 0) {
#pragma unroll 4
                        for (int j = 0; j < n; ++j) cb = fmaT(sCp[i + j * S], sD[0][j], cb);
                    }
                    t -= cb;
                }
                ((T *)a.tc)[dir * bs.sk + (size_t)k * S + i] = t;
            }
        }
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_kkt_tangent_rhs(const Dims &d, int R, const TangentArgs &a, hipStream_t st)
{
    if (R < 1 || d.B < 1 || d.B > 65535) { set_error("kkt_tangent_rhs: R = %d, B = %d", R, d.B); return GATO_EINVAL; }
    const int form = a.act ? bounds_form(a.w, a.w ? (a.cap ? a.cap : a.m_dot) : nullptr) : BOUNDS_HARD;
    return launch_per_knot("kkt_tangent_rhs", GATO_BOUNDS_KERNEL(kkt_tangent_rhs_kernel, form), d, st, a, d.K, R, batch_stride(d));
}

#define X(S_, C_)                                                                                                   \
    template int launch_kkt_tangent_rhs<float, S_, C_>(const Dims &, int, const TangentArgs &, hipStream_t);        \
    template int launch_kkt_tangent_rhs<double, S_, C_>(const Dims &, int, const TangentArgs &, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
