// Box-QP solution polishing and the bound gradients of a polished solution.
// From the active set act of an ADMM result the reduced KKT system [[H_FF, C_F^T], [C_F, 0]] (the active variables fixed at
// their bounds b) is solved exactly on the whole-solve stage path: C's identity blocks are implicit, so an active variable
// cannot be dropped from C; instead every stage after the inversion reads G only through Ginv, and Ginv' (the inverse of
// the free sub-blocks, active rows and columns zero) with the shifted right-hand side g' = g - H_:A b_A, c' = c - C_:A b_A
// gives x'_A = 0 and the reduced solution on F.
// Soft bounds (PolishArgs::w): a variable with a weight w_i > 0 is penalised by (w_i / 2) dist(x_i,
// [lo_i, hi_i])^2 instead of bounded: where it is active it stays in the reduced system - the diagonal entry of Q_k or R_k the
// inversion sees gains w_i, g' gains w_i b_i - and its multiplier is the penalty force y_i = w_i (x_i - b_i).  A variable with
// w_i = 0 is a hard bound; with no weights (w = nullptr) no kernel reads one and every variable is hard.
// Every kernel: one wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i of the knot.
#include "gato_common.h"
#include "gato_gj.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NSL = GATO_POLISH_NSLOT;        // the slot fields: gato_qp_common.h

// OSQP's rule on (z, y): +1 where hi - z < y, -1 where z - lo < -y, -1 wherever lo == hi, 0 on the states of x_0.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void qp_active_kernel(const T *__restrict__ z, const T *__restrict__ y, const T *__restrict__ lo,
                                                         const T *__restrict__ hi, signed char *__restrict__ act, int K, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t o = blockIdx.y * bs.n;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t v = o + (size_t)k * n + lane;
            const T zi = z[v], yi = y[v], l = lo[v], h = hi[v];
            signed char a = 0;
            if (h - zi < yi) a = 1;
            if (zi - l < -yi) a = -1;
            if (l == h) a = -1;
            if (k == 0 && lane < S) a = 0;
            act[v] = a;
        }
    }
}

// Ginv' of the knot (Q_k and R_k with the hard-active rows and columns replaced by the identity, inverted by the assembly's
// Gauss-Jordan, then the hard-active entries zeroed: with nothing active, the bits of the assembly's own inverse), g' and c'.
// A soft-active variable keeps its row and column: the diagonal entry the Gauss-Jordan sees gains w_i, g'_i gains w_i b_i
// (before the hard shift of its row), and c' does not see it.
// An act that is not -1 / 0 / 1, names an infinite bound or a state of x_0 counts the system in *bad and sets polish = 3.
// With caps (W = BOUNDS_CAPPED) a saturated variable (act = +-2, s its sign) is free: no diagonal term, no
// shift, g'_i = g_i - s m_i; +-2 is a bad act only where bad_active_capped says so.
template <typename T, int S, int C, int W>
__global__ __launch_bounds__(WAVE) void polish_prepare_kernel(PolishArgs a, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SN = S * n;
    __shared__ T sb[2][n];                   // bound values of knots k-1 (0) and k (1), 0 off the hard-active set
    __shared__ int sa[2][n];                 // hard-active
    __shared__ T sw[n], ss[n];               // W only: knot k's w_i on the soft-active set (0 elsewhere) and the bound there
    __shared__ T sm[W == BOUNDS_CAPPED ? n : 1];     // caps only: knot k's -s m_i on the saturated set (0 elsewhere)
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *Gd = (const T *)a.Gd + sys * bs.g, *Cd = (const T *)a.Cd + sys * bs.c;
    const T *g = (const T *)a.g + sys * bs.n, *c = (const T *)a.c + sys * bs.sk;
    const T *lo = (const T *)a.lo + sys * bs.n, *hi = (const T *)a.hi + sys * bs.n;
    const T *w = sys_weights<T, W>(a.w, sys, bs);
    const T *cap = sys_caps<T, W>(a.cap, sys, bs);
    const signed char *act = a.act + sys * bs.n;
    T *Gi = (T *)a.Ginv + sys * bs.g, *gp = (T *)a.gp + sys * bs.n, *cp = (T *)a.cp + sys * bs.sk;
    int bad = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int nk = k < K - 1 ? n : S;
        const size_t v0 = (size_t)k * n, gb = (size_t)k * (SS + CC);
        __syncthreads();                                                     // the previous knot's readers are done
        if (lane < n) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kk = k - 1 + h;
                int on = 0;
                T b = (T)0, wi = (T)0, bsoft = (T)0, push = (T)0;
                if (kk >= 0 && lane < (kk < K - 1 ? n : S)) {
                    const size_t v = (size_t)kk * n + lane;
                    const signed char ai = act[v];
                    b = bound_of(ai, lo[v], hi[v]);
                    if constexpr (W == BOUNDS_CAPPED) {
                        if (h == 1 && bad_active_capped(ai, b, kk == 0 && lane < S, w ? w[v] : (T)0, cap ? cap[v] : (T)INFINITY)) bad = 1;
                    } else {
                        if (h == 1 && bad_active(ai, b, kk == 0 && lane < S)) bad = 1;
                    }
                    if (soft_active(ai, w, v)) {
                        if (W == BOUNDS_CAPPED && cap && saturated(ai)) push = ai > 0 ? -cap[v] : cap[v];
                        else {
                            wi = w[v];
                            bsoft = b;
                        }
                        b = (T)0;
                    } else on = ai != 0;
                }
                sa[h][lane] = on;
                sb[h][lane] = b;
                if (W && h == 1) { sw[lane] = wi; ss[lane] = bsoft; }
                if (W == BOUNDS_CAPPED && h == 1) sm[lane] = push;
            }
        }
        __syncthreads();
        {                                                                    // Q_k
            T col[S];
#pragma unroll
            for (int r = 0; r < S; ++r) {
                T e = (T)(lane - S == r);
                if (lane < S) {
                    if (sa[1][lane] || sa[1][r]) e = (T)(lane == r);
                    else {
                        e = Gd[gb + lane * S + r];
                        if (W && lane == r && sw[lane] > (T)0) e += sw[lane];
                    }
                }
                col[r] = e;
            }
            gj_inverse_reg<T, S>(col);
            if (lane >= S && lane < 2 * S) {
                const int cc = lane - S;
#pragma unroll
                for (int r = 0; r < S; ++r) Gi[gb + cc * S + r] = (sa[1][cc] || sa[1][r]) ? (T)0 : col[r];
            }
        }
        if (k < K - 1) {                                                     // R_k
            T col[C];
#pragma unroll
            for (int r = 0; r < C; ++r) {
                T e = (T)(lane - C == r);
                if (lane < C) {
                    if (sa[1][S + lane] || sa[1][S + r]) e = (T)(lane == r);
                    else {
                        e = Gd[gb + SS + lane * C + r];
                        if (W && lane == r && sw[S + lane] > (T)0) e += sw[S + lane];
                    }
                }
                col[r] = e;
            }
            gj_inverse_reg<T, C>(col);
            if (lane >= C && lane < 2 * C) {
                const int cc = lane - C;
#pragma unroll
                for (int r = 0; r < C; ++r) Gi[gb + SS + cc * C + r] = (sa[1][S + cc] || sa[1][S + r]) ? (T)0 : col[r];
            }
        }
        if (lane < nk) {                                                     // g' = g + W b - H_:A b_A (0 on A: Ginv' ignores it)
            T t = g[v0 + lane];
            if (sa[1][lane]) t = (T)0;
            else {
                if (W && sw[lane] > (T)0) t = fmaT(sw[lane], ss[lane], t);
                if (W == BOUNDS_CAPPED) t += sm[lane];
                if (lane < S) {
                    for (int j = 0; j < S; ++j)
                        if (sa[1][j]) t = fmaT(-Gd[gb + j * S + lane], sb[1][j], t);
                } else {
                    for (int j = 0; j < C; ++j)
                        if (sa[1][S + j]) t = fmaT(-Gd[gb + SS + j * C + (lane - S)], sb[1][S + j], t);
                }
            }
            gp[v0 + lane] = t;
        }
        if (lane < S) {                                                      // c' = c - C_:A b_A, C's identity included
            T t = c[(size_t)k * S + lane];
            if (sa[1][lane]) t -= sb[1][lane];
            if (k > 0) {
                const T *Ck = Cd + (size_t)(k - 1) * SN;
                for (int j = 0; j < n; ++j)
                    if (sa[0][j]) t = fmaT(-Ck[lane + j * S], sb[0][j], t);
            }
            cp[(size_t)k * S + lane] = t;
        }
    }
    if (__any(bad) && lane == 0) {
        a.polish[sys] = GATO_QP_POLISH_BAD_ACTIVE;
        atomicAdd(a.bad, 1);
    }
}

// The polished point from the reduced solve (x = x' off the active set, the bound on it, z = clip(x), y_A = (g - H x -
// C^T lambda)_A, y_F = 0, lambda = lambda') and its residuals, folded per system with integer atomicMax on the bit patterns.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void polish_finish_kernel(PolishArgs a, int K, BatchStride bs)
{
    __shared__ PointLds<T, S, C> lds;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const PointSys<T> p = point_sys<T, BOUNDS_HARD>(a, sys, bs);             // the polish has no weights
    unsigned long long m[NSL];
#pragma unroll
    for (int f = 0; f < NSL; ++f) m[f] = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) polished_point_knot<T, S, C>(lds, p, k, K, lane, m);
    fold_into_slots(m, a.slots + sys * NSL, lane);
}

// The acceptance test of one system (every workgroup of it reads the same complete maxima) and, if it passes, the polished
// point over the caller's x, z, y, lambda; status CONVERGED and the residuals.  A rejected system is not written.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void polish_writeback_kernel(PolishArgs a, int K, BatchStride bs)
{
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const PointTest t = point_test(a.slots + sys * NSL, a.eps_abs, a.eps_rel);
    if (blockIdx.x == 0 && lane == 0) {
        a.polish[sys] = t.ok ? GATO_QP_POLISH_ACCEPTED : (t.finite ? GATO_QP_POLISH_REJECTED : GATO_QP_POLISH_NONFINITE);
        if (t.ok) {
            a.status[sys] = GATO_QP_CONVERGED;
            a.res[2 * sys] = t.rp;
            a.res[2 * sys + 1] = t.rd;
        }
    }
    if (t.ok) write_point<T, S, C>(a, sys, bs, K, lane);
}

// lo_bar, hi_bar and w_bar of a converged point from the adjoint [a; beta] of its last assembly.  Hard-active i: b_bar_i = xbar_i -
// (H a + C^T beta)_i - the row products of the finish step with rho 0: a_A = 0, so rho a_i vanishes there; soft-active i:
// b_bar_i = w_i a_i and w_bar_i = a_i (b_i - x_i); b_bar goes to hi_bar where act = +1 and to lo_bar where act = -1; every other
// entry of the three is 0.  Without weights lo, hi and x are not read; without w_bar it is not written.  With caps (W = BOUNDS_CAPPED,
// DESIGN.md section 3.11) a saturated i (act = +-2, s its sign) has cap_bar_i = -s a_i and 0 in the other three; cap_bar is 0 elsewhere.
template <typename T, int S, int C, int W>
__global__ __launch_bounds__(WAVE) void qp_bound_grad_kernel(BoundGradArgs q, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SN = S * n;
    __shared__ T sQ[SS], sR[CC], sCk[SN], sV[n], sLk[S], sLn[S];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *G = (const T *)q.G + sys * bs.g, *Cd = (const T *)q.Cd + sys * bs.c;
    const signed char *act = q.act + sys * bs.n;
    const T *w = sys_weights<T, W>(q.w, sys, bs);
    const T *xbar = (const T *)q.xbar + sys * bs.n, *adz = (const T *)q.adz + sys * bs.n, *beta = (const T *)q.beta + sys * bs.sk;
    T *lo_bar = (T *)q.lo_bar + sys * bs.n, *hi_bar = (T *)q.hi_bar + sys * bs.n;
    T *w_bar = W && q.w_bar ? (T *)q.w_bar + sys * bs.n : nullptr;
    const T *cap = sys_caps<T, W>(q.cap, sys, bs);
    T *cap_bar = W == BOUNDS_CAPPED && q.cap_bar ? (T *)q.cap_bar + sys * bs.n : nullptr;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int nk = k < K - 1 ? n : S;
        const size_t v0 = (size_t)k * n;
        __syncthreads();
        const T *Gk = G + (size_t)k * (SS + CC);
        for (int e = lane; e < SS; e += WAVE) sQ[e] = Gk[e];
        if (k < K - 1) {
            for (int e = lane; e < CC; e += WAVE) sR[e] = Gk[SS + e];
            for (int e = lane; e < SN; e += WAVE) sCk[e] = Cd[(size_t)k * SN + e];
        }
        if (lane < nk) sV[lane] = adz[v0 + lane];
        if (lane < S) {
            sLk[lane] = beta[(size_t)k * S + lane];
            if (k < K - 1) sLn[lane] = beta[(size_t)(k + 1) * S + lane];
        }
        __syncthreads();
        if (lane < nk) {
            const size_t v = v0 + lane;
            const signed char ai = act[v];
            T bb = (T)0, wb = (T)0, cb = (T)0;
            if (W == BOUNDS_CAPPED && cap && saturated(ai) && soft_active(ai, w, v) && __builtin_isfinite(cap[v])) {
                cb = ai > 0 ? -sV[lane] : sV[lane];
            } else if (soft_active(ai, w, v)) {
                const size_t o = sys * bs.n + v;                             // lo, hi and x: given with the weights only
                const T ad = sV[lane];
                bb = w[v] * ad;
                wb = ad * (bound_of(ai, ((const T *)q.lo)[o], ((const T *)q.hi)[o]) - ((const T *)q.x)[o]);
            } else if (ai != 0) {
                T hx, ctl;
                row_products<T, S, C>(lane, k < K - 1, sQ, sR, sCk, sV, sLk, sLn, (T)0, hx, ctl);
                bb = xbar[v] - (hx + ctl);
            }
            lo_bar[v] = ai < 0 ? bb : (T)0;
            hi_bar[v] = ai > 0 ? bb : (T)0;
            if (w_bar) w_bar[v] = wb;
            if (cap_bar) cap_bar[v] = cb;
        }
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_qp_active(const Dims &d, const void *z, const void *y, const void *lo, const void *hi, signed char *act, hipStream_t st)
{
    return launch_per_knot("qp_active", qp_active_kernel<T, S, C>, d, st, (const T *)z, (const T *)y, (const T *)lo, (const T *)hi,
                           act, d.K, batch_stride(d));
}

template <typename T, int S, int C>
int launch_polish_prepare(const Dims &d, const PolishArgs &a, hipStream_t st)
{
    return launch_per_knot("polish_prepare", GATO_BOUNDS_KERNEL(polish_prepare_kernel, bounds_form(a.w, a.cap)), d, st, a, d.K,
                           batch_stride(d));
}

template <typename T, int S, int C>
int launch_polish_finish(const Dims &d, const PolishArgs &a, hipStream_t st)
{
    const int rc = launch_per_knot("polish_finish", polish_finish_kernel<T, S, C>, d, st, a, d.K, batch_stride(d));
    return rc ? rc : launch_per_knot("polish_finish", polish_writeback_kernel<T, S, C>, d, st, a, d.K, batch_stride(d));
}

template <typename T, int S, int C>
int launch_qp_bound_grad(const Dims &d, const BoundGradArgs &a, hipStream_t st)
{
    // with w_bar alone (the soft entry without weights) the W kernel finds no weight at run time and writes w_bar = 0
    // with cap_bar alone (the capped entry without caps) the capped kernel finds no cap at run time and writes cap_bar = 0
    const int form = a.cap || a.cap_bar ? BOUNDS_CAPPED : (a.w || a.w_bar ? BOUNDS_SOFT : BOUNDS_HARD);
    return launch_per_knot("qp_bound_grad", GATO_BOUNDS_KERNEL(qp_bound_grad_kernel, form), d, st, a, d.K, batch_stride(d));
}

#define X(S_, C_)                                                                                                            \
    template int launch_qp_active<float, S_, C_>(const Dims &, const void *, const void *, const void *, const void *,        \
                                                 signed char *, hipStream_t);                                               \
    template int launch_qp_active<double, S_, C_>(const Dims &, const void *, const void *, const void *, const void *,       \
                                                  signed char *, hipStream_t);                                              \
    template int launch_polish_prepare<float, S_, C_>(const Dims &, const PolishArgs &, hipStream_t);                       \
    template int launch_polish_prepare<double, S_, C_>(const Dims &, const PolishArgs &, hipStream_t);                      \
    template int launch_polish_finish<float, S_, C_>(const Dims &, const PolishArgs &, hipStream_t);                        \
    template int launch_polish_finish<double, S_, C_>(const Dims &, const PolishArgs &, hipStream_t);                       \
    template int launch_qp_bound_grad<float, S_, C_>(const Dims &, const BoundGradArgs &, hipStream_t);                     \
    template int launch_qp_bound_grad<double, S_, C_>(const Dims &, const BoundGradArgs &, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
