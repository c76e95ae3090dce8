// Device helpers of the box-QP kernels (gato_qp.hip, gato_polish.hip, gato_pdas.hip).  Internal header.
#pragma once
#include "gato_common.h"

namespace gato {
namespace {

// workgroups per system of the one-wave-per-knot kernels: the knots past it are a second pass of the knot loop
inline int knot_grid(int K) { return K < 8192 ? K : 8192; }

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

// ---- the polished point of a reduced solve, shared by the polish (gato_polish.hip) and the active-set iteration (gato_pdas.hip)
// slot fields: the residuals and scales of the ADMM termination test, the largest wrong-sign multiplier, |lambda|
namespace polf {
enum { F_PRIM, F_DUAL, F_X, F_Z, F_C, F_HX, F_CTL, F_Y, F_G, F_SIGN, F_LAM, F_END };
}
static_assert(polf::F_END <= GATO_POLISH_NSLOT, "slot fields");

template <typename T>
__device__ __forceinline__ T bound_of(signed char act, T lo, T hi) { return act > 0 ? hi : (act < 0 ? lo : (T)0); }

// An act the reduced system cannot take: not -1 / 0 / 1, an infinite bound b = bound_of(act, lo, hi), or a state of x_0.
template <typename T>
__device__ __forceinline__ bool bad_active(signed char act, T b, bool x0)
{
    return act < -1 || act > 1 || (act != 0 && (!__builtin_isfinite(b) || x0));
}

// Capped soft bounds: act = +-2 names a saturated variable - its penalty force is held at the cap.
__device__ __forceinline__ bool saturated(signed char act) { return act == 2 || act == -2; }

// bad_active where caps are given: +-2 is an act too, but only on a variable with a weight w > 0 and a finite cap m (the bound
// finite and off x_0, as for every active variable).
template <typename T>
__device__ __forceinline__ bool bad_active_capped(signed char act, T b, bool x0, T w, T m)
{
    if (act < -2 || act > 2) return true;
    if (saturated(act) && !(w > (T)0 && __builtin_isfinite(m))) return true;
    return act != 0 && (!__builtin_isfinite(b) || x0);
}

// Row i of knot k of H v and C^T w, the products of qp_update_kernel: (G v)_i + rho v_i and w_k,i (states) + (C_k^T w_k+1)_i.
// sQ, sR: the knot's G blocks (without rho); sCk: C block k (rows of block row k+1); sV: v of the knot; sLk, sLn: w_k, w_k+1.
template <typename T, int S, int C>
__device__ __forceinline__ void row_products(int i, bool next, const T *sQ, const T *sR, const T *sCk, const T *sV, const T *sLk,
                                             const T *sLn, T rho, T &hx, T &ctl)
{
    hx = (T)0;
    ctl = (T)0;
    if (i < S) {
#pragma unroll 4
        for (int cc = 0; cc < S; ++cc) hx = fmaT(sQ[i + cc * S], sV[cc], hx);
        ctl = sLk[i];
    } else {
#pragma unroll 4
        for (int cc = 0; cc < C; ++cc) hx = fmaT(sR[(i - S) + cc * C], sV[S + cc], hx);
    }
    hx = fmaT(rho, sV[i], hx);
    if (next) {
#pragma unroll 4
        for (int r = 0; r < S; ++r) ctl = fmaT(sCk[r + i * S], sLn[r], ctl);
    }
}

// The form of the bounds a kernel is instantiated for (its template parameter W): all hard, soft weights, weights and caps.
enum { BOUNDS_HARD = 0, BOUNDS_SOFT = 1, BOUNDS_CAPPED = 2 };
inline int bounds_form(const void *w, const void *cap) { return w ? (cap ? BOUNDS_CAPPED : BOUNDS_SOFT) : BOUNDS_HARD; }

// The soft weights of system sys (w: [B][N]) in a kernel instantiated with weights (W); nullptr = all hard in one without: every
// test of it is then decided at compile time and the hard code is what it was before there were weights.
template <typename T, int W>
__device__ __forceinline__ const T *sys_weights(const void *w, size_t sys, const BatchStride &bs)
{
    return W && w ? (const T *)w + sys * bs.n : nullptr;
}
// The caps of system sys in a kernel instantiated with caps, nullptr in every other: no capped branch is compiled there.
template <typename T, int W>
__device__ __forceinline__ const T *sys_caps(const void *cap, size_t sys, const BatchStride &bs)
{
    return W == BOUNDS_CAPPED && cap ? (const T *)cap + sys * bs.n : nullptr;
}

// One system's arrays of PolishArgs, and the LDS one wave stages a knot in.
template <typename T>
struct PointSys {
    const T *G, *Cd, *g, *c, *lo, *hi, *xt, *lt;
    const T *w;                              // the system's soft weights, nullptr = all hard
    const T *cap;                            // the caps of the penalty force, nullptr = none
    const signed char *act;
    T *xp, *zp, *yp;
    T rho;
};
// W: the kernel is the instantiation with weights; without, w is a compile-time nullptr and no soft branch is compiled
template <typename T, int W>
__device__ __forceinline__ PointSys<T> point_sys(const PolishArgs &a, size_t sys, const BatchStride &bs)
{
    return PointSys<T>{(const T *)a.G + sys * bs.g,  (const T *)a.Cd + sys * bs.c,  (const T *)a.g + sys * bs.n,
                       (const T *)a.c + sys * bs.sk, (const T *)a.lo + sys * bs.n,  (const T *)a.hi + sys * bs.n,
                       (const T *)a.xt + sys * bs.n, (const T *)a.lt + sys * bs.sk, sys_weights<T, W>(a.w, sys, bs),
                       sys_caps<T, W>(a.cap, sys, bs),
                       a.act + sys * bs.n,           (T *)a.xp + sys * bs.n,        (T *)a.zp + sys * bs.n,
                       (T *)a.yp + sys * bs.n,       (T)a.rho};
}
template <typename T, int S, int C>
struct PointLds { T sQ[S * S], sR[C * C], sCp[S * (S + C)], sCk[S * (S + C)], sXn[S + C], sXp[S + C], sLk[S], sLn[S]; };
// what lane i keeps of variable i of the knot (on = false: the lane has no variable)
template <typename T>
struct PointVar { bool on; signed char act; T x, y, lo, hi; };

// Variable v of a system is soft-active: it is active and its weight is positive (w: the system's
// weights, nullptr = all hard).
template <typename T>
__device__ __forceinline__ bool soft_active(signed char act, const T *w, size_t v) { return act != 0 && w && w[v] > (T)0; }

// Knot k of the polished point from the reduced solve (x = x' off the active set, the bound on it, z = clip(x), y_A = (g - H x -
// C^T lambda)_A, y_F = 0) to xp, zp, yp, and its residuals folded into the lane's maxima m.  A soft-active variable keeps the
// reduced solution x', its multiplier is the penalty force y = w (x - b) and z = x (the violation is allowed); H in the residuals
// is without W.  With p.w nullptr or 0 no variable is soft-active.  With caps (p.cap) a saturated
// variable (act = +-2, s its sign) has y = s m bit for bit, and the sign slot also takes what keeps an act to its point: max(|y|
// - m, 0) of a soft quadratic-active variable, max(m - s w (x - b), 0) of a saturated one.  The whole wave calls it.
template <typename T, int S, int C>
__device__ __forceinline__ PointVar<T> polished_point_knot(PointLds<T, S, C> &L, const PointSys<T> &p, int k, int K, int lane,
                                                           unsigned long long (&m)[GATO_POLISH_NSLOT])
{
    using namespace polf;
    constexpr int WAVE = 64, n = S + C, SS = S * S, CC = C * C, SN = S * n;
    auto fold = [&](int f, T v) { const unsigned long long b = mag_bits(v); m[f] = b > m[f] ? b : m[f]; };
    const int nk = k < K - 1 ? n : S;
    const size_t v0 = (size_t)k * n;
    PointVar<T> out{false, 0, (T)0, (T)0, (T)0, (T)0};
    __syncthreads();
    const T *Gk = p.G + (size_t)k * (SS + CC);
    for (int e = lane; e < SS; e += WAVE) L.sQ[e] = Gk[e];
    if (k < K - 1) {
        for (int e = lane; e < CC; e += WAVE) L.sR[e] = Gk[SS + e];
        for (int e = lane; e < SN; e += WAVE) L.sCk[e] = p.Cd[(size_t)k * SN + e];
    }
    if (k > 0)
        for (int e = lane; e < SN; e += WAVE) L.sCp[e] = p.Cd[(size_t)(k - 1) * SN + e];
    if (lane < nk) {
        const size_t v = v0 + lane;
        const signed char ai = p.act[v];
        L.sXn[lane] = (ai != 0 && !soft_active(ai, p.w, v)) ? bound_of(ai, p.lo[v], p.hi[v]) : p.xt[v];
    }
    if (k > 0 && lane < n) {                                            // knot k-1's x (always a full knot)
        const size_t v = v0 - n + lane;
        const signed char ai = p.act[v];
        L.sXp[lane] = (ai != 0 && !soft_active(ai, p.w, v)) ? bound_of(ai, p.lo[v], p.hi[v]) : p.xt[v];
    }
    if (lane < S) {
        L.sLk[lane] = p.lt[(size_t)k * S + lane];
        if (k < K - 1) L.sLn[lane] = p.lt[(size_t)(k + 1) * S + lane];
    }
    __syncthreads();
    if (lane < nk) {
        const int i = lane;
        const size_t v = v0 + i;
        const signed char ai = p.act[v];
        const bool soft = soft_active(ai, p.w, v);
        T hx, ctl;
        row_products<T, S, C>(i, k < K - 1, L.sQ, L.sR, L.sCk, L.sXn, L.sLk, L.sLn, p.rho, hx, ctl);
        const T gv = p.g[v], l = p.lo[v], h = p.hi[v], xn = L.sXn[i];
        T zn = clip(xn, l, h);
        T yn = ai != 0 ? (gv - hx) - ctl : (T)0;
        T over = (T)0;                                                  // capped: how far the force is on the wrong side of its cap
        if (soft) {
            zn = xn;
            yn = p.w[v] * (xn - bound_of(ai, l, h));
            if (p.cap) {
                const T mi = p.cap[v];
                if (saturated(ai)) {
                    const T sf = ai > 0 ? yn : -yn;
                    over = mi - sf;
                    yn = ai > 0 ? mi : -mi;
                } else over = fabs(yn) - mi;
            }
        }
        const T rd = (hx - gv) + ctl + yn;
        p.xp[v] = xn; p.zp[v] = zn; p.yp[v] = yn;
        fold(F_PRIM, xn - zn);
        fold(F_DUAL, rd);
        fold(F_X, xn);
        fold(F_Z, zn);
        fold(F_HX, hx);
        fold(F_CTL, ctl);
        fold(F_Y, yn);
        fold(F_G, gv);
        if (ai != 0 && l != h) {                                        // the multiplier's sign: y >= 0 upper, <= 0 lower
            const T ws = ai > 0 ? -yn : yn;
            fold(F_SIGN, ws > (T)0 ? ws : (T)0);
        }
        if (p.cap && soft) fold(F_SIGN, over > (T)0 ? over : (T)0);
        if (i < S) {                                                    // row block k of C x - c
            const T ci = p.c[(size_t)k * S + i];
            T cx = xn;
            if (k > 0) {
#pragma unroll 4
                for (int j = 0; j < n; ++j) cx = fmaT(L.sCp[i + j * S], L.sXp[j], cx);
            }
            fold(F_PRIM, cx - ci);
            fold(F_C, ci);
            fold(F_LAM, L.sLk[i]);
        }
        out = PointVar<T>{true, ai, xn, yn, l, h};
    }
    return out;
}

// The lanes' maxima into the system's slots sl.  The slot only grows: a wave whose maximum it already holds skips the atomic
// (most waves of a long system: every wave of it folds into the same eleven words).
__device__ __forceinline__ void fold_into_slots(const unsigned long long (&m)[GATO_POLISH_NSLOT], unsigned long long *sl, int lane)
{
#pragma unroll
    for (int f = 0; f < polf::F_END; ++f) {
        const unsigned long long w = wave_max_bits(m[f]);
        if (lane == 0 && w != 0 && w > __hip_atomic_load(sl + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(sl + f, w);
    }
}

// The acceptance test on a system's complete maxima: every one finite, the termination test of the ADMM loop, and the largest
// wrong-sign multiplier within the dual tolerance.
struct PointTest { bool finite, ok; double rp, rd; };
__device__ __forceinline__ PointTest point_test(const unsigned long long *sl, double eps_abs, double eps_rel)
{
    using namespace polf;
    bool finite = true;
#pragma unroll
    for (int f = 0; f < F_END; ++f) finite = finite && __builtin_isfinite(slot_val(sl, f));
    const double rp = slot_val(sl, F_PRIM), rd = slot_val(sl, F_DUAL);
    const double sp = fmax(fmax(slot_val(sl, F_X), slot_val(sl, F_Z)), slot_val(sl, F_C));
    const double sd = fmax(fmax(slot_val(sl, F_HX), slot_val(sl, F_CTL)), fmax(slot_val(sl, F_Y), slot_val(sl, F_G)));
    const double tol_d = eps_abs + eps_rel * sd;
    const bool ok = finite && rp <= eps_abs + eps_rel * sp && rd <= tol_d && slot_val(sl, F_SIGN) <= tol_d;
    return PointTest{finite, ok, rp, rd};
}

// The polished point of system sys (xp, zp, yp and the reduced solve's lambda) over the caller's x, z, y, lambda: this
// workgroup's knots.
template <typename T, int S, int C>
__device__ __forceinline__ void write_point(const PolishArgs &a, size_t sys, const BatchStride &bs, int K, int lane)
{
    constexpr int n = S + C;
    const T *xp = (const T *)a.xp + sys * bs.n, *zp = (const T *)a.zp + sys * bs.n, *yp = (const T *)a.yp + sys * bs.n;
    const T *lt = (const T *)a.lt + sys * bs.sk;
    T *x = (T *)a.x + sys * bs.n, *z = (T *)a.z + sys * bs.n, *y = (T *)a.y + sys * bs.n, *lam = (T *)a.lam + sys * bs.sk;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t v = (size_t)k * n + lane;
            x[v] = xp[v]; z[v] = zp[v]; y[v] = yp[v];
        }
        if (lane < S) lam[(size_t)k * S + lane] = lt[(size_t)k * S + lane];
    }
}

// ---- host side: what the units' launch wrappers share --------------------------------------------------------------------------
// The one-wave-per-knot launch of `kernel` with args: knot_grid(d.K) workgroups of one wave for each of the d.B systems (the
// grid's y, hence B <= 65535).  name: the wrapper's, in the refusal of a B out of range.
constexpr int KNOT_THREADS = 64;            // one wave: the WAVE of every unit, the __launch_bounds__ of these kernels
template <typename... P, typename... A>
inline int launch_per_knot(const char *name, void (*kernel)(P...), const Dims &d, hipStream_t st, const A &...args)
{
    if (d.B < 1 || d.B > 65535) { set_error("%s: B = %d", name, d.B); return GATO_EINVAL; }
    hipLaunchKernelGGL(kernel, dim3(knot_grid(d.K), d.B), dim3(KNOT_THREADS), 0, st, args...);
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

// The instantiation of kernel template k<T, S, C, W> for a form of the bounds (BOUNDS_*).  For the units' launch wrappers only:
// it names their template parameters T, S and C, and stays defined to the end of the unit.
#define GATO_BOUNDS_KERNEL(k, form) \
    ((form) == BOUNDS_CAPPED ? k<T, S, C, BOUNDS_CAPPED> : (form) == BOUNDS_SOFT ? k<T, S, C, BOUNDS_SOFT> : k<T, S, C, BOUNDS_HARD>)

}  // namespace
}  // namespace gato
