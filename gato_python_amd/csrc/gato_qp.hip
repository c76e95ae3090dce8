// Box-constrained QP solves by ADMM over the KKT re-solve (gato_box_qp_solve):
//   min 1/2 x^T H x - g^T x   s.t.  C x = c,  lo <= x <= hi,   H = G + rho_reg I
// in the OSQP splitting with the dynamics kept as hard equality constraints.  The x-step matrix
// [[H + sigma I + diag(rho_i), C^T], [C, 0]] is assembled once per QP (the whole solve on G' = G + diag(sigma + rho_i));
// every iteration after the first is one warm-started re-solve plus one qp_update_kernel launch.
#include "gato_common.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NSL = GATO_QP_NSLOT;
// slot fields: the two residuals, then the scales of the tolerance test, then |g~| of the next x-step
enum { F_PRIM, F_DUAL, F_X, F_Z, F_C, F_HX, F_CTL, F_Y, F_G, F_GT };

// penalty of one variable: 0 free (both bounds infinite), 1e3 admm_rho for an equality (lo == hi), admm_rho otherwise
template <typename T>
__device__ __forceinline__ T penalty(T lo, T hi, T admm_rho)
{
    if (lo == -(T)INFINITY && hi == (T)INFINITY) return (T)0;
    return lo == hi ? (T)1e3 * admm_rho : admm_rho;
}

// One wave per knot (grid.x strides over the knots, grid.y = system), lane i = variable i of the knot.
// Classifies the bounds, writes rho_i, G' = G + diag(sigma + rho_i), z0 = x0 = clip(z_init or 0), y0 (0 on free variables)
// and g~0 = g + sigma x0 + rho z0 - y0; |g~0| and |c| go into slot 2 (read by launch 0 of qp_update_kernel: a zero
// right-hand side).  A NaN bound or lo > hi marks the system BAD_BOUNDS.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void qp_prepare_kernel(QpArgs a, int K, int B, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *G = (const T *)a.G + sys * bs.g, *g = (const T *)a.g + sys * bs.n, *c = (const T *)a.c + sys * bs.sk;
    const T *lo = (const T *)a.lo + sys * bs.n, *hi = (const T *)a.hi + sys * bs.n;
    T *Gp = (T *)a.Gp + sys * bs.g, *rho = (T *)a.rho + sys * bs.n, *x0 = (T *)a.xw + sys * bs.n;
    T *x = (T *)a.x + sys * bs.n, *z = (T *)a.z + sys * bs.n, *y = (T *)a.y + sys * bs.n, *gt = (T *)a.gt + sys * bs.n;
    const T sigma = (T)a.sigma, arho = (T)a.admm_rho;
    if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) a.ctr[0] = B;
    unsigned long long mg = 0, mc = 0;
    int bad = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int nk = k < K - 1 ? n : S;
        const size_t v0 = (size_t)k * n, gb = (size_t)k * (SS + CC);
        for (int e = lane; e < (k < K - 1 ? SS + CC : SS); e += WAVE) {     // G' (column-major Q_k, then R_k)
            int i = -1;
            if (e < SS) { if (e % S == e / S) i = e % S; }
            else if ((e - SS) % C == (e - SS) / C) i = S + (e - SS) % C;
            T w = G[gb + e];
            if (i >= 0) w += sigma + penalty(lo[v0 + i], hi[v0 + i], arho);
            Gp[gb + e] = w;
        }
        if (lane < nk) {
            const size_t v = v0 + lane;
            const T l = lo[v], h = hi[v];
            if (l != l || h != h || l > h) bad = 1;
            const T r = penalty(l, h, arho);
            const T zi = clip(a.warm ? z[v] : (T)0, l, h);
            const T yi = (a.warm && r != (T)0) ? y[v] : (T)0;
            T t = fmaT(sigma, zi, g[v]);
            t = fmaT(r, zi, t) - yi;
            rho[v] = r; x0[v] = zi; x[v] = zi; z[v] = zi; y[v] = yi; gt[v] = t;
            mg = mag_bits(t) > mg ? mag_bits(t) : mg;
            if (lane < S) mc = mag_bits(c[(size_t)k * S + lane]) > mc ? mag_bits(c[(size_t)k * S + lane]) : mc;
        }
    }
    mg = wave_max_bits(mg);
    mc = wave_max_bits(mc);
    const int anybad = __any(bad);
    if (lane == 0) {
        unsigned long long *sl = a.slots + (sys * 3 + 2) * NSL;
        atomicMax(sl + F_GT, mg);
        atomicMax(sl + F_C, mc);
        if (anybad) { a.status[sys] = GATO_QP_BAD_BOUNDS; atomicAdd(a.ctr + 1, 1); }
    }
}

// Iteration `it`.  Every workgroup of a system first reads the maxima of the iterate launch it-1
// wrote (slot (it-1) % 3): if they pass the test the system is frozen - its knot-0 workgroup alone records iters = it, the
// status and the two residuals - and nothing of it is written again.  Otherwise, per knot, from the x-step's solution
// (x~, lambda~):
//   x^ = alpha x~ + (1-alpha) z,  x+ = alpha x~ + (1-alpha) x,  z+ = clip(x^ + y / rho, lo, hi),  y+ = y + rho (x^ - z+)
//   (free variables: z+ = x^, y+ = 0),  lambda+ = lambda~,  g~+ = g + sigma x+ + rho z+ - y+
// and the true QP residuals of (x+, z+, lambda+, y+) on the knot's rows, folded into slot it % 3 with integer atomicMax
// on the bit patterns (exact in any order: no float atomics).  C x needs knot k-1's x+, recomputed here from x~ and x (the
// x of the iterations ping-pong between two buffers, so no wave reads what another writes); C^T lambda needs lambda~ of
// knot k+1.  A system whose x-step right-hand side was all zero (|g~| = |c| = 0) takes x~ = lambda~ = 0: its PCG formed 0/0.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void qp_update_kernel(QpArgs a, int it, int last, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SN = S * n;
    __shared__ T sQ[SS], sR[CC], sCp[SN], sCk[SN], sXn[n], sXp[n], sLk[S], sLn[S];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    if (a.status[sys] >= 0) return;                                        // frozen (or never started)
    unsigned long long *slots = a.slots + sys * 3 * NSL;
    bool zero_rhs;
    {
        const unsigned long long *prev = slots + ((it + 2) % 3) * NSL;
        if (it > 0) {
            const double rp = slot_val(prev, F_PRIM), rd = slot_val(prev, F_DUAL);
            const double sp = fmax(fmax(slot_val(prev, F_X), slot_val(prev, F_Z)), slot_val(prev, F_C));
            const double sd = fmax(fmax(slot_val(prev, F_HX), slot_val(prev, F_CTL)), fmax(slot_val(prev, F_Y), slot_val(prev, F_G)));
            const bool finite = __builtin_isfinite(rp) && __builtin_isfinite(rd);
            const bool conv = finite && rp <= a.eps_abs + a.eps_rel * sp && rd <= a.eps_abs + a.eps_rel * sd;
            if (!finite || conv || last) {
                if (blockIdx.x == 0 && lane == 0) {
                    a.status[sys] = !finite ? GATO_QP_NONFINITE : (conv ? GATO_QP_CONVERGED : GATO_QP_MAX_ITERS);
                    a.iters[sys] = it;
                    a.res[2 * sys] = rp;
                    a.res[2 * sys + 1] = rd;
                    atomicSub(a.ctr, 1);
                }
                return;
            }
        }
        zero_rhs = prev[F_GT] == 0 && prev[F_C] == 0;
    }
    if (blockIdx.x == 0) {
        if (lane < NSL) slots[((it + 1) % 3) * NSL + lane] = 0;           // the slot launch it+1 folds into
        if (lane == 0 && a.pcg_its) a.pcg_total[sys] += a.pcg_its[sys];
    }
    unsigned long long *cur = slots + (it % 3) * NSL;
    const T *G = (const T *)a.G + sys * bs.g, *Cd = (const T *)a.Cd + sys * bs.c;
    const T *g = (const T *)a.g + sys * bs.n, *c = (const T *)a.c + sys * bs.sk;
    const T *lo = (const T *)a.lo + sys * bs.n, *hi = (const T *)a.hi + sys * bs.n, *rho = (const T *)a.rho + sys * bs.n;
    const T *xr = (const T *)a.xr + sys * bs.n, *xt = (const T *)a.xt + sys * bs.n;
    T *xw = (T *)a.xw + sys * bs.n, *x = (T *)a.x + sys * bs.n, *z = (T *)a.z + sys * bs.n, *y = (T *)a.y + sys * bs.n;
    T *gt = (T *)a.gt + sys * bs.n, *lam = (T *)a.lam + sys * bs.sk, *lt = (T *)a.lt + sys * bs.sk;
    const T alpha = (T)a.alpha, beta = (T)1 - alpha, sigma = (T)a.sigma, rreg = (T)a.rho_reg;
    unsigned long long m[NSL];
#pragma unroll
    for (int f = 0; f < NSL; ++f) m[f] = 0;
    auto fold = [&](int f, T v) { const unsigned long long b = mag_bits(v); m[f] = b > m[f] ? b : m[f]; };
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int nk = k < K - 1 ? n : S;
        const size_t v0 = (size_t)k * n;
        __syncthreads();                                                     // the previous knot's readers are done
        const T *Gk = G + (size_t)k * (SS + CC);
        for (int e = lane; e < SS; e += WAVE) sQ[e] = Gk[e];
        if (k < K - 1) {
            for (int e = lane; e < CC; e += WAVE) sR[e] = Gk[SS + e];
            for (int e = lane; e < SN; e += WAVE) sCk[e] = Cd[(size_t)k * SN + e];
        }
        if (k > 0)
            for (int e = lane; e < SN; e += WAVE) sCp[e] = Cd[(size_t)(k - 1) * SN + e];
        T xn = 0, zn = 0, yn = 0;
        if (lane < nk) {
            const size_t v = v0 + lane;
            const T xs = zero_rhs ? (T)0 : xt[v];
            const T xh = fmaT(alpha, xs, beta * z[v]);
            xn = fmaT(alpha, xs, beta * xr[v]);
            const T r = rho[v];
            if (r == (T)0) { zn = xh; yn = (T)0; }
            else {
                const T yv = y[v];
                zn = clip(xh + yv / r, lo[v], hi[v]);
                yn = fmaT(r, xh - zn, yv);
            }
            sXn[lane] = xn;
        }
        if (k > 0 && lane < n) {                                            // knot k-1's x+ (always a full knot)
            const size_t v = v0 - n + lane;
            sXp[lane] = fmaT(alpha, zero_rhs ? (T)0 : xt[v], beta * xr[v]);
        }
        if (lane < S) {
            sLk[lane] = zero_rhs ? (T)0 : lt[(size_t)k * S + lane];
            if (k < K - 1) sLn[lane] = zero_rhs ? (T)0 : lt[(size_t)(k + 1) * S + lane];
        }
        __syncthreads();
        if (lane < nk) {
            const int i = lane;
            const size_t v = v0 + i;
            T hx = (T)0, ctl = (T)0;
            if (i < S) {
#pragma unroll 4
                for (int cc = 0; cc < S; ++cc) hx = fmaT(sQ[i + cc * S], sXn[cc], hx);
                ctl = sLk[i];
            } else {
#pragma unroll 4
                for (int cc = 0; cc < C; ++cc) hx = fmaT(sR[(i - S) + cc * C], sXn[S + cc], hx);
            }
            hx = fmaT(rreg, xn, hx);
            if (k < K - 1) {
#pragma unroll 4
                for (int r = 0; r < S; ++r) ctl = fmaT(sCk[r + i * S], sLn[r], ctl);
            }
            const T gv = g[v];
            const T rd = (hx - gv) + ctl + yn;
            const T r = rho[v];
            T t = fmaT(sigma, xn, gv);
            t = fmaT(r, zn, t) - yn;
            xw[v] = xn; x[v] = xn; z[v] = zn; y[v] = yn; gt[v] = t;
            fold(F_PRIM, xn - zn);
            fold(F_DUAL, rd);
            fold(F_X, xn);
            fold(F_Z, zn);
            fold(F_HX, hx);
            fold(F_CTL, ctl);
            fold(F_Y, yn);
            fold(F_G, gv);
            fold(F_GT, t);
            if (i < S) {                                                    // row block k of C x - c
                const T ci = c[(size_t)k * S + i];
                T cx = xn;
                if (k > 0) {
#pragma unroll 4
                    for (int j = 0; j < n; ++j) cx = fmaT(sCp[i + j * S], sXp[j], cx);
                }
                fold(F_PRIM, cx - ci);
                fold(F_C, ci);
                lam[(size_t)k * S + i] = sLk[i];
                if (zero_rhs) lt[(size_t)k * S + i] = (T)0;   // the next warm start from 0, not from 0/0
            }
        }
    }
    // the slot only grows: a wave whose maximum it already holds skips the atomic (most waves, once a large value is in)
#pragma unroll
    for (int f = 0; f < NSL; ++f) {
        const unsigned long long w = wave_max_bits(m[f]);
        if (lane == 0 && w != 0 && w > __hip_atomic_load(cur + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(cur + f, w);
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_qp_prepare(const Dims &d, const QpArgs &a, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("qp_prepare: B = %d", d.B); return GATO_EINVAL; }
    const int gx = d.K < 8192 ? d.K : 8192;
    hipLaunchKernelGGL((qp_prepare_kernel<T, S, C>), dim3(gx, d.B), dim3(WAVE), 0, st, a, d.K, d.B, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

template <typename T, int S, int C>
int launch_qp_update(const Dims &d, const QpArgs &a, int it, int last, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("qp_update: B = %d", d.B); return GATO_EINVAL; }
    const int gx = last ? 1 : (d.K < 8192 ? d.K : 8192);                // the test alone: one workgroup per system
    hipLaunchKernelGGL((qp_update_kernel<T, S, C>), dim3(gx, d.B), dim3(WAVE), 0, st, a, it, last, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

#define X(S_, C_)                                                                                       \
    template int launch_qp_prepare<float, S_, C_>(const Dims &, const QpArgs &, hipStream_t);          \
    template int launch_qp_prepare<double, S_, C_>(const Dims &, const QpArgs &, hipStream_t);         \
    template int launch_qp_update<float, S_, C_>(const Dims &, const QpArgs &, int, int, hipStream_t); \
    template int launch_qp_update<double, S_, C_>(const Dims &, const QpArgs &, int, int, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
