// Exact line search of the soft active-set iteration (gato_box_qp_pdas_ls, gato_box_qp_line_search).
// With every bounded variable soft the problem is the C1, strongly convex, piecewise-quadratic phi(x) = 1/2 x^T H x - g^T x +
// sum h_i(dist(x_i, [lo_i, hi_i])) on C x = c, the reduced solve on the act named by the iterate xc is its Newton point x+, and
// along d = x+ - xc the slope
//     phi'(alpha) = d^T (H xc - g) + alpha d^T H d + sum_i d_i f_i(xc_i + alpha d_i),   f = clamp(w (x - clip(x, lo, hi)), -m, m),
// is continuous, piecewise linear and non-decreasing: the step length is its root in (0, 1), or 1.
//   ls_knot_kernel     one wave per knot (grid as pdas_step_kernel): the knot's d_k^T (H_k xc_k - g_k) and d_k^T H_k d_k as doubles
//   ls_system_kernel   one workgroup per system: the sums in a fixed order, alpha by bisection down to one linear piece and a
//                      secant step on it, then the stepped iterate and - in the loop - act' of it and its changed count
//   ls_scope_kernel    the option's scope: a finite bound off x_0 without a weight is BAD_BOUNDS
// No float atomics and fixed summation orders: a run repeats bit for bit.
#include "gato_common.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NSL = GATO_POLISH_NSLOT;
constexpr int LS_THREADS = 256;
constexpr int LS_BISECTIONS = 64;

template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void ls_scope_kernel(LineSearchArgs a, int K, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *lo = (const T *)a.lo + sys * bs.n, *hi = (const T *)a.hi + sys * bs.n, *w = (const T *)a.w + sys * bs.n;
    int bad = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S) && !(k == 0 && lane < S)) {
            const size_t v = (size_t)k * n + lane;
            if ((__builtin_isfinite(lo[v]) || __builtin_isfinite(hi[v])) && !(w[v] > (T)0)) bad = 1;
        }
    }
    const int any = __any(bad);
    if (lane == 0 && any) { atomicMax(a.status_out + sys, GATO_QP_BAD_BOUNDS); atomicAdd(a.bad, 1); }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Knot k of d = x+ - xc and its two partial sums; the block rows of H as row_products takes them (G_k v + rho v, in T).
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void ls_knot_kernel(LineSearchArgs a, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C;
    __shared__ T sQ[SS], sR[CC], sX[n], sD[n];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    if (a.status && a.status[sys] >= 0) return;                         // frozen before this solve
    const T *G = (const T *)a.G + sys * bs.g, *g = (const T *)a.g + sys * bs.n;
    const T *xc = (const T *)a.xc + sys * bs.n, *xp = (const T *)a.xp + sys * bs.n;
    double *part = a.part + sys * (size_t)K * 2;
    const T rho = (T)a.rho;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int nk = k < K - 1 ? n : S;
        const size_t v = (size_t)k * n + lane;
        const T *Gk = G + (size_t)k * (SS + CC);
        __syncthreads();
        for (int e = lane; e < SS; e += WAVE) sQ[e] = Gk[e];
        if (k < K - 1)
            for (int e = lane; e < CC; e += WAVE) sR[e] = Gk[SS + e];
        if (lane < nk) {
            const T x = xc[v];
            sX[lane] = x;
            sD[lane] = xp[v] - x;
        }
        __syncthreads();
        double t0 = 0.0, t1 = 0.0;
        if (lane < nk) {
            T hx, hd, unused;
            row_products<T, S, C>(lane, false, sQ, sR, sQ, sX, sX, sX, rho, hx, unused);
            row_products<T, S, C>(lane, false, sQ, sR, sQ, sD, sD, sD, rho, hd, unused);
            const double dv = (double)sD[lane];
            t0 = dv * ((double)hx - (double)g[v]);
            t1 = dv * (double)hd;
        }
        t0 = wave_sum(t0);
        t1 = wave_sum(t1);
        if (lane == 0) { part[2 * k] = t0; part[2 * k + 1] = t1; }
    }
}

// The workgroup's sums of v and c, the same in every thread: the waves' butterflies, then the four waves in a fixed tree.
struct LsRed { double s[LS_THREADS / WAVE]; int c[LS_THREADS / WAVE]; };
__device__ __forceinline__ void block_sum(LsRed &L, double &v, int &c, int tid)
{
    v = wave_sum(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();                                                    // the reads of the round before
    if ((tid & 63) == 0) { L.s[tid >> 6] = v; L.c[tid >> 6] = c; }
    __syncthreads();
    v = (L.s[0] + L.s[1]) + (L.s[2] + L.s[3]);
    c = (L.c[0] + L.c[1]) + (L.c[2] + L.c[3]);
}

// One system's vectors, and what the slope reads of variable i: the weight (0 on the states of x_0 and where it is not positive)
// and the cap (+inf without caps).
template <typename T>
struct LsSys {
    const T *lo, *hi, *w, *cap, *xc, *xp;
    int S;
    __device__ __forceinline__ double weight(size_t i) const { return i >= (size_t)S && w[i] > (T)0 ? (double)w[i] : 0.0; }
    __device__ __forceinline__ double max_force(size_t i) const { return cap ? (double)cap[i] : (double)INFINITY; }
};

__device__ __forceinline__ double penalty_force(double x, double lo, double hi, double w, double m)
{
    const double t = w * (x - (x < lo ? lo : (x > hi ? hi : x)));
    return t > m ? m : (t < -m ? -m : t);
}

// sum_i d_i f_i(xc_i + alpha d_i), and the count of breakpoints of the slope - lo, hi, lo - m / w, hi + m / w of every soft
// variable - strictly between the points at bl and bh.
template <typename T>
__device__ __forceinline__ void penalty_slope(LsRed &L, const LsSys<T> &p, size_t N, double alpha, double bl, double bh, int tid,
                                              double &sum, int &count)
{
    sum = 0.0;
    count = 0;
    for (size_t i = tid; i < N; i += LS_THREADS) {
        const double w = p.weight(i);
        if (w > 0.0) {
            const double x = (double)p.xc[i], d = (double)p.xp[i] - x, lo = (double)p.lo[i], hi = (double)p.hi[i], m = p.max_force(i);
            sum += d * penalty_force(fma(alpha, d, x), lo, hi, w, m);
            const double xl = fma(bl, d, x), xh = fma(bh, d, x), r = m / w;
            const double bp[4] = {lo, hi, lo - r, hi + r};
#pragma unroll
            for (int j = 0; j < 4; ++j) count += (xl - bp[j]) * (xh - bp[j]) < 0.0;
        }
    }
    block_sum(L, sum, count, tid);
}

// act' of a variable from the iterate alone: the soft rule of pdas_step_kernel (sections 3.10, 3.11), the capped rule's products
// in T.  Every bounded variable is soft here; one without a weight has no bound and stays 0.
template <typename T>
__device__ __forceinline__ signed char soft_next_act(T x, T lo, T hi, T w, bool capped, T mi, bool x0)
{
    if (x0) return 0;
    if (capped) {
        const T fh = w * (x - hi), fl = w * (x - lo);
        if (lo == hi) return fh > mi ? 2 : (-fh > mi ? -2 : -1);
        if (fh > mi) return 2;
        if (x > hi) return 1;
        if (-fl > mi) return -2;
        return x < lo ? -1 : 0;
    }
    if (lo == hi) return -1;
    return x > hi ? 1 : (x < lo ? -1 : 0);
}

template <typename T, int S, int C>
__global__ __launch_bounds__(LS_THREADS) void ls_system_kernel(LineSearchArgs a, int K, BatchStride bs)
{
    __shared__ LsRed L;
    const int tid = threadIdx.x;
    const size_t sys = blockIdx.x, N = bs.n;
    const int cur = a.it & 1;
    if (a.status) {
        if (a.status[sys] >= 0) return;                                 // frozen before this solve
        const PointTest t = point_test(a.slots + (sys * 2 + cur) * NSL, a.eps_abs, a.eps_rel);
        if (t.ok || !t.finite) return;                                  // the decision freezes the system: no step, alpha stays 0
    }
    const LsSys<T> p{(const T *)a.lo + sys * N, (const T *)a.hi + sys * N, (const T *)a.w + sys * N,
                     a.cap ? (const T *)a.cap + sys * N : nullptr, (const T *)a.xc + sys * N, (const T *)a.xp + sys * N, S};
    double alpha = 1.0;
    if (a.it > 1) {
        const double *part = a.part + sys * (size_t)K * 2;
        double a0 = 0.0, a1 = 0.0, pm = 0.0;
        int none = 0;
        for (int k = tid; k < K; k += LS_THREADS) { a0 += part[2 * k]; a1 += part[2 * k + 1]; }
        block_sum(L, a0, none, tid);
        block_sum(L, a1, none, tid);
        double p0, p1;
        penalty_slope(L, p, N, 0.0, 0.0, 0.0, tid, p0, none);
        penalty_slope(L, p, N, 1.0, 0.0, 0.0, tid, p1, none);
        const double s0 = a0 + p0, s1 = (a0 + a1) + p1;
        if (a.slope && tid == 0) { a.slope[2 * sys] = s0; a.slope[2 * sys + 1] = s1; }
        if (s0 < 0.0 && s1 > 0.0) {                                     // else the full step: no root inside, or no descent
            double bl = 0.0, fl = s0, bh = 1.0, fh = s1;
            for (int j = 0; j < LS_BISECTIONS; ++j) {
                const double mid = 0.5 * (bl + bh);
                int inside;
                penalty_slope(L, p, N, mid, bl, bh, tid, pm, inside);
                if (inside == 0) break;                                 // one linear piece: the secant step is exact
                const double fm = fma(mid, a1, a0) + pm;
                if (fm < 0.0) { bl = mid; fl = fm; }
                else { bh = mid; fh = fm; }
            }
            alpha = bl - fl * (bh - bl) / (fh - fl);
            alpha = alpha < bl ? bl : (alpha > bh ? bh : alpha);
        }
    }
    if (a.alpha && tid == 0) a.alpha[sys * a.alpha_stride] = alpha;
    T *xout = a.xout ? (T *)a.xout + sys * N : nullptr;
    const signed char *act = a.status ? a.act + sys * N : nullptr;
    signed char *act2 = a.status ? a.act2 + sys * N : nullptr;
    int changed = 0;
    for (size_t i = tid; i < N; i += LS_THREADS) {
        const T xc = p.xc[i], xp = p.xp[i];
        const T xn = alpha == 1.0 ? xp : (T)fma(alpha, (double)xp - (double)xc, (double)xc);
        if (xout) xout[i] = xn;
        if (act2) {
            const T w = p.w[i];
            const T mi = p.cap && w > (T)0 ? p.cap[i] : (T)INFINITY;
            const signed char a2 = soft_next_act(xn, p.lo[i], p.hi[i], w, w > (T)0 && __builtin_isfinite(mi), mi, i < (size_t)S);
            act2[i] = a2;
            changed += a2 != act[i];
        }
    }
    if (act2) {
        double none = 0.0;
        block_sum(L, none, changed, tid);
        if (tid == 0) a.round[(sys * 2 + cur) * 2] = changed;           // over the step kernel's count, which read x+
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_ls_scope(const Dims &d, const LineSearchArgs &a, hipStream_t st)
{
    return launch_per_knot("ls_scope", ls_scope_kernel<T, S, C>, d, st, a, d.K, batch_stride(d));
}

template <typename T, int S, int C>
int launch_line_search(const Dims &d, const LineSearchArgs &a, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("line_search: B = %d", d.B); return GATO_EINVAL; }
    if (a.it > 1) {                                                     // the first solve of a call takes the full step
        const int rc = launch_per_knot("line_search", ls_knot_kernel<T, S, C>, d, st, a, d.K, batch_stride(d));
        if (rc) return rc;
    }
    hipLaunchKernelGGL((ls_system_kernel<T, S, C>), dim3(d.B), dim3(LS_THREADS), 0, st, a, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

#define X(S_, C_)                                                                                      \
    template int launch_ls_scope<float, S_, C_>(const Dims &, const LineSearchArgs &, hipStream_t);    \
    template int launch_ls_scope<double, S_, C_>(const Dims &, const LineSearchArgs &, hipStream_t);   \
    template int launch_line_search<float, S_, C_>(const Dims &, const LineSearchArgs &, hipStream_t); \
    template int launch_line_search<double, S_, C_>(const Dims &, const LineSearchArgs &, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
