// Hard bounds of a box QP by the method of multipliers over the line-search iteration (gato_box_qp_alm).
// For x in [lo, hi] the augmented Lagrangian with multiplier mu and weight w is the all-soft problem of section 3.12 on the
// bounds shifted by -mu / w, and the multiplier update mu <- w (x + mu / w - clip(x + mu / w)) is that solve's penalty force y.
// An ALM variable has a finite bound and no user weight and is off the states of x_0; every other variable keeps the caller's
// bound, weight and cap (a user-soft bound stays soft).
//   alm_check_kernel    the parameters, bounds, weights and caps (BAD_BOUNDS), and the inner inputs of the first step
//   alm_update_kernel   after an inner run: v = max dist(x_i, [lo_i, hi_i]) over the ALM variables and |x|_inf into the step's
//                       set of maxima, mu <- y on the ALM variables
//   alm_decide_kernel   one decision per system, read by all its workgroups: accept (the caller's outputs), stop, or the next
//                       weight and the inner bounds and weights of the next step
// Every kernel: one wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i of the knot.  Maxima are
// integer atomicMax on bit patterns of non-negative doubles, the per-system state lives in two sets (step k reads set k % 2 and
// writes the other): no float atomics, and a run repeats bit for bit.
#include "gato_common.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;

template <typename T>
__device__ __forceinline__ bool alm_variable(T lo, T hi, const T *w, size_t v, bool x0)
{
    return !x0 && (__builtin_isfinite(lo) || __builtin_isfinite(hi)) && !(w && w[v] > (T)0);
}

template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void alm_check_kernel(AlmArgs a, int K, int B, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y, o = sys * bs.n;
    const T *lo = (const T *)a.lo + o, *hi = (const T *)a.hi + o;
    const T *w = a.w ? (const T *)a.w + o : nullptr, *cap = a.w && a.cap ? (const T *)a.cap + o : nullptr;
    const T *mu0 = a.mu0 ? (const T *)a.mu0 + o : nullptr;
    T *lo2 = (T *)a.lo2 + o, *hi2 = (T *)a.hi2 + o, *w2 = (T *)a.w2 + o, *mu = (T *)a.mu + o;
    T *cap2 = a.cap2 ? (T *)a.cap2 + o : nullptr;
    if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) a.ctr[0] = B;
    const bool params_ok = __builtin_isfinite(a.alm_weight) && a.alm_weight > 0.0 && a.growth > 1.0 && a.weight_max >= a.alm_weight;
    const T wt = (T)a.alm_weight;
    int bad = !params_ok;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t v = (size_t)k * n + lane;
            const T l = lo[v], h = hi[v], wi = w ? w[v] : (T)0;
            const T mi = cap && wi > (T)0 ? cap[v] : (T)INFINITY;
            if (l != l || h != h || l > h || !(wi >= (T)0) || !__builtin_isfinite(wi) || !(mi >= (T)0)) bad = 1;
            const bool av = alm_variable(l, h, w, v, k == 0 && lane < S);
            const T m = av && mu0 ? mu0[v] : (T)0;
            mu[v] = m;
            lo2[v] = av ? l - m / wt : l;
            hi2[v] = av ? h - m / wt : h;
            w2[v] = av ? wt : wi;
            if (cap2) cap2[v] = av ? (T)INFINITY : mi;
            if (a.act0) a.act[o + v] = a.act0[o + v];
        }
    }
    const int any = __any(bad);
    if (lane == 0 && any) { atomicMax(a.status + sys, GATO_QP_BAD_BOUNDS); atomicAdd(a.ctr + 1, 1); }
    if (blockIdx.x == 0 && lane == 0) {                                 // step 1 reads set 1
        a.state[(sys * 2 + 1) * 2] = a.alm_weight;
        a.state[(sys * 2 + 1) * 2 + 1] = (double)INFINITY;
    }
}

template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void alm_update_kernel(AlmArgs a, int it, int K, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y, o = sys * bs.n;
    const bool frozen = a.status[sys] >= 0;
    if (blockIdx.x == 0 && lane == 0) a.flag[sys] = frozen;
    if (frozen || a.status_i[sys] != GATO_QP_CONVERGED) return;
    const T *lo = (const T *)a.lo + o, *hi = (const T *)a.hi + o, *w = a.w ? (const T *)a.w + o : nullptr;
    const T *xi = (const T *)a.xi + o, *yi = (const T *)a.yi + o;
    T *mu = (T *)a.mu + o;
    unsigned long long mv = 0, mx = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t v = (size_t)k * n + lane;
            const T x = xi[v], l = lo[v], h = hi[v];
            const unsigned long long bx = mag_bits(x);
            mx = bx > mx ? bx : mx;
            if (alm_variable(l, h, w, v, k == 0 && lane < S)) {
                const unsigned long long bv = mag_bits(x - clip(x, l, h));
                mv = bv > mv ? bv : mv;
                mu[v] = yi[v];
            }
        }
    }
    unsigned long long *sl = a.slots + (sys * 2 + (it & 1)) * 2;
    mv = wave_max_bits(mv);
    mx = wave_max_bits(mx);
    if (lane == 0 && mv != 0) atomicMax(sl, mv);
    if (lane == 0 && mx != 0) atomicMax(sl + 1, mx);
}

// The decision of outer step `it` for one system (every workgroup of it reads the same complete maxima and state):
//   the inner run did not converge    its status (MAX_ITERS, NONFINITE); nothing else of the system is written
//   v <= eps_abs + eps_rel |x|_inf    CONVERGED: x, z (clipped on the ALM variables), y, lambda, the act and the residuals
//   the last step                     MAX_ITERS, res_prim = v
// - iters = the solves of all steps, outer = it, weight = the step's, and the system is frozen - otherwise the weight grows where v
// did not fall below a quarter of the step before, and the inner bounds and weights of the next step are written.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void alm_decide_kernel(AlmArgs a, int it, int last, int K, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y, o = sys * bs.n;
    if (a.flag[sys]) return;                                            // frozen before this step
    const int cur = it & 1;
    const unsigned long long *sl = a.slots + (sys * 2 + cur) * 2;
    const double *st = a.state + (sys * 2 + cur) * 2;
    const double v = slot_val(sl, 0), xinf = slot_val(sl, 1), wk = st[0], v_prev = st[1];
    const int inner = a.status_i[sys];
    const bool failed = inner != GATO_QP_CONVERGED;
    const bool ok = !failed && v <= a.eps_abs + a.eps_rel * xinf;
    const bool stop = failed || ok || last;
    const bool grow = !stop && v > 0.25 * v_prev && wk < a.weight_max;
    const double wn = grow ? a.growth * wk : wk;
    if (blockIdx.x == 0 && lane == 0) {
        const int tot = a.tot[sys] + a.iters_i[sys];
        a.tot[sys] = tot;
        if (a.dec) a.dec[sys] = ok ? GATO_ALM_ACCEPT : (failed ? GATO_ALM_INNER : (last ? GATO_ALM_LAST : (grow ? GATO_ALM_GROW : GATO_ALM_KEEP)));
        if (stop) {
            a.status[sys] = ok ? GATO_QP_CONVERGED : (failed ? inner : GATO_QP_MAX_ITERS);
            a.iters[sys] = tot;
            if (a.outer) a.outer[sys] = it;
            if (a.weight) a.weight[sys] = wk;
            if (ok) {
                a.res[2 * sys] = fmax(v, a.res_i[2 * sys]);
                a.res[2 * sys + 1] = a.res_i[2 * sys + 1];
            } else if (!failed) a.res[2 * sys] = v;
            atomicSub(a.ctr, 1);
        } else {
            double *sn = a.state + (sys * 2 + (cur ^ 1)) * 2;
            unsigned long long *ln = a.slots + (sys * 2 + (cur ^ 1)) * 2;
            sn[0] = wn; sn[1] = v;
            ln[0] = 0; ln[1] = 0;
        }
    }
    if (stop && !ok) return;
    const T *lo = (const T *)a.lo + o, *hi = (const T *)a.hi + o, *w = a.w ? (const T *)a.w + o : nullptr;
    if (ok) {
        const T *xi = (const T *)a.xi + o, *zi = (const T *)a.zi + o, *yi = (const T *)a.yi + o, *li = (const T *)a.li + sys * bs.sk;
        T *x = (T *)a.x + o, *z = (T *)a.z + o, *y = (T *)a.y + o, *lam = (T *)a.lam + sys * bs.sk;
        for (int k = blockIdx.x; k < K; k += gridDim.x) {
            if (lane < (k < K - 1 ? n : S)) {
                const size_t j = (size_t)k * n + lane;
                const T xv = xi[j], l = lo[j], h = hi[j];
                x[j] = xv;
                z[j] = alm_variable(l, h, w, j, k == 0 && lane < S) ? clip(xv, l, h) : zi[j];
                y[j] = yi[j];
                if (a.act_out) a.act_out[o + j] = a.act[o + j];
            }
            if (lane < S) lam[(size_t)k * S + lane] = li[(size_t)k * S + lane];
        }
        return;
    }
    const T *mu = (const T *)a.mu + o;
    T *lo2 = (T *)a.lo2 + o, *hi2 = (T *)a.hi2 + o, *w2 = (T *)a.w2 + o;
    const T wt = (T)wn;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t j = (size_t)k * n + lane;
            const T l = lo[j], h = hi[j];
            if (alm_variable(l, h, w, j, k == 0 && lane < S)) {
                const T sh = mu[j] / wt;
                lo2[j] = l - sh;
                hi2[j] = h - sh;
                w2[j] = wt;
            }
        }
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_alm_check(const Dims &d, const AlmArgs &a, hipStream_t st)
{
    return launch_per_knot("alm_check", alm_check_kernel<T, S, C>, d, st, a, d.K, d.B, batch_stride(d));
}

template <typename T, int S, int C>
int launch_alm_update(const Dims &d, const AlmArgs &a, int it, int last, hipStream_t st)
{
    const int rc = launch_per_knot("alm_update", alm_update_kernel<T, S, C>, d, st, a, it, d.K, batch_stride(d));
    return rc ? rc : launch_per_knot("alm_update", alm_decide_kernel<T, S, C>, d, st, a, it, last, d.K, batch_stride(d));
}

#define X(S_, C_)                                                                                     \
    template int launch_alm_check<float, S_, C_>(const Dims &, const AlmArgs &, hipStream_t);         \
    template int launch_alm_check<double, S_, C_>(const Dims &, const AlmArgs &, hipStream_t);        \
    template int launch_alm_update<float, S_, C_>(const Dims &, const AlmArgs &, int, int, hipStream_t);  \
    template int launch_alm_update<double, S_, C_>(const Dims &, const AlmArgs &, int, int, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
