// Primal-dual active-set iteration for box QPs over the polish path (gato_box_qp_pdas).
// Every iteration is the reduced solve of the polish on the current act (add_rho, polish_prepare_kernel, the whole solve with
// the given inverses), then pdas_step_kernel - the polished point, its residuals and the next active set act' - and
// pdas_decide_kernel, which accepts the point, freezes the system or moves act' into act.  The per-system maxima and the count
// of changed entries live in two sets, set it % 2 for solve it: the decision of solve it clears the set solve it + 1 folds into.
// Every kernel: one wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i of the knot.
#include "gato_common.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NSL = GATO_POLISH_NSLOT;

// The first launch of a call: a NaN bound, lo > hi or a weight that is NaN, negative or +inf marks the system BAD_BOUNDS, a start
// act the reduced system cannot take (polish_prepare_kernel's rule) BAD_ACTIVE; ctr = {B live systems, waves that saw a bad bound
// or weight, waves that saw a bad act}.  With caps (W = BOUNDS_CAPPED): a cap that is NaN or negative, read only where the weight
// is positive, is BAD_BOUNDS too, and a start act of +-2 is taken where bad_active_capped allows it.
template <typename T, int S, int C, int W>
__global__ __launch_bounds__(WAVE) void pdas_check_kernel(PdasArgs a, int K, int B, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *lo = (const T *)a.p.lo + sys * bs.n, *hi = (const T *)a.p.hi + sys * bs.n;
    const T *w = sys_weights<T, W>(a.p.w, sys, bs);
    const T *cap = sys_caps<T, W>(a.p.cap, sys, bs);
    const signed char *act = a.p.act + sys * bs.n;
    if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) a.ctr[0] = B;
    int bad_b = 0, bad_a = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t v = (size_t)k * n + lane;
            const T l = lo[v], h = hi[v], wi = w ? w[v] : (T)0;
            const signed char ai = act[v];
            if (l != l || h != h || l > h || !(wi >= (T)0) || !__builtin_isfinite(wi)) bad_b = 1;
            else if constexpr (W == BOUNDS_CAPPED) {
                const T mi = cap && wi > (T)0 ? cap[v] : (T)INFINITY;
                if (!(mi >= (T)0)) bad_b = 1;
                else if (bad_active_capped(ai, bound_of(ai, l, h), k == 0 && lane < S, wi, mi)) bad_a = 1;
            }
            else if (bad_active(ai, bound_of(ai, l, h), k == 0 && lane < S)) bad_a = 1;
        }
    }
    const int any_b = __any(bad_b), any_a = __any(bad_a);
    if (lane == 0) {
        if (any_b) { atomicMax(a.p.status + sys, GATO_QP_BAD_BOUNDS); atomicAdd(a.ctr + 1, 1); }
        if (any_a) { atomicMax(a.p.status + sys, GATO_QP_BAD_ACTIVE); atomicAdd(a.ctr + 2, 1); }
    }
}

// Solve `it`: the polished point of the reduced solve and its eleven maxima (polished_point_knot, the polish's own pass), and
// in the same pass act' from the point:
//   0 on the states of x_0, -1 where lo == hi;  free: +1 where x > hi, -1 where x < lo;  active upper: kept while y > 0;
//   active lower: kept while y < 0;  0 otherwise
// - exact comparisons: near-ties are the acceptance test's, which runs first - and the count of entries where act' differs
// from act (an integer atomicAdd per wave that saw a change).  A soft variable (weight > 0) takes the rule of a free one, from x
// alone, whatever its act was.  A soft variable with a finite cap m (W = BOUNDS_CAPPED) is saturated, +-2,
// where the product w (x - b) passes the cap: +2 where w (x - hi) > m, else +1 where x > hi; -2 where -(w (x - lo)) > m, else -1 where
// x < lo; lo == hi: +2, -2 by the same products, else -1.  A system frozen before this solve is only marked.
template <typename T, int S, int C, int W>
__global__ __launch_bounds__(WAVE) void pdas_step_kernel(PdasArgs a, int it, int K, BatchStride bs)
{
    constexpr int n = S + C;
    __shared__ PointLds<T, S, C> lds;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const int cur = it & 1;
    int *rn = a.round + (sys * 2 + cur) * 2;
    if (a.p.status[sys] >= 0) {
        if (blockIdx.x == 0 && lane == 0) rn[1] = 1;
        return;
    }
    const PointSys<T> p = point_sys<T, W>(a.p, sys, bs);
    signed char *act2 = a.act2 + sys * bs.n;
    unsigned long long m[NSL];
#pragma unroll
    for (int f = 0; f < NSL; ++f) m[f] = 0;
    int changed = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const PointVar<T> v = polished_point_knot<T, S, C>(lds, p, k, K, lane, m);
        if (v.on) {
            const size_t j = (size_t)k * n + lane;
            const bool soft = p.w && p.w[j] > (T)0;
            signed char a2;
            bool capped = false;
            T mi = (T)0;
            if constexpr (W == BOUNDS_CAPPED) {
                if (soft && p.cap) {
                    mi = p.cap[j];
                    capped = __builtin_isfinite(mi);
                }
            }
            if (k == 0 && lane < S) a2 = 0;
            else if (capped) {
                const T fh = p.w[j] * (v.x - v.hi), fl = p.w[j] * (v.x - v.lo);
                if (v.lo == v.hi) a2 = fh > mi ? 2 : (-fh > mi ? -2 : -1);
                else if (fh > mi) a2 = 2;
                else if (v.x > v.hi) a2 = 1;
                else if (-fl > mi) a2 = -2;
                else a2 = v.x < v.lo ? -1 : 0;
            }
            else if (v.lo == v.hi) a2 = -1;
            else if (v.act == 0 || soft) a2 = v.x > v.hi ? 1 : (v.x < v.lo ? -1 : 0);
            else if (v.act > 0) a2 = v.y > (T)0 ? 1 : 0;
            else a2 = v.y < (T)0 ? -1 : 0;
            act2[j] = a2;
            changed += a2 != v.act;
        }
    }
    fold_into_slots(m, a.p.slots + (sys * 2 + cur) * NSL, lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
    if (lane == 0 && changed > 0) atomicAdd(rn, changed);
}

// The decision of solve `it` for one system (every workgroup of it reads the same complete maxima and change count):
//   the acceptance test passes   the point over the caller's x, z, y, lambda; CONVERGED, the residuals
//   a maximum is not finite      NONFINITE
//   act' == act, or the last     MAX_ITERS (the next solve would repeat this one)
// - iters = it and the system is frozen: nothing of it is written again - otherwise act' moves into act and the other set
// of maxima and counts is cleared for solve it + 1.  The knot-0 workgroup records the decision and keeps the live count.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void pdas_decide_kernel(PdasArgs a, int it, int last, int K, BatchStride bs)
{
    constexpr int n = S + C;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const int cur = it & 1;
    const int *rn = a.round + (sys * 2 + cur) * 2;
    if (rn[1]) return;                                                      // frozen before this solve
    const PointTest t = point_test(a.p.slots + (sys * 2 + cur) * NSL, a.p.eps_abs, a.p.eps_rel);
    const bool stop = t.ok || !t.finite || rn[0] == 0 || last;
    if (blockIdx.x == 0) {
        if (stop) {
            if (lane == 0) {
                a.p.status[sys] = t.ok ? GATO_QP_CONVERGED : (t.finite ? GATO_QP_MAX_ITERS : GATO_QP_NONFINITE);
                a.iters[sys] = it;
                if (t.ok) {
                    a.p.res[2 * sys] = t.rp;
                    a.p.res[2 * sys + 1] = t.rd;
                }
                atomicSub(a.ctr, 1);
            }
        } else {
            if (lane < NSL) a.p.slots[(sys * 2 + (cur ^ 1)) * NSL + lane] = 0;
            if (lane < 2) a.round[(sys * 2 + (cur ^ 1)) * 2 + lane] = 0;
        }
    }
    if (t.ok) write_point<T, S, C>(a.p, sys, bs, K, lane);
    else if (!stop) {
        signed char *act = a.act + sys * bs.n;
        const signed char *act2 = a.act2 + sys * bs.n;
        for (int k = blockIdx.x; k < K; k += gridDim.x) {
            if (lane < (k < K - 1 ? n : S)) {
                const size_t v = (size_t)k * n + lane;
                act[v] = act2[v];
            }
        }
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_pdas_check(const Dims &d, const PdasArgs &a, hipStream_t st)
{
    return launch_per_knot("pdas_check", GATO_BOUNDS_KERNEL(pdas_check_kernel, bounds_form(a.p.w, a.p.cap)), d, st, a, d.K, d.B,
                           batch_stride(d));
}

template <typename T, int S, int C>
int launch_pdas_step(const Dims &d, const PdasArgs &a, int it, hipStream_t st)
{
    return launch_per_knot("pdas_step", GATO_BOUNDS_KERNEL(pdas_step_kernel, bounds_form(a.p.w, a.p.cap)), d, st, a, it, d.K,
                           batch_stride(d));
}

template <typename T, int S, int C>
int launch_pdas_decide(const Dims &d, const PdasArgs &a, int it, int last, hipStream_t st)
{
    return launch_per_knot("pdas_decide", pdas_decide_kernel<T, S, C>, d, st, a, it, last, d.K, batch_stride(d));
}

#define X(S_, C_)                                                                                        \
    template int launch_pdas_decide<float, S_, C_>(const Dims &, const PdasArgs &, int, int, hipStream_t);  \
    template int launch_pdas_decide<double, S_, C_>(const Dims &, const PdasArgs &, int, int, hipStream_t); \
    template int launch_pdas_check<float, S_, C_>(const Dims &, const PdasArgs &, hipStream_t);         \
    template int launch_pdas_check<double, S_, C_>(const Dims &, const PdasArgs &, hipStream_t);        \
    template int launch_pdas_step<float, S_, C_>(const Dims &, const PdasArgs &, int, hipStream_t);     \
    template int launch_pdas_step<double, S_, C_>(const Dims &, const PdasArgs &, int, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
