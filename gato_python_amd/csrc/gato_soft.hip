// Soft bounds in the primal-dual active-set iteration (gato_box_qp_pdas_soft).  A variable with a weight
// w_i > 0 is penalised by (w_i / 2) dist(x_i, [lo_i, hi_i])^2 instead of bounded: where it is active it stays in the reduced
// system - the diagonal entry of Q_k or R_k the inversion sees gains w_i, g' gains w_i b_i - and its multiplier is the penalty
// force y_i = w_i (x_i - b_i).  A variable with w_i = 0 is the hard bound of gato_pdas.hip; with no weights every kernel here
// computes what its hard counterpart computes.  The decision of a solve is pdas_decide_kernel as it is (launch_pdas_decide).
// Every kernel: one wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i of the knot.
#include "gato_common.h"
#include "gato_gj.h"
#include "gato_qp_common.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NSL = GATO_POLISH_NSLOT;

// pdas_check_kernel's checks, and a weight that is NaN, negative or +inf marks the system BAD_BOUNDS.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void soft_check_kernel(SoftArgs a, int K, int B, BatchStride bs)
{
    constexpr int n = S + C;
    const PdasArgs &d = a.d;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *lo = (const T *)d.p.lo + sys * bs.n, *hi = (const T *)d.p.hi + sys * bs.n;
    const T *w = a.w ? (const T *)a.w + sys * bs.n : nullptr;
    const signed char *act = d.p.act + sys * bs.n;
    if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) d.ctr[0] = B;
    int bad_b = 0, bad_a = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (lane < (k < K - 1 ? n : S)) {
            const size_t v = (size_t)k * n + lane;
            const T l = lo[v], h = hi[v], wi = w ? w[v] : (T)0;
            const signed char ai = act[v];
            if (l != l || h != h || l > h || !(wi >= (T)0) || !__builtin_isfinite(wi)) bad_b = 1;
            else if (bad_active(ai, bound_of(ai, l, h), k == 0 && lane < S)) bad_a = 1;
        }
    }
    const int any_b = __any(bad_b), any_a = __any(bad_a);
    if (lane == 0) {
        if (any_b) { atomicMax(d.p.status + sys, GATO_QP_BAD_BOUNDS); atomicAdd(d.ctr + 1, 1); }
        if (any_a) { atomicMax(d.p.status + sys, GATO_QP_BAD_ACTIVE); atomicAdd(d.ctr + 2, 1); }
    }
}

// polish_prepare_kernel's pass with the hard-active set in place of the active set: a soft-active variable keeps its row and
// column, the diagonal entry the Gauss-Jordan sees gains w_i, g'_i gains w_i b_i (before the hard shift of its row), and c' does
// not see it.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void soft_prepare_kernel(SoftArgs s, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SN = S * n;
    __shared__ T sb[2][n];                   // bound values of knots k-1 (0) and k (1), 0 off the hard-active set
    __shared__ int sa[2][n];                 // hard-active
    __shared__ T sw[n], ss[n];               // knot k: w_i on the soft-active set (0 elsewhere) and the bound there
    const PolishArgs &a = s.d.p;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *Gd = (const T *)a.Gd + sys * bs.g, *Cd = (const T *)a.Cd + sys * bs.c;
    const T *g = (const T *)a.g + sys * bs.n, *c = (const T *)a.c + sys * bs.sk;
    const T *lo = (const T *)a.lo + sys * bs.n, *hi = (const T *)a.hi + sys * bs.n;
    const T *w = s.w ? (const T *)s.w + sys * bs.n : nullptr;
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
                T b = (T)0, wi = (T)0, bsoft = (T)0;
                if (kk >= 0 && lane < (kk < K - 1 ? n : S)) {
                    const size_t v = (size_t)kk * n + lane;
                    const signed char ai = act[v];
                    b = bound_of(ai, lo[v], hi[v]);
                    if (h == 1 && bad_active(ai, b, kk == 0 && lane < S)) bad = 1;
                    if (soft_active(ai, w, v)) {
                        wi = w[v];
                        bsoft = b;
                        b = (T)0;
                    } else on = ai != 0;
                }
                sa[h][lane] = on;
                sb[h][lane] = b;
                if (h == 1) { sw[lane] = wi; ss[lane] = bsoft; }
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
                        if (lane == r && sw[lane] > (T)0) e += sw[lane];
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
                        if (lane == r && sw[S + lane] > (T)0) e += sw[S + lane];
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
                if (sw[lane] > (T)0) t = fmaT(sw[lane], ss[lane], t);
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

// Solve `it`: the point of the reduced solve and its maxima (soft_point_knot), and in the same pass act' from the point.  A hard
// variable follows pdas_step_kernel's rule; a soft one is decided from x alone, whatever its act was:
//   0 on the states of x_0, -1 where lo == hi, +1 where x > hi, -1 where x < lo, 0 otherwise
// - exact comparisons.  A system frozen before this solve is only marked.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void soft_step_kernel(SoftArgs s, int it, int K, BatchStride bs)
{
    constexpr int n = S + C;
    __shared__ PointLds<T, S, C> lds;
    const PdasArgs &a = s.d;
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const int cur = it & 1;
    int *rn = a.round + (sys * 2 + cur) * 2;
    if (a.p.status[sys] >= 0) {
        if (blockIdx.x == 0 && lane == 0) rn[1] = 1;
        return;
    }
    const PointSys<T> p = point_sys<T>(a.p, sys, bs);
    const T *w = s.w ? (const T *)s.w + sys * bs.n : nullptr;
    signed char *act2 = a.act2 + sys * bs.n;
    unsigned long long m[NSL];
#pragma unroll
    for (int f = 0; f < NSL; ++f) m[f] = 0;
    int changed = 0;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const PointVar<T> v = soft_point_knot<T, S, C>(lds, p, w, k, K, lane, m);
        if (v.on) {
            const size_t j = (size_t)k * n + lane;
            const bool soft = w && w[j] > (T)0;
            signed char a2;
            if (k == 0 && lane < S) a2 = 0;
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

// lo_bar, hi_bar and w_bar of a converged point from the adjoint [a; beta] of its last assembly.  Hard-active i: b_bar_i = xbar_i -
// (H a + C^T beta)_i, qp_bound_grad_kernel's row products; soft-active i: b_bar_i = w_i a_i and w_bar_i = a_i (b_i - x_i); b_bar
// goes to hi_bar where act = +1 and to lo_bar where act = -1; every other entry of the three is 0.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void soft_grad_kernel(SoftGradArgs q, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SN = S * n;
    __shared__ T sQ[SS], sR[CC], sCk[SN], sV[n], sLk[S], sLn[S];
    const int lane = threadIdx.x;
    const size_t sys = blockIdx.y;
    const T *G = (const T *)q.G + sys * bs.g, *Cd = (const T *)q.Cd + sys * bs.c;
    const signed char *act = q.act + sys * bs.n;
    const T *w = q.w ? (const T *)q.w + sys * bs.n : nullptr;
    const T *lo = (const T *)q.lo + sys * bs.n, *hi = (const T *)q.hi + sys * bs.n, *x = (const T *)q.x + sys * bs.n;
    const T *xbar = (const T *)q.xbar + sys * bs.n, *adz = (const T *)q.adz + sys * bs.n, *beta = (const T *)q.beta + sys * bs.sk;
    T *lo_bar = (T *)q.lo_bar + sys * bs.n, *hi_bar = (T *)q.hi_bar + sys * bs.n, *w_bar = (T *)q.w_bar + sys * bs.n;
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
            T bb = (T)0, wb = (T)0;
            if (soft_active(ai, w, v)) {
                const T ad = sV[lane];
                bb = w[v] * ad;
                wb = ad * (bound_of(ai, lo[v], hi[v]) - x[v]);
            } else if (ai != 0) {
                T hx, ctl;
                row_products<T, S, C>(lane, k < K - 1, sQ, sR, sCk, sV, sLk, sLn, (T)0, hx, ctl);
                bb = xbar[v] - (hx + ctl);
            }
            lo_bar[v] = ai < 0 ? bb : (T)0;
            hi_bar[v] = ai > 0 ? bb : (T)0;
            w_bar[v] = wb;
        }
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_soft_check(const Dims &d, const SoftArgs &a, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("soft_check: B = %d", d.B); return GATO_EINVAL; }
    hipLaunchKernelGGL((soft_check_kernel<T, S, C>), dim3(knot_grid(d.K), d.B), dim3(WAVE), 0, st, a, d.K, d.B, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

template <typename T, int S, int C>
int launch_soft_prepare(const Dims &d, const SoftArgs &a, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("soft_prepare: B = %d", d.B); return GATO_EINVAL; }
    hipLaunchKernelGGL((soft_prepare_kernel<T, S, C>), dim3(knot_grid(d.K), d.B), dim3(WAVE), 0, st, a, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

template <typename T, int S, int C>
int launch_soft_step(const Dims &d, const SoftArgs &a, int it, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("soft_step: B = %d", d.B); return GATO_EINVAL; }
    hipLaunchKernelGGL((soft_step_kernel<T, S, C>), dim3(knot_grid(d.K), d.B), dim3(WAVE), 0, st, a, it, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

template <typename T, int S, int C>
int launch_soft_grad(const Dims &d, const SoftGradArgs &a, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("soft_grad: B = %d", d.B); return GATO_EINVAL; }
    hipLaunchKernelGGL((soft_grad_kernel<T, S, C>), dim3(knot_grid(d.K), d.B), dim3(WAVE), 0, st, a, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

#define X(S_, C_)                                                                                        \
    template int launch_soft_check<float, S_, C_>(const Dims &, const SoftArgs &, hipStream_t);          \
    template int launch_soft_check<double, S_, C_>(const Dims &, const SoftArgs &, hipStream_t);         \
    template int launch_soft_prepare<float, S_, C_>(const Dims &, const SoftArgs &, hipStream_t);        \
    template int launch_soft_prepare<double, S_, C_>(const Dims &, const SoftArgs &, hipStream_t);       \
    template int launch_soft_step<float, S_, C_>(const Dims &, const SoftArgs &, int, hipStream_t);      \
    template int launch_soft_step<double, S_, C_>(const Dims &, const SoftArgs &, int, hipStream_t);     \
    template int launch_soft_grad<float, S_, C_>(const Dims &, const SoftGradArgs &, hipStream_t);       \
    template int launch_soft_grad<double, S_, C_>(const Dims &, const SoftGradArgs &, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
