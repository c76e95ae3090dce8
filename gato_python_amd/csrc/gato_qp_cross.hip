// The ADMM update of a box QP whose stage cost has a state-control cross term (gato_box_qp_solve_cross):
//   min 1/2 x^T H x - g^T x   s.t.  C x = c,  lo <= x <= hi,   H = G + rho_reg I,   G_k = [[Q_k, M_k], [M_k^T, R_k]].
// The x-step matrix [[H + sigma I + diag(rho_i), C^T], [C, 0]] is assembled once in the variables (x, v), u_k = v_k - W_k x_k, of
// section 3.15 (W_k = (R_k + sigma + diag(rho_i) + rho_reg I)^-1 M_k^T); the projection onto the box, the multipliers and the
// residuals stay in (x, u), so a box on u stays a box.  qp_update_cross_kernel is qp_update_kernel (gato_qp.hip) with the two maps
// of an iteration fused in: it reads the x-step's solution in (x, v) and maps it back as cross_finish_kernel does, and writes the
// next right-hand side already transformed as cross_rhs_kernel does.  An iteration stays at two launches: the re-solve and this.
// One wave per knot, grid.x strides over the knots, grid.y = system, lane i = variable i, operands staged in LDS.  Every output
// element has one writer and one chain of fused multiply-adds over the ascending inner index; the only atomics are the integer
// atomicMax on the bit patterns of the maxima and the atomicSub of the live count, as in qp_update_kernel.
#include "gato_cross_device.h"

namespace gato {
namespace {

constexpr int WAVE = 64;
constexpr int NSL = GATO_QP_NSLOT;
// slot fields, as gato_qp.hip's: qp_prepare_kernel writes slot 2 and the freeze test of either update kernel reads them
enum { F_PRIM, F_DUAL, F_X, F_Z, F_C, F_HX, F_CTL, F_Y, F_G, F_GT };

// Iteration `it`.  The freeze test on the maxima of slot (it-1) % 3, the zero right-hand side rule, x+, z+, y+, lambda+, the PCG
// totals and the slot rotation are qp_update_kernel's, statement for statement.  What differs, per knot k:
//   x~ = (x~'_x, x~'_v - W_k x~'_x) of knots k and k-1 (x~' itself is not rewritten; launch 0 reads the whole solve's output);
//   (H x)_i gains sum_c M_k[i, c] u_c on a state row and sum_s M_k[s, j] x_s on control row j, after the row's own chain;
//   g~+ = g + sigma x+ + rho z+ - y+ goes to gt as g~'_x = g~+_x - W_k^T g~+_u, g~'_u = g~+_u (the last knot has no W), and F_GT
//   folds g~': what the PCG will read (g~ and g~' vanish together).
// With M = 0 (W = 0) every added term is a fused multiply-add of a zero product: the values are qp_update_kernel's.
template <typename T, int S, int C>
__global__ __launch_bounds__(WAVE) void qp_update_cross_kernel(QpCrossArgs ca, int it, int last, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SC = S * C, SN = S * n;
    __shared__ T sQ[SS], sR[CC], sM[SC], sWk[SC], sWp[SC], sCp[SN], sCk[SN];
    __shared__ T sTk[n], sTp[n], sXn[n], sXp[n], sGt[n], sLk[S], sLn[S];
    const QpArgs &a = ca.q;
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
    const size_t ms = (size_t)(K - 1) * SC;
    const T *G = (const T *)a.G + sys * bs.g, *Cd = (const T *)a.Cd + sys * bs.c;
    const T *M = (const T *)ca.M + sys * ms, *W = (const T *)ca.W + sys * ms;
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
        const bool full = k < K - 1;
        const int nk = full ? n : S;
        const size_t v0 = (size_t)k * n;
        __syncthreads();                                                     // the previous knot's readers are done
        const T *Gk = G + (size_t)k * (SS + CC);
        for (int e = lane; e < SS; e += WAVE) sQ[e] = Gk[e];
        if (full) {
            for (int e = lane; e < CC; e += WAVE) sR[e] = Gk[SS + e];
            for (int e = lane; e < SC; e += WAVE) { sM[e] = M[(size_t)k * SC + e]; sWk[e] = W[(size_t)k * SC + e]; }
            for (int e = lane; e < SN; e += WAVE) sCk[e] = Cd[(size_t)k * SN + e];
        }
        if (k > 0) {
            for (int e = lane; e < SC; e += WAVE) sWp[e] = W[(size_t)(k - 1) * SC + e];
            for (int e = lane; e < SN; e += WAVE) sCp[e] = Cd[(size_t)(k - 1) * SN + e];
        }
        if (lane < nk) sTk[lane] = zero_rhs ? (T)0 : xt[v0 + lane];          // x~' of knot k and of knot k-1 (always a full knot)
        if (k > 0 && lane < n) sTp[lane] = zero_rhs ? (T)0 : xt[v0 - n + lane];
        if (lane < S) {
            sLk[lane] = zero_rhs ? (T)0 : lt[(size_t)k * S + lane];
            if (full) sLn[lane] = zero_rhs ? (T)0 : lt[(size_t)(k + 1) * S + lane];
        }
        __syncthreads();
        T xn = 0, zn = 0, yn = 0, gv = 0, t = 0;
        if (lane < nk) {
            const size_t v = v0 + lane;
            T xs = sTk[lane];
            if (lane >= S) xs = cross_unfold_u<T, S, C>(sWk, sTk, xs, lane - S);    // u~ = v~ - W_k x~
            const T xh = fmaT(alpha, xs, beta * z[v]);
            xn = fmaT(alpha, xs, beta * xr[v]);
            const T r = rho[v];
            if (r == (T)0) { zn = xh; yn = (T)0; }
            else {
                const T yv = y[v];
                zn = clip(xh + yv / r, lo[v], hi[v]);
                yn = fmaT(r, xh - zn, yv);
            }
            gv = g[v];
            t = fmaT(sigma, xn, gv);
            t = fmaT(r, zn, t) - yn;
            sXn[lane] = xn;
            sGt[lane] = t;
        }
        if (k > 0 && lane < n) {                                            // knot k-1's x+
            const size_t v = v0 - n + lane;
            T xs = sTp[lane];
            if (lane >= S) xs = cross_unfold_u<T, S, C>(sWp, sTp, xs, lane - S);
            sXp[lane] = fmaT(alpha, xs, beta * xr[v]);
        }
        __syncthreads();
        if (lane < nk) {
            const int i = lane;
            const size_t v = v0 + i;
            T hx = (T)0, ctl = (T)0;
            if (i < S) {
#pragma unroll 4
                for (int cc = 0; cc < S; ++cc) hx = fmaT(sQ[i + cc * S], sXn[cc], hx);
                if (full) {
#pragma unroll 4
                    for (int cc = 0; cc < C; ++cc) hx = fmaT(sM[i + cc * S], sXn[S + cc], hx);
                }
                ctl = sLk[i];
            } else {
#pragma unroll 4
                for (int cc = 0; cc < C; ++cc) hx = fmaT(sR[(i - S) + cc * C], sXn[S + cc], hx);
#pragma unroll 4
                for (int s = 0; s < S; ++s) hx = fmaT(sM[s + (i - S) * S], sXn[s], hx);
            }
            hx = fmaT(rreg, xn, hx);
            if (full) {
#pragma unroll 4
                for (int r = 0; r < S; ++r) ctl = fmaT(sCk[r + i * S], sLn[r], ctl);
            }
            const T rd = (hx - gv) + ctl + yn;
            if (full && i < S) t = cross_fold_g<T, S, C>(sWk, sGt + S, t, i);      // g~'_x = g~+_x - W_k^T g~+_u
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

template <typename T, int S, int C>
int launch_update(const Dims &d, const QpCrossArgs &a, int it, int last, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("qp_update_cross: B = %d", d.B); return GATO_EINVAL; }
    if (d.K < 2) { set_error("qp_update_cross: K = %d has no cross term", d.K); return GATO_EINVAL; }
    const int gx = last ? 1 : knot_grid(d.K);                             // the test alone: one workgroup per system
    hipLaunchKernelGGL((qp_update_cross_kernel<T, S, C>), dim3(gx, d.B), dim3(WAVE), 0, st, a, it, last, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

}  // namespace
}  // namespace gato

int qp_update_cross(const Dims &d, int dtype, const QpCrossArgs &a, int it, int last, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_update<T, S_, C_>(d, a, it, last, st)
    GATO_CROSS_DISPATCH("qp_update_cross");
#undef GATO_CROSS_LAUNCH
}
