// The one-workgroup kernels of the resident PCG with two rows per lane - pcg_single_f32x2_kernel (fp32) and the headline
// pcg_single_f64m_kernel (fp64, mixed rows) -, the helper blocks of their one-system launches (L2 warm-up, dz) and their
// launcher.  launch_pcg_resident (gato_pcg_resident.hip) sends the launches with option pair here.
#include "gato_pcg_geometry.h"
#include "gato_pcg_launch.h"

namespace gato {
namespace {

// Helper blocks of the ONE-SYSTEM launches of the one-workgroup kernels (gridDim = 1 + 8 x helpers; block 0 solves).  Called by
// every block but block 0; `scratch`: LDS, (4 S^2 + 6 S) values per wave of the block.
template <typename T, int S>
__device__ __forceinline__ void one_system_helper(const PcgLaunch &a, T *scratch)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x, nwv = nt >> 6, K = a.K;
    if ((blockIdx.x & 7) != 0) return;
    const size_t h = (blockIdx.x >> 3) - 1, nh = (gridDim.x - 1) >> 3;
    const size_t bytes = a.imgS ? (size_t)3 * S * a.img_ld * sizeof(T) : (size_t)3 * S * S * K * sizeof(T);   // of each array the solver loads from
    const size_t lines = (bytes + 127) / 128;
    typedef int I4 __attribute__((ext_vector_type(4)));
    const I4 *s4 = static_cast<const I4 *>(a.imgS ? a.imgS : a.S_bd), *p4 = static_cast<const I4 *>(a.imgS ? a.imgP : a.P_bd);
    const size_t last16 = bytes / 16 - 1;                                     // last whole 16-byte unit of an array
    I4 acc = {0, 0, 0, 0};
    for (size_t l = h * nt + tid; l < lines; l += nh * nt) {
        const size_t u = l * 8 < last16 ? l * 8 : last16;
        acc ^= s4[u] ^ p4[u];
    }
    asm volatile("" ::"v"(acc));
    // ... and then stay for the dz back-substitution (compute_dz, gato_schur.cuh:758-867): wave w of helper h takes knot
    // h * WT + w, brings Q_k^-1, R_k^-1, A_k, B_k and g_k into LDS while the solve runs, waits (sleeping) until the solving
    // workgroup has stored launch_id in *dz_flag - lambda is complete and written through - and finishes in about a microsecond.
    // That replaces a launch of its own (5.3 us + the gap in front of it) at the end of every step.  Formulas and
    // accumulation order of dz_kernel (gato_assembly.hip), row by row: the same bits.  The solving workgroup never waits for
    // a helper, so helpers that are scheduled late (or after it has finished) just find the flag set.
    if (a.dz_helpers && a.dz != nullptr) {
        const int kq = (int)h * nwv + wave;
        if (kq >= K) return;
        const int Cn = a.C, n = S + Cn, SS = S * S;
        const size_t gs = (size_t)(SS + Cn * Cn), cs = (size_t)(SS + S * Cn);
        const T *__restrict__ Qg = static_cast<const T *>(a.dz_Ginv) + (size_t)kq * gs;
        const T *__restrict__ Ag = static_cast<const T *>(a.dz_Cd) + (size_t)kq * cs;
        const T *__restrict__ gg = static_cast<const T *>(a.dz_g) + (size_t)kq * n;
        const T *__restrict__ lg = static_cast<const T *>(a.lambda) + (size_t)kq * S;
        T *__restrict__ dzo = static_cast<T *>(a.dz) + (size_t)kq * n;
        const bool last = kq == K - 1;
        T *scr = scratch + (size_t)wave * (4 * SS + 6 * S);                                   // this wave's own part of the LDS
        T *sQi = scr, *sA = sQi + SS, *sRi = sA + SS, *sB = sRi + SS, *sl = sB + SS, *st = sl + 2 * S, *sg = st + 2 * S;
        for (int i = lane; i < SS; i += 64) sQi[i] = Qg[i];
        for (int i = lane; i < (last ? S : n); i += 64) sg[i] = gg[i];
        if (!last) {
            for (int i = lane; i < Cn * Cn; i += 64) sRi[i] = Qg[SS + i];
            for (int i = lane; i < SS; i += 64) sA[i] = Ag[i];
            for (int i = lane; i < S * Cn; i += 64) sB[i] = Ag[SS + i];
        }
        gi32 *flag = (gi32 *)a.dz_flag;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        // the solve itself may legitimately take longer than the hand-off time-out (max_iters is the caller's): the helpers allow
        // it 50 us per iteration on top (25 x what an iteration takes) before they call the solving workgroup dead
        const unsigned long long patience = a.timeout_ticks + (unsigned long long)(a.max_iters > 0 ? a.max_iters : 0) * 5000ull;
        bool late = false;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != a.launch_id) {
            __builtin_amdgcn_s_sleep(4);                      // ~0.1 us between looks: 50 waves, one load each
            if (__builtin_amdgcn_s_memrealtime() - t0 > patience) { late = true; break; }
        }
        if (late) {         // cannot happen unless the solving workgroup died: report it like a hand-off time-out (the solving
            // workgroup, should it still arrive, reads the status word and marks the solve incomplete: iters = -1)
            if (lane == 0) __hip_atomic_store((gi32 *)a.status, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        // No agent-scope acquire (buffer_inv: 2.4 us of this wave's 4.2): lambda is all this wave reads of what the launch wrote,
        // through agent-scope loads - past this CU's L1 - of bytes the solving workgroup stored write-through and drained in
        // front of its flag store.  The wavefront-scope fence is no instruction; it keeps the loads below the poll.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < (last ? S : 2 * S); i += 64) sl[i] = __hip_atomic_load(lg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wave_lds_fence();
        if (!last) {
            for (int i = lane; i < S; i += 64) {                                  // A_k^T lambda_{k+1}   :833-838
                T res = (T)0;
#pragma unroll
                for (int t = 0; t < S; ++t) res = gato::fmaT(sA[i * S + t], sl[S + t], res);
                st[i] = res;
            }
            for (int i = lane; i < Cn; i += 64) {                                 // B_k^T lambda_{k+1}   :784-789
                T res = (T)0;
#pragma unroll
                for (int t = 0; t < S; ++t) res = gato::fmaT(sB[i * S + t], sl[S + t], res);
                st[S + i] = res;
            }
            wave_lds_fence();
            for (int i = lane; i < S; i += 64) st[i] = sg[i] - (sl[i] + st[i]);                    // :841-852
            for (int i = lane; i < Cn; i += 64) st[S + i] = sg[S + i] - st[S + i];                 // :792-796
        } else {
            for (int i = lane; i < S; i += 64) st[i] = sg[i] - sl[i];             // last state row (D2)
        }
        wave_lds_fence();
        for (int r = lane; r < S; r += 64) {                                      // Q_k^-1 (...)         :856-865
            T res = (T)0;
#pragma unroll
            for (int cc = 0; cc < S; ++cc) res = gato::fmaT(sQi[r + cc * S], st[cc], res);
            dzo[r] = res;
        }
        if (!last) {
            for (int r = lane; r < Cn; r += 64) {                                 // R_k^-1 (...)         :799-808
                T res = (T)0;
                for (int cc = 0; cc < Cn; ++cc) res = gato::fmaT(sRi[r + cc * Cn], st[S + cc], res);
                dzo[S + r] = res;
            }
        }
    }
}

// Independent accumulation chains per row of the fp32 two-rows-per-lane kernel's products.  One chain of 3S dependent packed
// FMAs (the reference's left-to-right order, GATO_PAIR_CHAINS = 1) is latency: a SIMD that hosts one wave of the launch idles
// between them and the compiler pads every one with a wait state.  2 = even columns + odd columns (the order of
// row_times_window's packed form, which every other fp32 kernel of the family runs): 14/7/50 f32 1.365 -> 1.256 us per
// iteration (same box; 3 chains 1.27, 4 chains 1.29; S even: a column's parity is its parity inside the 16-byte read).  fp32 parity is measured against the fp64 oracle beside the reference
// order's own error (tests/f32_parity.py); fp64 keeps the reference's order everywhere.
#ifndef GATO_PAIR_CHAINS
#define GATO_PAIR_CHAINS 2
#endif
#if GATO_PAIR_CHAINS != 1 && GATO_PAIR_CHAINS != 2
#error "GATO_PAIR_CHAINS: 1 (the reference's left-to-right order) or 2 (even + odd columns)"
#endif
// ---- fp32, one workgroup (or one workgroup per system of a batch), TWO rows per lane --------------------------
// The single-workgroup loop is instruction-issue bound: with two rows of the same knot per lane
// the operand-window reads are shared by both rows, the FMAs pair up as v_pk_fma_f32 and the wave count halves
// (IIWA 14/7/50: 6 waves instead of 11), and the one-CU regime extends to K*S <= 2*MAXT rows.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// WAVE-PRIVATE operand windows (round 3; the shared-window form it replaced - option shared_windows - was removed in round 5).  In a shared-window form an iteration has four
// barriers: two inside the block sums and two between a vector update and the product that reads the updated window (every
// lane must have stored its entries of r / p before any lane reads its neighbours').  Here every wave keeps its OWN copy of
// the part of the r and p windows its lanes read - its own 128 rows plus a halo of up to 2S - 1 rows on either side - and
// advances the halo rows itself: up to 4S - 2 lanes of the wave hold one halo row of r and p in a register, fetch that row's
// entry of upsilon (of r~) from a shared exchange window which the owners fill BEFORE the block sum's barrier, and apply the
// owner's own FMA (r - alpha upsilon, r~ + beta p: the same bits, tools/pw_check.py and test_private_windows_*).  A wave then
// reads only LDS words it wrote itself (LDS operations of one wave execute in order: no barrier, no wait), so the two window
// barriers and the LDS write latency in front of them are gone: two barriers per iteration.  14/7/50 fp32: 1.405 -> 1.340 us
// per iteration (with 14 spilled VGPRs).  The fp64 mixed-rows kernel gains nothing from it (its loop is bound by the LDS read
// queue, not by barriers: measured 1.945 us with two barriers and no halo update at all against 1.94) and keeps shared windows.
template <int S, int MAXT>
__global__ __launch_bounds__(MAXT) void pcg_single_f32x2_kernel(PcgLaunch a)
{
    constexpr int H = S / 2;                       // lanes per knot
    constexpr int SP = pad_to(S, 4);
    constexpr int MAXK = (MAXT + H - 1) / H;
    static_assert(S % 2 == 0, "two rows per lane need an even STATE_SIZE");
    __shared__ __attribute__((aligned(16))) float xs[2][(MAXK + 2) * SP];
    // (partials_total_all8 reads the four row sums of EIGHT waves whatever the launch has: slots of waves that do not exist - MAXT =
    //  256 for the generic shapes - exist here and hold zeros)
    constexpr int WPW = (MAXT + 63) / 64 < 8 ? 8 : (MAXT + 63) / 64;
    __shared__ __attribute__((aligned(32))) float wpart[2][4 * WPW];
    static_assert(MAXT > 512 || sizeof(wpart) / 2 >= 32 * sizeof(float), "partials_total_all8 reads 32 values per parity");
    constexpr int PK = (128 - 1 + S - 1) / S + 1 + 2;                 // knots a wave's 128 rows can span + a halo knot on either side
    constexpr int PWLEN = (MAXT / 64) * PK * SP;
    static_assert(4 * S - 2 <= 64, "private windows: one halo row per lane");
    __shared__ __attribute__((aligned(16))) float pwin[2][PWLEN];     // [0] = p, [1] = r, wave after wave

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int K = a.K;
    // one system: helper blocks (L2 warm-up of S and Pinv, then dz) as in pcg_single_f64m_kernel
    __shared__ __attribute__((aligned(16))) float hscr[(MAXT / 64) * (4 * S * S + 6 * S)];
    if (a.batch <= 1 && blockIdx.x > 0) {
        one_system_helper<float, S>(a, hscr);
        return;
    }
    const size_t sys = a.batch > 1 ? blockIdx.x : 0;
    const size_t msys = a.rhs > 1 ? sys / (size_t)a.rhs : sys;      // whose S / Pinv / Ginv / C_dense: rhs consecutive workgroups share one system's
    const int j = tid / H, h = tid - j * H;        // knot, row pair (2h, 2h + 1): adjacent, so every matrix column is ONE 8-byte load
    const bool active = j < K;                     // (pairs (h, h + H) cost two scattered 4-byte loads per column: 10 us per launch)
    const int r0 = 2 * h, r1 = 2 * h + 1;

    const float *__restrict__ dS = static_cast<const float *>(a.S_bd) + msys * 3 * S * S * K;
    const float *__restrict__ dP = static_cast<const float *>(a.P_bd) + msys * 3 * S * S * K;
    const float *__restrict__ dG = static_cast<const float *>(a.gamma) + sys * S * K;
    float *__restrict__ dL = static_cast<float *>(a.lambda) + sys * S * K;

    f32x2 sm[3 * S], pm[3 * S];
    if (a.imgS != nullptr) {          // transposed copies written by the assembly launch of this solve (see pcg_single_f64m_kernel)
        const float *__restrict__ iS = static_cast<const float *>(a.imgS) + 2 * tid, *__restrict__ iP = static_cast<const float *>(a.imgP) + 2 * tid;
        const size_t ld = (size_t)a.img_ld;            // rows (2 tid, 2 tid + 1) = (j S + r0, j S + r1): the lane's pair
#pragma unroll
        for (int c = 0; c < 3 * S; ++c) sm[c] = *reinterpret_cast<const f32x2 *>(iS + c * ld);
#pragma unroll
        for (int c = 0; c < 3 * S; ++c) pm[c] = *reinterpret_cast<const f32x2 *>(iP + c * ld);
    } else {
        const size_t base = (size_t)(active ? j : 0) * 3 * S * S;
#pragma unroll
        for (int c = 0; c < 3 * S; ++c) sm[c] = *reinterpret_cast<const f32x2 *>(dS + base + c * S + r0);   // even index: 8-byte aligned
#pragma unroll
        for (int c = 0; c < 3 * S; ++c) pm[c] = *reinterpret_cast<const f32x2 *>(dP + base + c * S + r0);
#pragma unroll
        for (int c = 0; c < 3 * S; ++c) {        // (the selects after ALL loads: see pcg_single_f64m_kernel; 14/7/50 f32 1.423 -> 1.408 us per iteration)
            const bool ok = active && !(j == 0 && c < S) && !(j == K - 1 && c >= 2 * S);   // gato_utils.cuh:157-174
            sm[c] = ok ? sm[c] : f32x2{0.f, 0.f};
            pm[c] = ok ? pm[c] : f32x2{0.f, 0.f};
        }
    }
    for (int i = tid; i < 2 * (MAXK + 2) * SP; i += blockDim.x) (&xs[0][0])[i] = 0.f;
    for (int i = tid; i < 2 * 4 * WPW; i += blockDim.x) (&wpart[0][0])[i] = 0.f;       // partials_total_all8 reads all eight waves' slots
    for (int i = tid; i < 2 * PWLEN; i += blockDim.x) (&pwin[0][0])[i] = 0.f;
    __syncthreads();
    // the wave's rows [R0, R1), its private windows (slot 0 = knot jf - 1) and the lane's halo row
    int hoff = 0, hpo = 0, own_po = 0, win_po = 0;
    bool hvalid = false;
    float *pw_p = nullptr, *pw_r = nullptr;
    {
        const int R0 = 128 * wave, R1 = min(R0 + 128, K * S);
        pw_p = &pwin[0][wave * PK * SP]; pw_r = &pwin[1][wave * PK * SP];
        if (R0 < R1) {
            const int jf = R0 / S, jl = (R1 - 1) / S, base_row = (jf - 1) * S;
            const int nb = R0 - base_row, na = (jl + 2) * S - R1;
            const int hrow = lane < nb ? base_row + lane : R1 + (lane - nb);
            hvalid = lane < nb + na && hrow >= 0 && hrow < K * S;
            const int hj = hvalid ? hrow / S : 0, hr = hvalid ? hrow - hj * S : 0;
            hoff = hvalid ? (hj + 1) * SP + hr : 0;
            hpo = hvalid ? (hj - jf + 1) * SP + hr : 0;
            own_po = active ? (j - jf + 1) * SP + r0 : 0;
            win_po = active ? (j - jf) * SP : 0;
        }
    }

    auto times_window = [&](const f32x2 (&m)[3 * S], const float *xw) -> f32x2 {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
#if GATO_PAIR_CHAINS == 2
        // even and odd columns in chains of their own.  (Written exactly like this: with the accumulators in an array indexed by
        // column % 2 the scheduler ran one whole chain after the other - no gain - and pinning the interleaved order with empty
        // asm statements cost as many wait states as it saved; this form compiles to alternating FMAs without any.)
        f32x2 acc = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 3; ++b) {
#pragma unroll
            for (int i = 0; i < SP / 4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(xw + b * SP + i * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i * 4 + e < S) {
                        if (e & 1) acc1 = __builtin_elementwise_fma(m[b * S + i * 4 + e], f32x2{v[e], v[e]}, acc1);
                        else acc = __builtin_elementwise_fma(m[b * S + i * 4 + e], f32x2{v[e], v[e]}, acc);
                    }
            }
        }
        return acc + acc1;
#else
        f32x2 acc = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 3; ++b) {
#pragma unroll
            for (int i = 0; i < SP / 4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(xw + b * SP + i * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i * 4 + e < S) acc = __builtin_elementwise_fma(m[b * S + i * 4 + e], f32x2{v[e], v[e]}, acc);
            }
        }
        return acc;
#endif
    };
    unsigned epoch = 0;
    // (lanes without rows hold zeros in every vector - their matrix rows are zero - and store them into the zero padding in
    //  front of knot 0 instead of sitting out behind an exec mask, as in pcg_single_f64m_kernel)
    const int put_off = active ? (j + 1) * SP + r0 : r0;
    auto put = [&](float *buf, f32x2 v) { *reinterpret_cast<f32x2 *>(buf + put_off) = v; };

    const float *wp_ = pw_p + win_po, *wr_ = pw_r + win_po;
    auto put_private = [&](float *pw, f32x2 v, float g) {
        if (active) *reinterpret_cast<f32x2 *>(pw + own_po) = v;
        if (hvalid) pw[hpo] = g;
        wave_lds_fence();
    };
    auto block_sum_x = [&](float prod, const float *xw, float &hx) -> float {
        ++epoch;
        float *wp = wpart[epoch & 1];
        partials_store(wp, wave, lane, prod);
        __syncthreads();
        hx = xw[hoff];
        if constexpr (MAXT <= 512) return partials_total_all8<float>(wp, lane);
        return partials_total<float, 16>(wp, nwaves, lane);
    };

    f32x2 lam = {0.f, 0.f};
    f32x2 r = active ? f32x2{dG[(size_t)j * S + r0], dG[(size_t)j * S + r1]} : f32x2{0.f, 0.f};
    if (a.lambda0) {                                                       // true warm start (opt-in)
        const float *__restrict__ dL0 = static_cast<const float *>(a.lambda0) + sys * S * K;
        if (active) lam = f32x2{dL0[(size_t)j * S + r0], dL0[(size_t)j * S + r1]};
        put(xs[0], lam);
        __syncthreads();
        r -= times_window(sm, &xs[0][j * SP]);
        __syncthreads();
    }
    float gr = 0.f, gp = 0.f;                                              // r and p of the lane's halo row
    put(xs[0], r);
    __syncthreads();
    gr = hvalid ? xs[0][hoff] : 0.f;
    put_private(pw_r, r, gr);
    f32x2 rt = times_window(pm, wr_);                                      // gato_pcg.cuh:316-335
    float eta, eta_new = 0.f;
    put(xs[1], rt);
    eta = block_sum_x(r[0] * rt[0] + r[1] * rt[1], xs[1], gp);
    const bool rec = a.eta_hist && tid == 0 && sys == 0;
    if (rec) a.eta_hist[0] = (double)eta;
    f32x2 p = rt, ups;
    put_private(pw_p, p, gp);
    int iters = a.max_iters;
    const float tol = (float)a.exit_tol;
    for (int it = 0; it < a.max_iters; ++it) {                             // gato_pcg.cuh:348
        ups = times_window(sm, wp_);
        float hx = 0.f;
        put(xs[0], ups);
        const float v = block_sum_x(p[0] * ups[0] + p[1] * ups[1], xs[0], hx);
        const float alpha = quotient(eta, v);
        lam += alpha * p;
        r -= alpha * ups;
        gr -= alpha * hx;
        asm volatile("" : "+v"(gr) : : "memory");          // the halo value first: no wait for hx BETWEEN the two LDS writes
        put_private(pw_r, r, gr);
        rt = times_window(pm, wr_);
        put(xs[1], rt);
        eta_new = block_sum_x(r[0] * rt[0] + r[1] * rt[1], xs[1], hx);
        if (rec) a.eta_hist[it + 1] = (double)eta_new;
        if (__builtin_amdgcn_readfirstlane((int)(fabsf(eta_new) < tol))) { iters = it; break; }                   // :404-411
        const float beta = quotient(eta_new, eta);
        p = rt + beta * p;
        eta = eta_new;
        gp = hx + beta * gp;
        asm volatile("" : "+v"(gp) : : "memory");
        put_private(pw_p, p, gp);
    }
    if (a.dz_helpers && a.dz != nullptr && a.batch <= 1) {       // lambda is complete: to the helper blocks without fences, as in pcg_single_f64m_kernel
        if (active) {
            __hip_atomic_store(dL + (size_t)j * S + r0, lam[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(dL + (size_t)j * S + r1, lam[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store((gi32 *)a.dz_flag, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (active) { dL[(size_t)j * S + r0] = lam[0]; dL[(size_t)j * S + r1] = lam[1]; }
    // ---- dz back-substitution in the same launch (batches: one workgroup per system), as in pcg_single_f64m_kernel: formulas and
    // accumulation order of dz_kernel (gato_assembly.hip; gato_schur.cuh:758-867, D2 fixed), row by row: bit-identical results.
    if (a.dz != nullptr && !a.dz_helpers) {
        const int Cn = a.C, n = S + Cn, k = j;
        const size_t gs = (size_t)(S * S + Cn * Cn), cs = (size_t)(S * S + S * Cn), Nn = (size_t)n * K - Cn;
        const float *__restrict__ Gi = static_cast<const float *>(a.dz_Ginv) + msys * (gs * K - (size_t)Cn * Cn);
        const float *__restrict__ Cdn = static_cast<const float *>(a.dz_Cd) + msys * (cs * (K - 1));
        const float *__restrict__ gv = static_cast<const float *>(a.dz_g) + sys * Nn;
        float *__restrict__ dzo = static_cast<float *>(a.dz) + sys * Nn;
        const bool last = k == K - 1;
        __syncthreads();                                                     // every wave has left the loop: both windows are free
        put(xs[0], lam);                                                     // lambda window
        __syncthreads();
        float tx[2] = {0.f, 0.f}, tu[2] = {0.f, 0.f};
        if (active) {
            for (int q = 0; q < 2; ++q) {
                const int rr = r0 + q;
                if (!last) {
                    const float *__restrict__ A = Cdn + (size_t)k * cs;
                    const float *lp = &xs[0][(j + 2) * SP];                  // lambda_{k+1}
                    float res = 0.f;
#pragma unroll
                    for (int t = 0; t < S; ++t) res = gato::fmaT(A[rr * S + t], lp[t], res);          // A_k^T lambda_{k+1}   :833-838
                    tx[q] = gv[(size_t)k * n + rr] - (lam[q] + res);                                  // :841-852
                    if (rr < Cn) {
                        const float *__restrict__ B = A + S * S;
                        float rb = 0.f;
#pragma unroll
                        for (int t = 0; t < S; ++t) rb = gato::fmaT(B[rr * S + t], lp[t], rb);        // B_k^T lambda_{k+1}   :784-789
                        tu[q] = gv[(size_t)k * n + S + rr] - rb;                                      // :792-796
                    }
                } else tx[q] = gv[(size_t)k * n + rr] - lam[q];                                       // last state row (D2)
                xs[1][(j + 1) * SP + rr] = tx[q];
            }
        }
        __syncthreads();                                                     // lambda_{k+1} has been read everywhere
        if (active && !last) {
            for (int q = 0; q < 2; ++q)
                if (r0 + q < Cn) xs[0][(j + 1) * SP + r0 + q] = tu[q];
        }
        __syncthreads();
        if (active) {
            const float *__restrict__ Qi = Gi + (size_t)k * gs;
            const float *tv = &xs[1][(j + 1) * SP];
            for (int q = 0; q < 2; ++q) {
                const int rr = r0 + q;
                float res = 0.f;
#pragma unroll
                for (int cc = 0; cc < S; ++cc) res = gato::fmaT(Qi[rr + cc * S], tv[cc], res);        // Q_k^-1 (...)         :856-865
                dzo[(size_t)k * n + rr] = res;
                if (!last && rr < Cn) {
                    const float *__restrict__ Ri = Qi + S * S;
                    const float *uv = &xs[0][(j + 1) * SP];
                    float ru = 0.f;
                    for (int cc = 0; cc < Cn; ++cc) ru = gato::fmaT(Ri[rr + cc * Cn], uv[cc], ru);    // R_k^-1 (...)         :799-808
                    dzo[(size_t)k * n + S + rr] = ru;
                }
            }
        }
    }
    if (tid == 0) {
        // a helper block that gave up on this launch (see one_system_helper) left dz rows unwritten: in-band, as a hand-off time-out
        const bool dz_lost = a.dz_helpers && a.dz != nullptr && a.batch <= 1 &&
                             __hip_atomic_load((gi32 *)a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
        a.iters[sys] = dz_lost ? -1 : iters;
        if (a.final_eta && sys == 0) *a.final_eta = (double)eta_new;
    }
}

// scheduling pattern for the straight-line block in front of it: DEPTH LDS reads, then (FA FMAs, RA reads) until the reads are
// out - FA : RA = the block's FMAs per read, so that the number of reads in flight stays at DEPTH - then the remaining FMAs
template <int DEPTH, int NREAD, int NFMA, int FA, int RA>
__device__ __forceinline__ void pin_reads_then_fmas()
{
    constexpr int D = DEPTH < NREAD ? DEPTH : NREAD, STEPS = (NREAD - D) / RA, TAILR = NREAD - D - STEPS * RA;
    __builtin_amdgcn_sched_group_barrier(0x100, D, 0);
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x002, FA, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, RA, 0);
    }
    if constexpr (TAILR > 0) {
        __builtin_amdgcn_sched_group_barrier(0x002, FA, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, TAILR, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x002, NFMA - FA * (STEPS + (TAILR > 0 ? 1 : 0)), 0);
}

// (Round 4 also had a HYBRID fp32 kernel here - four two-row waves + four DPP-row waves, one of each per SIMD, option f32_hybrid.
// Measured equal to the kernel above for two rounds (14/7/50: 1.234 against 1.250 us per iteration, 14/7/45 1.232 / 1.220): the
// fp32 iteration is bound by the serial chain around its two block sums, which every wave repeats, not by what a SIMD pulls
// through its LDS return path.  Removed in round 5.)
// threads of the two-rows-per-lane kernel: 2*3S*2 matrix registers + window + state must stay under the cap
// ---- fp64, one workgroup, MIXED rows per lane (IIWA 14/7/50 in fp64 = BASELINE configs[1]) -------------------------------
// The one-workgroup loop is bound by its LDS reads: every lane reads the 3S-entry operand window of its knot for each
// of the two products (16-byte broadcast reads), and 700 rows x 84 doubles do not fit the register file, so part of Pinv
// lives in LDS as well (pcg_resident_kernel<double, 14, 704, NL = 24>: 54 reads per lane and iteration on 11 waves = 594
// wave-reads).  Here 8 waves instead of 11: the lanes of the first W2 waves own TWO adjacent rows of a knot each - both
// rows share every window read - and the other waves own one knot per 16-lane DPP row with S and Pinv entirely in registers
// (round 2's layout had dense one-row waves there: option mixed_dense, removed in round 5 after two rounds of A/B at 1.94
// against 1.54 us per iteration).  Same recurrence, same per-row summation order as every other kernel of the family (a row's
// 3S products are added left to right); block sums as in partials_store.
// ABL: timing-only switches (bench.py's latency floor) as COMPILE-TIME constants - 3 no products, 4 no block sums, 15 loop
// skeleton; with run-time switches this loop compiles 40 % slower than the production kernel, which is no yardstick.
#ifndef GATO_L2_HELPERS
#define GATO_L2_HELPERS 8
#endif
// Round 4.  In-kernel s_memtime stamps of one iteration (tools/f64m_stamps.py, wave by wave) said: products 1020 + 1660 cycles of
// 4560, the two block sums 620 each, quotient + update + window write 260 / 330 - and that the waves sharing a SIMD with a
// two-row wave finish their products late while the two one-row waves that share the fourth SIMD are done after 690 / 770
// cycles = 42 reads x 16: a ds_read_b128 occupies its SIMD's LDS return path for 16 cycles (64 B per clock and SIMD; the 256 B
// per clock of the LDS array needs all four SIMDs reading).  What a SIMD reads per iteration is therefore the bound of the
// products: 126 reads on three SIMDs (two-row wave 21 + 63, one-row wave 21 + 21), 84 on the fourth.  Changes:
//  (1) DR: the one-row waves own 16-lane DPP rows (one knot per row, lanes S..15 idle, row_times_dpp: the operand window comes
//      from the neighbouring lanes' registers, 2 eight-byte LDS reads per product instead of 21 sixteen-byte ones) and FOUR waves
//      hold two rows per lane, one per SIMD beside one DPP wave: the same reads per SIMD and iteration on all four.  The lanes
//      the DPP rows leave idle are paid for by LDS: K2MAX knots x S / 2 two-row lanes keep the ODD columns of S and of Pinv there
//      (the even ones in registers - see m[] below: either product reads 3S/2 windows + 3S/2 pairs, one read per two packed-row
//      FMAs), less Pinv's last NPR odd columns, which stay in registers so that it fits (14/7: 34 knots = 238 lanes + 1 slot of
//      zeros, x 41 pairs x 16 B = 156,784 B + one window 5,824 + partial sums 512 = 163,120 of 163,840 B).  Same per-row
//      summation order as before (left to right): the same bits.
//  (2) the Pinv pairs in LDS through base registers + 16-bit immediate offsets (the compiler gave every column beyond the offset
//      range an address register of its own: 20 VGPRs);
//  (3) the order of LDS reads and FMAs of the two-row products is PINNED (sched_group_barrier: DEPTH reads first, then reads and
//      FMAs in the block's own ratio): the compiler's order keeps 3-5 reads in flight;
//  (4) wave-uniform branches around the two forms of a product (readfirstlane) that start with DIFFERENT empty asm statements:
//      the compiler had hoisted their common first window read and FMA in front of the branch with s_waitcnt lgkmcnt(0)
//      between them - one exposed LDS latency per product.
// Measured and not kept (same box, tools/ab_libs.py): block sums on the matrix core (two v_mfma_f64_16x16x4 with B = ones per
// wave sum + every lane adding the eight wave totals: 1.94 -> 2.04 us per iteration), the divisor-only half of beta = eta' / eta
// formed during the Pinv product (1.835 -> 1.833), Pinv pairs read before the barrier in front of the Pinv product.
#ifndef GATO_F64M_D0
#define GATO_F64M_D0 8      // reads in flight: two-row lanes, S product (21 reads, 84 FMAs)
#endif
#ifndef GATO_F64M_D2
#define GATO_F64M_D2 8      // two-row lanes, Pinv product (60 or 63 reads, 84 FMAs)
#endif
// Round 5, VERDICT r4 #3 - both routes measured, neither kept (profiles/r05_headline_experiments.log, r05_f64m_stamps.log; DESIGN_LOG.md R5.3):
//  (i) the SINGLE-REDUCTION recurrence in this layout (one block sum of two values, three barriers, a second operand window paid
//      for by two more Pinv pairs in registers): 2.36 us per iteration with all vectors in registers (256 VGPRs: the products'
//      landing registers are gone and their LDS reads run two at a time), 1.75 with r and u re-read from the windows, 1.70 with
//      them live between the products only - against 1.55 for the default recurrence.  This layout has 12 registers to spare;
//      the recurrence needs 16 more.  pcg_variant = 1 at this shape therefore stays with the general kernel of gato_pcg_cg1.hip.
//  (ii) neighbour-wave synchronisation instead of the two window barriers (K = 50: a product reads window entries of its own
//      and the adjacent waves only, so a wave bumped an LDS epoch word after its window entries were written and polled the
//      two neighbouring waves' words; built, measured and removed - DESIGN_LOG.md R5.3, profiles/r05_headline_experiments.log):
//      1.684 against 1.555 - two dependent LDS round trips (flag write -> visible -> poll) cost more than s_waitcnt +
//      s_barrier (188 / 120 cycles in the stamps, of which ~100 are the window write's own latency).
template <int S, int W2, int WT, int ABL = 0, int K2MAX = 0, int NPR = 0>
__global__ __launch_bounds__(64 * WT) void pcg_single_f64m_kernel(PcgLaunch a)
{
    typedef double T;
    typedef double V2 __attribute__((ext_vector_type(2)));
    constexpr int SP = pad_to(S, 2), NT = 64 * WT, L2 = 64 * W2;
    constexpr int KD = 4 * (WT - W2);                             // knots of the DPP waves (one per 16-lane row)
    constexpr int L2U = K2MAX * (S / 2);                          // two-row lanes that can own rows
    constexpr int LSTR = L2U + 1;                                 // lane slots per Pinv column in LDS (+ one slot of zeros for the idle lanes)
    constexpr int NC = 3 * S - NPR;                               // column pairs of a two-row lane in LDS (the other 3S + NPR in registers)
    constexpr int MAXK = K2MAX + KD;
    static_assert(S % 2 == 0 && W2 >= 1 && W2 < WT && WT <= 16, "two adjacent rows of one knot per lane in the first W2 waves");
    static_assert(DppRows<S>::ok && DppRows<S>::lanes == 16 && L2U <= L2 && L2U < NT && NPR >= 0 && NPR < 3 * S, "DPP rows: one knot per 16 lanes");
    // ONE operand window: p while the S product reads it, r while the Pinv product does.  Either is written after a barrier
    // behind the other's last read (the block sum's), so the two never meet - and a second window's 5.8 KB are what lets the
    // Pinv pairs of 238 two-row lanes fit the LDS with only NPR of them in registers
    __shared__ __attribute__((aligned(16))) T xs[(MAXK + 2) * SP];
    constexpr int WPW = WT < 8 ? 8 : WT;                                           // partials_total_all8 reads eight waves' slots (zeros beyond WT)
    __shared__ __attribute__((aligned(32))) T wpart[2][4 * WPW];
    static_assert(WT > 8 || sizeof(wpart) / 2 >= 32 * sizeof(T), "partials_total_all8 reads 32 values per buffer");
    __shared__ __attribute__((aligned(16))) V2 ptail[NC][LSTR];                    // Pinv entry NPR + c of (row a, row b) of a two-row lane
    static_assert(sizeof(xs) + sizeof(wpart) + sizeof(ptail) <= 160 * 1024, "LDS of one CU");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool two = __builtin_amdgcn_readfirstlane(wave) < W2;                    // wave-uniform and known as such: scalar branches
    const int K = a.K;
    // One system: the launch brings HELPER blocks (gridDim = 1 + 8 x helpers).  In-kernel time stamps said the solving
    // workgroup spends 15.4 of its 201 us loading its 470 KB of S and Pinv - written a moment ago by the assembly launch on
    // other XCDs, so every line is an L2 miss, and one CU has at most 8 x 63 loads in flight.  The blocks dealt to the XCD of
    // block 0 (blockIdx % 8 == 0: blocks go round-robin over the XCDs) touch every 128-byte line of both arrays once, each
    // thread one line per array, and leave; the solving workgroup's loads then find the lines in that XCD's L2 or merge with
    // the misses in flight.  A speed hint only: wherever the blocks really run, nothing read or written depends on it.
    if (a.batch <= 1 && blockIdx.x > 0) {
        static_assert((size_t)WT * (4 * S * S + 6 * S) * sizeof(T) <= sizeof(ptail), "dz scratch of the helper waves");
        one_system_helper<T, S>(a, reinterpret_cast<T *>(&ptail[0][0]));
        return;
    }
    const size_t sys = a.batch > 1 ? blockIdx.x : 0;
    const size_t msys = a.rhs > 1 ? sys / (size_t)a.rhs : sys;      // whose S / Pinv / Ginv / C_dense: rhs consecutive workgroups share one system's
    // lane -> row(s): the first K - KD knots (at most K2MAX) in the two-row lanes (rows 2 tid, 2 tid + 1), the last KD knots one
    // per 16-lane row of the other waves.
    int row0, j, r0, tp = tid;                                                      // first row, its knot, its row in the knot; lane slot in ptail
    bool active;
    const int K2 = K > KD ? K - KD : 0;
    if (two) {
        row0 = 2 * tid; j = row0 / S; r0 = row0 - j * S;
        active = j < K2;
        tp = tid < L2U ? tid : L2U;
    } else {
        const int q = (tid - L2) >> 4;
        r0 = tid & 15; j = K2 + q;
        active = j < K && r0 < S;
        row0 = j * S + r0;
        tp = 0;
    }
    constexpr int abl = ABL;

    const T *__restrict__ dS = static_cast<const T *>(a.S_bd) + msys * 3 * S * S * K;
    const T *__restrict__ dP = static_cast<const T *>(a.P_bd) + msys * 3 * S * S * K;
    const T *__restrict__ dG = static_cast<const T *>(a.gamma) + sys * S * K;
    T *__restrict__ dL = static_cast<T *>(a.lambda) + sys * S * K;

    // gamma (and lambda0 of a warm start) FIRST: the assembly launch wrote them a moment ago on other XCDs, put(xs, r) and the
    // first product need them at once, and loads return in order - issued behind the matrices they were one more fully exposed
    // miss (entry -> loop entered 7.26 -> 6.80 us, tools/hs_single.py).  One straight line for cold and warm starts: a cold
    // start loads gamma a second time where a warm start loads lambda0, and replaces it by zeros in front of the loop.  (With
    // the lambda0 loads behind `if (a.lambda0)` the compiler zeroed their registers on the other side of the branch - behind
    // an s_waitcnt vmcnt(0), a load of those registers being in flight on the side not taken: gamma's latency, exposed again.)
    V2 lam = {0, 0}, r = {0, 0};
    {
        const T *__restrict__ dL0 = a.lambda0 ? static_cast<const T *>(a.lambda0) + sys * S * K : dG;
        if (active) {
            r[0] = dG[(size_t)j * S + r0];
            lam[0] = dL0[(size_t)j * S + r0];
            if (two) {
                r[1] = dG[(size_t)j * S + r0 + 1];
                lam[1] = dL0[(size_t)j * S + r0 + 1];
            }
        }
    }
    // m: two-row lanes [S row a | S row b], one-row lanes [S row | Pinv row]; pr: the first NPR Pinv pairs of a two-row lane
    // The loads are issued in BATCHES with nothing that needs their data in between: written column by column (load S, load
    // Pinv, select, store the Pinv pair to LDS) the compiler reused one set of registers and waited for every column's loads
    // before the next (84 memory round trips in a row: 9 us of a 198 us launch even with every line in L2).
    // Two-row lanes keep 3S + NPR column PAIRS (row a, row b) in registers, the other 3S - NPR in LDS: the EVEN columns of both
    // matrices in registers (and the last NPR odd ones of Pinv), the odd ones in LDS - either product then reads 3S/2 windows +
    // 3S/2 pairs, one read per two FMAs throughout.
    T m[6 * S + 2 * NPR];
    auto in_reg = [](int which, int c) -> bool {
        return c % 2 == 0 || (which == 1 && c >= 3 * S - 2 * NPR);
    };
    auto reg_idx = [](int which, int c) -> int {             // pair index in m (entries 2 i, 2 i + 1)
        if (c % 2 == 0) return (which ? 3 * S / 2 : 0) + c / 2;
        return 3 * S + (c - (3 * S - 2 * NPR)) / 2;
    };
    auto lds_idx = [](int which, int c) -> int {             // column slot in ptail
        return (which ? 3 * S / 2 : 0) + (c - 1) / 2;
    };
    {
        const bool in_sys = active && j < K;
        const size_t base = (size_t)(in_sys ? j : 0) * 3 * S * S + (r0 < S ? r0 : 0);
        auto ok_col = [&](int c) { return active && !(j == 0 && c < S) && !(j == K - 1 && c >= 2 * S); };   // gato_utils.cuh:157-174
        auto keep_pair = [&](int which, int c, V2 v) {                             // pair of column c of S (0) / Pinv (1): registers or LDS slot
            if (in_reg(which, c)) { m[2 * reg_idx(which, c)] = v[0]; m[2 * reg_idx(which, c) + 1] = v[1]; }
            else ptail[lds_idx(which, c)][tp] = v;                                 // own slot (idle lanes: zeros, all into the one spare slot)
        };
        if (a.imgS != nullptr) {
            // the assembly launch of this solve also left S and Pinv transposed (column c of ALL rows contiguous, zeros where a
            // block or a row does not exist): the lane's entries are unit-stride across the wave, no boundary selects (a lane
            // without rows of its own reads rows of other lanes and drops them)
            const int rowc = active ? row0 : 0;
            const T *__restrict__ iS = static_cast<const T *>(a.imgS) + rowc, *__restrict__ iP = static_cast<const T *>(a.imgP) + rowc;
            const size_t ld = (size_t)a.img_ld;
            if (two) {
                V2 sv[3 * S];
#pragma unroll
                for (int c = 0; c < 3 * S; ++c) sv[c] = *reinterpret_cast<const V2 *>(iS + c * ld);      // row0 even, ld even: 16-byte aligned
#pragma unroll
                for (int c = 0; c < 3 * S; ++c) keep_pair(0, c, active ? sv[c] : V2{0, 0});
                constexpr int PB = 14;
#pragma unroll
                for (int c0 = 0; c0 < 3 * S; c0 += PB) {
                    V2 pv[PB];
#pragma unroll
                    for (int q = 0; q < PB; ++q) pv[q] = *reinterpret_cast<const V2 *>(iP + (c0 + q) * ld);
#pragma unroll
                    for (int q = 0; q < PB; ++q) keep_pair(1, c0 + q, active ? pv[q] : V2{0, 0});
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3 * S; ++c) m[c] = iS[c * ld];
#pragma unroll
                for (int c = 0; c < 3 * S; ++c) m[3 * S + c] = iP[c * ld];
#pragma unroll
                for (int c = 0; c < 6 * S; ++c) m[c] = active ? m[c] : (T)0;
            }
        } else if (two) {
            V2 sv[3 * S];
#pragma unroll
            for (int c = 0; c < 3 * S; ++c) sv[c] = *reinterpret_cast<const V2 *>(dS + base + (size_t)c * S);   // rows r0, r0 + 1: adjacent, 16-byte aligned
#pragma unroll
            for (int c = 0; c < 3 * S; ++c) keep_pair(0, c, ok_col(c) ? sv[c] : V2{0, 0});
            constexpr int PB = 14;                                                            // Pinv pairs per batch (56 registers)
            static_assert((3 * S) % PB == 0, "batches of Pinv columns");
#pragma unroll
            for (int c0 = 0; c0 < 3 * S; c0 += PB) {
                V2 pv[PB];
#pragma unroll
                for (int q = 0; q < PB; ++q) pv[q] = *reinterpret_cast<const V2 *>(dP + base + (size_t)(c0 + q) * S);
#pragma unroll
                for (int q = 0; q < PB; ++q) keep_pair(1, c0 + q, ok_col(c0 + q) ? pv[q] : V2{0, 0});
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3 * S; ++c) m[c] = dS[base + (size_t)c * S];
#pragma unroll
            for (int c = 0; c < 3 * S; ++c) m[3 * S + c] = dP[base + (size_t)c * S];
#pragma unroll
            for (int c = 0; c < 3 * S; ++c) {
                const bool ok = ok_col(c);
                m[c] = ok ? m[c] : (T)0;
                m[3 * S + c] = ok ? m[3 * S + c] : (T)0;
            }
        }
    }
    for (int i = tid; i < (MAXK + 2) * SP; i += NT) xs[i] = (T)0;
    for (int i = tid; i < 2 * 4 * WPW; i += NT) (&wpart[0][0])[i] = (T)0;
    __syncthreads();

    // the lane's Pinv pairs in LDS: column NPR + c at ptail[c][tp].  A few LDS base registers, the rest 16-bit immediate offsets.
    typedef __attribute__((address_space(3))) V2 LV2;
    constexpr int PCH = 65535 / (LSTR * 16) + 1 < NC ? 65535 / (LSTR * 16) + 1 : NC;     // columns per base register
    constexpr int NBASE = (NC + PCH - 1) / PCH;
    static_assert((PCH - 1) * LSTR * 16 < 65536 && NBASE <= 4, "immediate offsets of a base register's columns");
    LV2 *ptb[NBASE];
#pragma unroll
    for (int i = 0; i < NBASE; ++i) {
        ptb[i] = (LV2 *)&ptail[i * PCH][tp];
        if (i > 0) asm volatile("" : "+v"(ptb[i]));               // opaque: or the compiler re-derives it from ptb[0] with a 17-bit offset
    }
    auto pair_of = [&](int which, int c) -> V2 {
        if (in_reg(which, c)) return V2{m[2 * reg_idx(which, c)], m[2 * reg_idx(which, c) + 1]};
        return ptb[lds_idx(which, c) / PCH][(lds_idx(which, c) % PCH) * LSTR];
    };
    // y = [L M R]_row . window for the lane's row(s); which = 0: S, 1: Pinv; own: the lane's own entries of the operand (DPP rows)
    auto times_window = [&](int which, const T *xw, V2 own) -> V2 {
        T ya = (T)0, yb = (T)0;
        constexpr int NW = 3 * (SP / 2);                                         // window reads of a product
        if (two) {
            asm volatile("; two rows per lane" ::: "memory");
#pragma unroll
            for (int b = 0; b < 3; ++b) {
#pragma unroll
                for (int i = 0; i < SP / 2; ++i) {
                    const V2 v = *reinterpret_cast<const V2 *>(xw + b * SP + i * 2);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int c = b * S + i * 2 + e;
                        if (i * 2 + e < S) {
                            const V2 t = pair_of(which, c);
                            ya = gato::fmaT(t[0], v[e], ya);
                            yb = gato::fmaT(t[1], v[e], yb);
                        }
                    }
                }
            }
            if (which == 0) pin_reads_then_fmas<GATO_F64M_D0, NW + 3 * S / 2, 6 * S, 4, 2>();
            else pin_reads_then_fmas<GATO_F64M_D2, NW + 3 * S / 2 - NPR, 6 * S, 4, 2>();
        } else {
            asm volatile("; one row per lane, DPP rows" ::: "memory");
            const int rc = r0 < S ? r0 : S - 1;                                  // idle lanes read inside the window (their rows are zero)
            const T x3[3] = {xw[rc], own[0], xw[2 * SP + rc]};                   // the lane's row index in knots j - 1, j, j + 1
            ya = row_times_dpp<T, S>(*reinterpret_cast<const T(*)[3 * S]>(m + (which ? 3 * S : 0)), x3);
        }
        return V2{ya, yb};
    };
#ifdef GATO_F64M_STAMP      // scratch builds only (tools/f64m_stamps.py): s_memtime at the phase boundaries of ONE iteration, per wave
    unsigned long long st_[16] = {};
    bool st_on = false;
#define GATO_ST(i) do { if (st_on) st_[i] = clock64(); } while (0)
#else
#define GATO_ST(i) do { } while (0)
#endif
    // `which`: the partials buffer of this call site - consecutive block sums alternate between the two (p . upsilon in [0],
    // r . r~ in [1]), so a wave may store its next partials while a slower one still reads the previous ones
    auto block_sum = [&](T prod, int si, int which) -> T {
        if (abl & 4) return (T)1 + prod * (T)1e-30;
        T *wp = wpart[which];
        partials_store(wp, wave, lane, prod);
#ifdef GATO_F64M_STAMP
        if (st_on) st_[si] = clock64();
#endif
        __syncthreads();
#ifdef GATO_F64M_STAMP
        if (st_on) st_[si + 1] = clock64();
#endif
        if constexpr (WT <= 8) return partials_total_all8<T>(wp, lane);        // (wpart is zeroed at set-up: waves beyond WT add zeros)
        return partials_total<T, (WT <= 8 ? 8 : 16)>(wp, WT, lane);
    };
    // own entries into the operand window.  Lanes without rows hold zeros in every vector (their matrix rows are zero): they
    // store them into the zero padding in front of knot 0 instead of sitting out behind an exec mask - no mask, no branch but the
    // wave-uniform one in the loop
    const int put_off = active ? (j + 1) * SP + r0 : (r0 < S ? r0 & ~1 : 0);
    auto put = [&](T *buf, V2 v) {                                               // (1.567 -> 1.537 us per iteration against the masked form)
        if (two) *reinterpret_cast<V2 *>(buf + put_off) = v;                    // r0 even, SP even: aligned
        else buf[put_off] = v[0];
    };
    const T *wp_ = &xs[j * SP], *wr_ = wp_;                                      // the lane's window: slot j = left neighbour

    if (a.lambda0) {                                                             // true warm start (opt-in): lam holds lambda0
        put(xs, lam);
        __syncthreads();
        r -= times_window(0, wp_, lam);
        __syncthreads();
    }
    const bool rec = a.eta_hist && tid == 0 && sys == 0;
    int iters = a.max_iters;
    const T tol = (T)a.exit_tol;
    T eta = (T)0, eta_new = (T)0;
    put(xs, r);
    __syncthreads();
    V2 rt = times_window(1, wr_, r);                                             // gato_pcg.cuh:316-335
    eta = block_sum(r[0] * rt[0] + r[1] * rt[1], 0, 1);
    if (rec) a.eta_hist[0] = (double)eta;
    V2 p = rt, ups;
    put(xs, p);
    if (!a.lambda0) lam = V2{0, 0};                                              // cold start (see the loads of gamma)
    __syncthreads();
    for (int it = 0; it < a.max_iters; ++it) {                                   // gato_pcg.cuh:348
#ifdef GATO_F64M_STAMP
        st_on = it == a.max_iters - 2;
#endif
        GATO_ST(0);
        ups = (abl & 1) ? p * m[0] : times_window(0, wp_, p);                    // upsilon = S p         (:349-351)
        GATO_ST(1);
        const T v = block_sum(p[0] * ups[0] + p[1] * ups[1], 2, 0);              // v = p . upsilon       (:353-357)
        GATO_ST(4);
        const T alpha = quotient(eta, v);                                        // :364
        lam += alpha * p;                                                        // :373-377
        r -= alpha * ups;
        put(xs, r);
        GATO_ST(5);
        if (!(abl & 8)) __syncthreads();
        GATO_ST(6);
        rt = (abl & 2) ? r * m[1] : times_window(1, wr_, r);                     // r~ = Pinv r           (:380-381)
        GATO_ST(7);
        eta_new = block_sum(r[0] * rt[0] + r[1] * rt[1], 8, 1);                  // eta' = r . r~         (:382-394)
        GATO_ST(10);
        if (rec) a.eta_hist[it + 1] = (double)eta_new;
        if (__builtin_amdgcn_readfirstlane((int)(fabs(eta_new) < tol))) { iters = it; break; }   // :404-411 (eta' is the same in every lane)
        const T beta = quotient(eta_new, eta);                                   // :415
        p = rt + beta * p;                                                       // :416-419
        put(xs, p);
        eta = eta_new;                                                           // :420
        GATO_ST(11);
        if (!(abl & 8)) __syncthreads();
        GATO_ST(12);
    }
#ifdef GATO_F64M_STAMP
    if (a.eta_hist && lane == 0 && sys == 0)
        for (int i = 0; i < 13; ++i) a.eta_hist[1024 + wave * 16 + i] = (double)(st_[i] & 0xffffffffffull);
#endif
    if (a.dz_helpers && a.dz != nullptr && a.batch <= 1) {
        // lambda is complete: hand it to the helper blocks WITHOUT fences.  Every byte is stored write-through (agent scope:
        // sc1), every storing wave drains its stores, a workgroup barrier, then ONE lane stores the flag; the helpers poll the
        // flag and read lambda with agent-scope loads, and nothing else that this launch wrote (one_system_helper).  An
        // agent-scope release here (buffer_wbl2 in all 512 threads) and the acquire there cost 3.3 us: loop left -> dz
        // stored 6.08 -> 2.82 us (tools/hs_single.py).  The kernel's end makes lambda visible to later launches as before.
        if (active) {                                                            // :433-435
            __hip_atomic_store(dL + (size_t)j * S + r0, lam[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (two) __hip_atomic_store(dL + (size_t)j * S + r0 + 1, lam[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store((gi32 *)a.dz_flag, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (active) {                                                         // :433-435
        dL[(size_t)j * S + r0] = lam[0];
        if (two) dL[(size_t)j * S + r0 + 1] = lam[1];
    }
    // ---- dz back-substitution in the same launch (batches: one workgroup per system).  Formulas and accumulation order of
    // dz_kernel (gato_assembly.hip; gato_schur.cuh:758-867, D2 fixed), row by row: bit-identical results.
    if (a.dz != nullptr && !a.dz_helpers) {
        const int Cn = a.C, n = S + Cn, k = j, nrow = two ? 2 : 1;
        const size_t gs = (size_t)(S * S + Cn * Cn), cs = (size_t)(S * S + S * Cn), Nn = (size_t)n * K - Cn;
        const T *__restrict__ Gi = static_cast<const T *>(a.dz_Ginv) + msys * (gs * K - (size_t)Cn * Cn);
        const T *__restrict__ Cdn = static_cast<const T *>(a.dz_Cd) + msys * (cs * (K - 1));
        const T *__restrict__ gv = static_cast<const T *>(a.dz_g) + sys * Nn;
        T *__restrict__ dzo = static_cast<T *>(a.dz) + sys * Nn;
        const bool last = k == K - 1;
        __syncthreads();                                                         // every wave has left the loop: the window and the Pinv pairs are free
        T *xs0 = xs, *xs1 = reinterpret_cast<T *>(&ptail[0][0]);                 // two windows for the back-substitution
        static_assert(sizeof(xs) <= sizeof(ptail), "second window of the dz epilogue");
        put(xs0, lam);                                                           // lambda window
        __syncthreads();
        T tx[2] = {0, 0}, tu[2] = {0, 0};
        if (active) {
            for (int q = 0; q < nrow; ++q) {
                const int rr = r0 + q;
                if (!last) {
                    const T *__restrict__ A = Cdn + (size_t)k * cs;
                    const T *lp = &xs0[(j + 2) * SP];                          // lambda_{k+1}
                    T res = (T)0;
#pragma unroll
                    for (int t = 0; t < S; ++t) res = gato::fmaT(A[rr * S + t], lp[t], res);          // A_k^T lambda_{k+1}   :833-838
                    tx[q] = gv[(size_t)k * n + rr] - (lam[q] + res);                                  // :841-852
                    if (rr < Cn) {
                        const T *__restrict__ B = A + S * S;
                        T rb = (T)0;
#pragma unroll
                        for (int t = 0; t < S; ++t) rb = gato::fmaT(B[rr * S + t], lp[t], rb);        // B_k^T lambda_{k+1}   :784-789
                        tu[q] = gv[(size_t)k * n + S + rr] - rb;                                      // :792-796
                    }
                } else tx[q] = gv[(size_t)k * n + rr] - lam[q];                                       // last state row (D2)
                xs1[(j + 1) * SP + rr] = tx[q];
            }
        }
        __syncthreads();                                                         // lambda_{k+1} has been read everywhere
        if (active && !last) {
            for (int q = 0; q < nrow; ++q)
                if (r0 + q < Cn) xs0[(j + 1) * SP + r0 + q] = tu[q];
        }
        __syncthreads();
        if (active) {
            const T *__restrict__ Qi = Gi + (size_t)k * gs;
            const T *tv = &xs1[(j + 1) * SP];
            for (int q = 0; q < nrow; ++q) {
                const int rr = r0 + q;
                T res = (T)0;
#pragma unroll
                for (int cc = 0; cc < S; ++cc) res = gato::fmaT(Qi[rr + cc * S], tv[cc], res);        // Q_k^-1 (...)         :856-865
                dzo[(size_t)k * n + rr] = res;
                if (!last && rr < Cn) {
                    const T *__restrict__ Ri = Qi + S * S;
                    const T *uv = &xs0[(j + 1) * SP];
                    T ru = (T)0;
                    for (int cc = 0; cc < Cn; ++cc) ru = gato::fmaT(Ri[rr + cc * Cn], uv[cc], ru);    // R_k^-1 (...)         :799-808
                    dzo[(size_t)k * n + S + rr] = ru;
                }
            }
        }
    }
    if (tid == 0) {
        // a helper block that gave up on this launch (see one_system_helper) left dz rows unwritten: in-band, as a hand-off time-out
        const bool dz_lost = a.dz_helpers && a.dz != nullptr && a.batch <= 1 &&
                             __hip_atomic_load((gi32 *)a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
        a.iters[sys] = dz_lost ? -1 : iters;
        if (a.final_eta && sys == 0) *a.final_eta = (double)eta_new;
    }
}

}  // namespace

template <typename T, int S>
int launch_pcg_single(const PcgLaunch &a, bool mr, hipStream_t st)
{
    if constexpr (sizeof(T) == 4 && S % 2 == 0 && PairThreads<S>::v > 0) {
        if (a.pair) {
            constexpr int PT = PairThreads<S>::v;
            if (a.groups != 1 || a.threads > PT || a.threads % 64 != 0 || a.K * (S / 2) > a.threads) {
                set_error("pcg_resident(pair): bad geometry K=%d threads=%d max=%d", a.K, a.threads, PT);
                return GATO_EINVAL;
            }
            // one system: + helper blocks (enough waves for one knot each: they also do dz), see pcg_single_f64m_kernel
            const int helpers = (a.K + a.threads / 64 - 1) / (a.threads / 64);
            const dim3 grid(a.batch > 1 ? a.batch : 1 + 8 * helpers);
            return pcg_launch(pcg_single_f32x2_kernel<S, PT>, grid, dim3(a.threads), a, st);
        }
    }
    if constexpr (sizeof(T) == 8 && MixedCfg<S>::wt > 0) {
        if (a.pair == 2) {
            constexpr int W2 = MixedCfg<S>::w2, WT = MixedCfg<S>::wt, K2 = MixedCfg<S>::k2, NPR = MixedCfg<S>::npr;
            if (mr || a.groups != 1 || a.threads != 64 * WT || a.K * S > mixed_rows<S>() || a.stamps) {
                set_error("pcg_resident(mixed): bad launch K=%d threads=%d", a.K, a.threads);
                return GATO_EINVAL;
            }
            static_assert(GATO_L2_HELPERS * WT * S >= mixed_rows<S>(), "one helper wave per knot (they do dz)");
            const dim3 grid(a.batch > 1 ? a.batch : 1 + 8 * GATO_L2_HELPERS), block(64 * WT);          // one system: + helper blocks that warm the L2
            const int abl = a.diag == 2 ? a.ablate : 0;
            return pcg_launch(abl == 3 ? pcg_single_f64m_kernel<S, W2, WT, 3, K2, NPR>
                              : abl == 4 ? pcg_single_f64m_kernel<S, W2, WT, 4, K2, NPR>
                              : abl == 15 ? pcg_single_f64m_kernel<S, W2, WT, 15, K2, NPR> : pcg_single_f64m_kernel<S, W2, WT, 0, K2, NPR>,
                              grid, block, a, st);
        }
    }
    set_error("pcg_resident: no one-workgroup two-rows-per-lane kernel for this shape and type (pair=%d)", a.pair);
    return GATO_EINVAL;
}

#define X(S_, C_)                                                          \
    template int launch_pcg_single<float, S_>(const PcgLaunch &, bool, hipStream_t); \
    template int launch_pcg_single<double, S_>(const PcgLaunch &, bool, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
