// Resident PCG for gfx950: the whole preconditioned-CG solve on the block-tridiagonal Schur
// system in ONE persistent launch, matrices register-resident.
//
// Replaces parallelPCG / parallelPCG_inner (src/gato_pcg.cuh:270-470) and its helpers
// loadBlockTriDiagonal_offDiagonal / matVecMultBlockTriDiagonal (src/gato_utils.cuh:121-185),
// dotProd / reducePlus (:253-287) and the atomicAdd + grid.sync() reductions (gato_pcg.cuh:331-393).
//
// MI355X design (not the reference's one-block-of-S-threads-per-knot):
//  * lane = one row of one knot; the lane keeps its 3S entries of S and 3S entries of Pinv in
//    VGPRs for the whole solve (84 VGPRs fp32 / 168 fp64 at S=14) - the 128 MB register file of
//    the chip holds every BASELINE shape, so the hot loop touches no HBM at all.
//  * a workgroup owns a contiguous range of knots; the 3S-wide operand window [x_{k-1};x_k;x_{k+1}]
//    is read from LDS with 16-byte broadcast reads (knot stride padded to 16 B multiples).
//  * dots: in-lane product -> wave64 butterfly -> per-wave LDS partial -> fixed-order sum.
//    Deterministic, no float atomics (the reference's atomicAdd order is unspecified).
//  * one workgroup (K=50 fp32: 11 waves on one CU): no inter-workgroup traffic at all, six
//    s_barriers per iteration.
//  * several workgroups: two hand-offs per iteration (the algorithmic minimum for PCG).  Each
//    workgroup publishes [partial dot | first S-block | last S-block] of the vector it just
//    produced as 8-byte {epoch,payload} granules (write-through agent-scope stores), wave 0 of
//    every workgroup sweeps the W partials and its two neighbours' blocks until every tag equals
//    the epoch (MI355X guide: "R2: the data IS the flag").  Ghost blocks of r and p are then
//    advanced locally (ghost_r -= alpha*ghost_upsilon, ghost_p = ghost_rtilde + beta*ghost_p), so
//    the reference's four grid.sync() per iteration become two all-gathers and no barrier.
//    Granules are double-buffered by epoch parity; every spin is bounded.
#pragma once
#include <type_traits>

#include "gato_pcg_device.h"

namespace gato {
namespace {

template <typename T, int S, int MAXT>
struct ResidentCfg {
    static constexpr int VW = VecOf<T>::W;
    static constexpr int SP = pad_to(S, VW);           // padded knot stride in LDS (16-B multiple)
    static constexpr int MAXK = (MAXT + S - 1) / S;    // local knots incl. the partly filled one
    static constexpr int NV = SP / VW;
    static constexpr int MAXW = 256;                   // workgroups (one per CU)
    static constexpr int PM = MAXW / 64;               // partial granule loads per lane
};

// STAMP: diagnostic build only - wave 0 of workgroup 0 accumulates s_memtime deltas per segment into
// a.stamps (never used for timing claims; it perturbs the schedule).
#define GATO_STAMP(i)                                                                       \
    if (STAMP) {                                                                            \
        if (wg == 0 && wave == 0) {                                                         \
            unsigned long long t_;                                                          \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
            seg[i] += t_ - t_prev;                                                          \
            t_prev = t_;                                                                    \
        }                                                                                   \
    }

// Same product with the last NL entries of the row read from LDS (16 B per lane, lane-contiguous: conflict
// free) instead of registers.  Needs S % VW == 0 and (3S-NL) % VW == 0 so that vectors never straddle blocks.
template <typename T, int S, int SP, int NL, int MAXT>
__device__ __forceinline__ T row_times_window_lds(const T (&m)[3 * S - NL], const typename VecOf<T>::type (*tail)[MAXT],
                                                  int tid, const T *xw)
{
    typedef typename VecOf<T>::type V;
    constexpr int VW = VecOf<T>::W;
    constexpr int NREG = 3 * S - NL;
    static_assert(S % VW == 0 && NREG % VW == 0 && NL % VW == 0, "vector alignment");
    T acc = (T)0;
#pragma unroll
    for (int c = 0; c < NREG; c += VW) {
        V v = *reinterpret_cast<const V *>(xw + (c / S) * SP + (c % S));
#pragma unroll
        for (int e = 0; e < VW; ++e) acc = gato::fmaT(m[c + e], v[e], acc);
    }
#pragma unroll
    for (int c = NREG; c < 3 * S; c += VW) {
        V v = *reinterpret_cast<const V *>(xw + (c / S) * SP + (c % S));
        V mv = tail[(c - NREG) / VW][tid];
#pragma unroll
        for (int e = 0; e < VW; ++e) acc = gato::fmaT(mv[e], v[e], acc);
    }
    return acc;
}

// Same product for a row whose 3S matrix entries are NOT register resident: they are loaded (L2 / Infinity Cache /
// HBM) every time, all 3S loads in flight before the first FMA.  Rows handled this way are never in the system's
// first or last block row, so no boundary entries have to be zeroed.
template <typename T, int S, int SP>
__device__ __forceinline__ T row_from_memory(const T *__restrict__ src, const T *xw, bool no_left = false, bool no_right = false)
{
    T m[3 * S];
#pragma unroll
    for (int c = 0; c < 3 * S; ++c) m[c] = src[(size_t)c * S];
    // first / last block row of the system: the left / right block is not part of the matrix (never written) - drop it
#pragma unroll
    for (int c = 0; c < S; ++c) {
        if (no_left) m[c] = (T)0;
        if (no_right) m[2 * S + c] = (T)0;
    }
    return row_times_window<T, S, SP>(m, xw);
}

// NL > 0: single-workgroup variant whose Pinv rows do not fit the register budget: the last NL entries of
// every Pinv row live in LDS (IIWA 14/7/50 in fp64: 700 rows x 84 doubles = 470 KB > the 168 VGPRs/lane that
// 11 waves on one CU leave; 24 doubles per row = 135 KB go to LDS, the rest stays in registers).
// XR > 0: SEMI-resident variant for K beyond the register file: a workgroup owns more knots than it
// has lanes for.  The first n_res-1 knots and the LAST knot of its range keep the lane = row mapping above (so the
// boundary blocks the hand-off publishes are resident rows and nothing of the hand-off changes); the knots in between
// are "extra" rows, up to XR per lane: their r and p entries live in the LDS operand windows anyway, lambda and the
// product just formed in two more LDS arrays,
// their matrix rows are re-read from memory (mostly L2 / Infinity Cache at these sizes) in every product, one row per
// trip of a plain runtime loop (unrolling it cost registers and instruction cache and ran slower).  Still ONE persistent launch with
// two hand-offs per iteration - against two launches per iteration of the streaming kernels.
// NR (with XR > 0): NO resident rows at all - every row of the workgroup's range is an "extra" row.  Without the 6S
// matrix registers per lane the workgroup can be 2-4x larger (more loads in flight per CU): the variant for shapes whose
// resident rows leave one wave per SIMD (fp64, S = 32) and for the HBM-bound end of the range.  The boundary blocks the
// hand-off publishes are then read from the product array in LDS instead of from lane registers.
// MR: cluster launch (gato_cluster_pcg) - this kernel is ONE RANK of a solve whose knots are sharded over the GPUs of a
// node (the reference is single-device, gato_utils.cuh:831).  The hand-off gets a second level:
// after the workgroups of this GPU have gathered their partials (level 1, unchanged), workgroup 0 stores the rank's
// total into EVERY rank's mirror (peer-mapped fine-grained memory: xGMI peer stores, system scope), the rank's first /
// last workgroup store their boundary block into the left / right neighbour rank's mirror, and wave 0 of every
// workgroup polls its OWN GPU's mirror until the R totals (and, at the rank's edges, the neighbour's block) carry the
// epoch; totals are summed in rank order (identical on every rank => identical exit decision).  The grid barriers of
// the reference (gato_pcg.cuh:363,378,393,428) thus become two device-initiated all-gathers per iteration across the
// node, no host involvement, no collective library inside the loop.
// WP: launches of 2..32 workgroups of the plain variant.  EVERY WAVE publishes its own partial (one granule per wave in line 0
// of the workgroup's slot - still one writing workgroup per line) and the polling wave of every workgroup reads W x waves
// granules: the same W lines as before, coalesced.  The gather of the workgroup's total in wave 0 (LDS write, barrier B1, LDS
// read, second DPP sum) leaves the critical path of the hand-off and an iteration has four barriers instead of six.  (Not the
// "every wave polls" form that DESIGN.md 3.1 records as a dead end: one polling wave per workgroup it stays.)  The ghost
// blocks of r and p live in registers of the polling lanes (lanes 0..S-1 left, 32..32+S-1 right) - no staging array, no LDS
// read-modify-write on the way to the next product.  A compile-time variant: as a run-time switch in the one kernel the
// extra scalar paths cost every launch 3-5 % (measured, same box: 14/7/512 f32 2.93 -> 3.02 us per iteration).
// WPM = poll loads per lane of that form (0 = the gathered form): 4 serves W << ceil(log2(waves)) <= 256 granules (up to 32
// workgroups of 8 waves).  Measured and rejected: 16 loads per lane for up to 128 workgroups (14/7/4096 f32, W = 114: 4.77 us
// per iteration against 3.87 gathered - fifteen load instructions per sweep cost more than the gather they replace).
// DR: DPP-row layout (gato_pcg_device.h: row_times_dpp) - a knot owns whole 16-lane DPP rows and the products read their operand
// window from the neighbouring lanes' REGISTERS (v_fmac_*_dpp row_newbcast) instead of 16-byte LDS reads: the LDS-window
// products are bound by the LDS return path (fp64 14/7: 1.13 us of a 3.56 us iteration at 15 workgroups, 21 16-byte reads per
// lane and product), this form reads two scalars per lane and product.  Same summation order per row: identical bits.
// Plain and cluster launches (NL = 0, XR = 0); lanes S..15 of a row idle (S = 14: 32 knots per 512 threads instead of 36).
template <typename T, int S, int MAXT, int NL = 0, int DIAG = 0, int XR = 0, bool NR = false, bool MR = false, int WPM = 0, bool DR = false>
__global__ __launch_bounds__(MAXT) void pcg_resident_kernel(PcgLaunch a)
{
    static_assert(!DR || (NL == 0 && XR == 0 && !NR && DIAG != 1 && DppRows<S>::ok), "DPP-row layout: plain and cluster variants");
    constexpr int LPK = DR ? DppRows<S>::lanes : S;                            // lanes per knot
    constexpr bool WP = WPM > 0;            // per-wave published partials
    constexpr bool RG = WPM != 0;           // ghost blocks in the polling lanes' registers (WPM = -1: that alone, gathered partials)
    static_assert(!RG || (NL == 0 && XR == 0 && !NR && DIAG != 1), "wave-published partials / register ghosts: plain and cluster variants");
    // DIAG: 0 = production; 1 = cycle stamps + the timing-only switches of a.ablate; 2 = the switches alone (what
    // bench.py's latency floor times: the stamps cost registers, and this instantiation has none to spare)
    constexpr bool STAMP = DIAG == 1, ABL = DIAG != 0;
    typedef ResidentCfg<T, S, MAXT> Cfg;
    typedef Granule<T> Gr;
    typedef GranuleXcd<T> LGr;
    typedef GranuleSys<T> XGr;
    constexpr int SP = Cfg::SP;
    constexpr int GPV = Gr::GPV;
    // hand-off layout invariant (DESIGN.md 3.1 dead end 2: granules of two writers in one 128-B line get lost across
    // XCDs): a workgroup's slot is a whole number of 128-B lines (16 granules), the partial has line 0 to itself
    static_assert(MAXT % 64 == 0 && 2 * S * GPV <= 16 * ((2 * S * GPV + 15) / 16), "slot layout");
    static_assert(!MR || (NL == 0 && DIAG == 0), "cluster launches use the plain and the semi-resident variants");
    static_assert(DIAG == 0 || !MR, "diagnostic builds are single-GPU");

    constexpr int MAXKX = NR ? Cfg::MAXK * XR : Cfg::MAXK * (1 + XR);          // local knots incl. the extra ones
    static_assert(NL == 0 || XR == 0, "the LDS-tail variant is single-workgroup only");
    static_assert(!NR || (XR > 0 && 2 * S <= 64), "NR: every row is an extra row; wave 0 publishes both boundary blocks");
    __shared__ __attribute__((aligned(16))) T xs[2][(MAXKX + 2) * SP];        // [0] = p window, [1] = r window
    __shared__ __attribute__((aligned(32))) T wpart[2][4 * ((MAXT + 63) / 64)];   // per-wave, per-row partial dots, double-buffered by epoch parity
    typedef typename VecOf<T>::type V;
    constexpr int NREG = 3 * S - NL;
    __shared__ __attribute__((aligned(16))) V ptail[NL > 0 ? NL / VecOf<T>::W : 1][NL > 0 ? MAXT : 1];
    __shared__ T gh[2][32];          // ghost blocks of the vector just gathered: [0] left, [1] right
    __shared__ T bc[2];              // broadcast scalars
    __shared__ int s_abort;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    // batch > 1: one workgroup per independent system (blockIdx.x = system), no inter-workgroup traffic
    const bool batched = a.batch > 1;
    // xcd_pack = X in 1..7: blocks are dealt round-robin over the 8 XCDs, so with an oversubscribed grid of 8*per blocks
    // of which only those with blockIdx % 8 < X work, the W working groups sit on X XCDs, neighbouring knot ranges on
    // the same one (hand-offs inside an XCD are 15-20 % faster).  A speed hint only: nothing below depends on where a
    // block really runs.
    const int X = a.xcd_pack;
    const int xres = X > 0 ? (int)((blockIdx.x - (unsigned)a.xcd_sel) & 7) : 0;      // a.xcd_sel: which XCD(s) of the eight host the working blocks
    if (X > 0 && xres >= X) return;
    const int per_x = X > 0 ? (int)(gridDim.x >> 3) : 0;
    const int wg = batched ? 0 : (X > 0 ? xres * per_x + (int)(blockIdx.x >> 3) : (int)blockIdx.x);
    const int W = (NL > 0 || batched) ? 1 : (X > 0 ? a.groups : (int)gridDim.x);
    if (X > 0 && wg >= W) return;
    const size_t sys = batched ? blockIdx.x : 0;
    const size_t msys = a.rhs > 1 ? sys / (size_t)a.rhs : sys;      // whose S / Pinv / Ginv / C_dense: rhs consecutive workgroups share one system's
    const int K = a.K;
    // this launch's knot range: the whole system, or this rank's shard of it (MR)
    const int k_begin = MR ? a.k_begin : 0, k_end = MR ? a.k_end : K;
    const int R = MR ? a.nranks : 1;
    const int k0 = k_begin + wg * a.knots_per_wg;
    const int nk = min(a.knots_per_wg, k_end - k0);
    const int jl = tid / LPK;              // the lane's slot
    const int r_ = tid - jl * LPK;         // row inside the knot (DR: rows S..LPK-1 do not exist, those lanes idle)
    const int n_res = NR ? 0 : (XR > 0 ? min(nk, (int)blockDim.x / S) : nk);    // knots with lanes of their own
    const int n_ext = nk - n_res;                                    // knots handled as extra rows (XR > 0 only)
    const int j = (XR > 0 && !NR && n_ext > 0 && jl == n_res - 1) ? nk - 1 : jl;   // local knot: the last slot holds the LAST knot
    const bool active = jl < n_res && (!DR || r_ < S);
    const int xk = NR ? 0 : n_res - 1;                               // first local knot of the extra rows
    // extra rows of this lane: rows q = tid + e * blockDim.x (e < ne) of the knots [xk, xk + n_ext)
    const int n_ext_rows = n_ext * S;
    const int ne = XR > 0 ? (n_ext_rows + (int)blockDim.x - 1) / (int)blockDim.x : 0;      // workgroup-uniform trip count
    __shared__ T xst[2][XR > 0 ? XR * MAXT : 1];                                            // [lambda | product][row]; r, p: the windows
    const int k = k0 + j;
    const bool has_left = k0 > 0;          // a neighbouring block row exists in the SYSTEM ...
    const bool has_right = k0 + nk < K;
    const bool loc_left = MR ? wg > 0 : has_left;            // ... and it belongs to a workgroup of this launch,
    const bool loc_right = MR ? wg < W - 1 : has_right;
    const bool x_left = MR && wg == 0 && has_left;           // or to the neighbouring rank (another GPU)
    const bool x_right = MR && wg == W - 1 && has_right;
    const bool multi = W > 1 || (MR && R > 1);               // ghost blocks exist and travel through the hand-off

    const T *__restrict__ dS = static_cast<const T *>(a.S_bd) + msys * 3 * S * S * K;
    const T *__restrict__ dP = static_cast<const T *>(a.P_bd) + msys * 3 * S * S * K;
    const T *__restrict__ dG = static_cast<const T *>(a.gamma) + sys * S * K;
    T *__restrict__ dL = static_cast<T *>(a.lambda) + sys * S * K;

    // ---- load this lane's rows of S and Pinv into registers (once per solve) ----------------
    // bd layout: block-row k = [left|main|right], each S*S column-major -> element (r, c) of the
    // S x 3S strip sits at c*S + r (gato_utils.cuh:53-54,97-98).  First/last block rows have no
    // left/right block (gato_utils.cuh:157-174): those entries are forced to zero here.
    T sm[NR ? 1 : 3 * S], pm[NR ? 1 : NREG];
    if constexpr (!NR) {
        const size_t base = (size_t)(active ? k : 0) * 3 * S * S + r_;
#pragma unroll
        for (int c = 0; c < 3 * S; ++c) {
            const bool ok = active && !(k == 0 && c < S) && !(k == K - 1 && c >= 2 * S);
            sm[c] = ok ? dS[base + (size_t)c * S] : (T)0;
            const T pv_ = ok ? dP[base + (size_t)c * S] : (T)0;
            if (c < NREG) pm[c < NREG ? c : 0] = pv_;
            else ptail[(c - NREG) / VecOf<T>::W][tid][(c - NREG) % VecOf<T>::W] = pv_;   // own lane only: no barrier
        }
        // (issuing all 6S loads first and selecting afterwards - what pays in the one-workgroup kernels of gato_pcg_resident_single.hip - measured no
        //  better here: 14/7/1024 f32 2.34 -> 2.31 but 14/7/4096 f32 3.44 -> 3.53, 32/16/256 2.53 -> 2.62 us per iteration)
    }

    // ---- hand-off area ----------------------------------------------------------------------
    const int slotG = pcg_slot_granules(S, (int)sizeof(T));
    gu64 *slots = (gu64 *)a.slots;
    gi32 *g_status = (gi32 *)a.status;
    const unsigned long long t_limit = a.timeout_ticks;
    // cross-GPU mirror (MR): granules per parity, ghost block offsets
    const int xslotG = pcg_xslot_granules(S, (int)sizeof(T));
    const int xghL = 16 * GATO_MAX_RANKS, xghR = xghL + pcg_xghost_granules(S, (int)sizeof(T));
    unsigned xepoch = MR ? a.xepoch0 : 0u;
    // mirrors of the peers, read once from the device table: the neighbouring ranks' (edge blocks) and, in lane r of
    // wave 0 of workgroup 0, rank r's (the rank total goes to every rank)
    gu64 *xp_prev = nullptr, *xp_next = nullptr;
    __shared__ unsigned long long s_xpeer[MR ? GATO_MAX_RANKS : 1];      // the peers' mirrors: lane r of wave 0 fetches rank r's at each hand-off
    if constexpr (MR) {
        if (a.rank > 0) xp_prev = (gu64 *)a.xpeer[a.rank - 1];
        if (a.rank < R - 1) xp_next = (gu64 *)a.xpeer[a.rank + 1];
        if (wave == 0 && lane < R) s_xpeer[lane] = (unsigned long long)a.xpeer[lane];   // read back by the same lanes only
    }

    if (tid == 0) s_abort = 0;     // the status word is never cleared here: the host matches launch ids (gato_pcg_status)
    // test hook, diagnostic build only (options stamp_pcg + ablate = 16): the last workgroup never shows up, as if it
    // had not been scheduled - the others must give up after the time-out and report it
    if (ABL && (a.ablate & 16) && W > 1 && wg == W - 1) return;
    for (int i = tid; i < 2 * (MAXKX + 2) * SP; i += blockDim.x) (&xs[0][0])[i] = (T)0;
    __syncthreads();

    // r = gamma, lambda = 0 (gato_pcg.cuh:300-304); ghost r read straight from gamma.
    T lam = (T)0;
    T r = active ? dG[(size_t)k * S + r_] : (T)0;
    T p = (T)0, ups, rt;
#pragma unroll 1
    for (int e = 0; e < ne; ++e) {
        const int q = tid + e * (int)blockDim.x;
        if (q < n_ext_rows) {
            const int jx = xk + q / S, rx = q % S;
            const T g_ = dG[(size_t)(k0 + jx) * S + rx];
            xst[0][q] = (T)0; xst[1][q] = (T)0;
            xs[1][(jx + 1) * SP + rx] = g_;
        }
    }
    // product = M x on the extra rows (x = window w: 0 = p, 1 = r); returns this lane's share of x . (M x)
    auto extra_rows = [&](const T *__restrict__ M, int w) -> T {
        T dot = (T)0;
        if constexpr (NR && S % 2 == 0) {
            // No resident rows: a lane takes TWO adjacent rows of a knot per trip.  Element (r, c) of a block row sits at
            // c*S + r, so the pair (r, r+1) of a column is ONE 8-byte (f32) / 16-byte (f64) load: half the load
            // instructions and half the L1 sector accesses per byte (the 4-byte-per-lane form keeps the L1 at 83 % of
            // its 64 B/clk - DESIGN.md 3.1), and both rows share the operand-window reads (packed FMAs in f32).
            typedef T T2 __attribute__((ext_vector_type(2)));
            typedef typename VecOf<T>::type V;
            constexpr int VW = VecOf<T>::W, H = S / 2;
            const int n_pairs = n_ext * H;
            const int ne2 = (n_pairs + (int)blockDim.x - 1) / (int)blockDim.x;
#pragma unroll 1
            for (int e = 0; e < ne2; ++e) {
                const int qp = tid + e * (int)blockDim.x;
                const bool on = qp < n_pairs;
                const int qq = on ? qp : 0;
                const int jx = xk + qq / H, r0 = 2 * (qq % H);
                const T *__restrict__ src = M + (size_t)(k0 + jx) * 3 * S * S + r0;
                T2 m[3 * S];
#pragma unroll
                for (int c = 0; c < 3 * S; ++c) m[c] = *reinterpret_cast<const T2 *>(src + (size_t)c * S);
                const bool nl = k0 + jx == 0, nr = k0 + jx == K - 1;        // first / last block row of the system
#pragma unroll
                for (int c = 0; c < S; ++c) {
                    if (nl) m[c] = T2{(T)0, (T)0};
                    if (nr) m[2 * S + c] = T2{(T)0, (T)0};
                }
                const T *xw = &xs[w][jx * SP];
                T2 acc = {(T)0, (T)0};
#pragma unroll
                for (int b = 0; b < 3; ++b) {
#pragma unroll
                    for (int i = 0; i < SP / VW; ++i) {
                        const V v = *reinterpret_cast<const V *>(xw + b * SP + i * VW);
#pragma unroll
                        for (int e2 = 0; e2 < VW; ++e2)
                            if (i * VW + e2 < S) acc = __builtin_elementwise_fma(m[b * S + i * VW + e2], T2{v[e2], v[e2]}, acc);
                    }
                }
                if (on) {
                    const int q0 = (jx - xk) * S + r0;
                    xst[1][q0] = acc[0];
                    xst[1][q0 + 1] = acc[1];
                    dot = gato::fmaT(xw[SP + r0], acc[0], dot);
                    dot = gato::fmaT(xw[SP + r0 + 1], acc[1], dot);
                }
            }
            return dot;
        }
#pragma unroll 1
        for (int e = 0; e < ne; ++e) {
            const int q = tid + e * (int)blockDim.x;
            const bool on = q < n_ext_rows;
            const int qq = on ? q : 0;                                      // lanes without a row here read row 0
            const int jx = xk + qq / S, rx = qq % S;
            const T y = row_from_memory<T, S, SP>(M + (size_t)(k0 + jx) * 3 * S * S + rx, &xs[w][jx * SP],
                                                  NR && k0 + jx == 0, NR && k0 + jx == K - 1);
            if (on) {
                xst[1][q] = y;
                dot = gato::fmaT(xs[w][(jx + 1) * SP + rx], y, dot);
            }
        }
        return dot;
    };
    if (active) xs[1][(j + 1) * SP + r_] = r;
    if (tid < S) {
        if (has_left) xs[1][tid] = dG[(size_t)(k0 - 1) * S + tid];
    } else if (tid < 2 * S) {
        if (has_right) xs[1][(nk + 1) * SP + (tid - S)] = dG[(size_t)(k0 + nk) * S + (tid - S)];
    }
    __syncthreads();

    T g_r_init = (T)0;
    if constexpr (RG) {                     // ghost r starts as the neighbours' gamma blocks (just written to the window)
        if (wave == 0 && (lane < S || (lane >= 32 && lane < 32 + S))) g_r_init = xs[1][lane < 32 ? lane : (nk + 1) * SP + (lane - 32)];
    }
    unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t_prev = 0, t_begin = 0, rt_begin = 0;
    if (STAMP) {
        t_begin = t_prev = __builtin_amdgcn_s_memtime();
        rt_begin = __builtin_amdgcn_s_memrealtime();
    }
    unsigned epoch = a.epoch0;
    T eta = (T)0, eta_new = (T)0;
    int iters = a.max_iters;
    const T tol = (T)a.exit_tol;
    bool aborted = false;

    // One reduction + halo exchange.  `val` = the vector just produced (upsilon or r~), `prod` the
    // lane's dot contribution.  On return: total in every thread; gh[][] = neighbours' boundary
    // blocks of `val` (zeros where there is no neighbour).
    const int abl = ABL ? a.ablate : 0;   // diagnostic timing-only switches, compiled out of the production build
    // One-XCD launches (xcd_pack): once the workgroups have verified - below, with agent-scope granules - that they really all
    // sit on ONE XCD, the hand-off granules are stored with WORKGROUP scope: they stay in that XCD's L2 (its CUs' sc1 loads see
    // them there) instead of being written through to memory.  A placement that is not what the launch hoped for (the
    // dispatcher is free to place blocks anywhere) just keeps the agent-scope stores.
    bool fast_st = false;
    auto gstore = [&](gu64 *g, unsigned ep, T v) {
        if (fast_st) LGr::store(g, ep, v);
        else Gr::store(g, ep, v);
    };
    // WP: the ghost blocks of r and p and the boundary entry just gathered, in the polling lanes' registers
    T hv_reg = (T)0, g_r = g_r_init, g_p = (T)0;
    const bool g_lane = RG && wave == 0 && (lane < S || (lane >= 32 && lane < 32 + S));
    const int gslot = lane < 32 ? lane : (nk + 1) * SP + (lane - 32);      // the lane's ghost entry in an operand window
    auto allreduce_and_halo = [&](T val, T prod, T &total) {
        ++epoch;
        if constexpr (MR) ++xepoch;
        if (abl & 4) { total = (T)1 + prod * (T)1e-30; return; }
        if (aborted) { total = (T)0; return; }             // the placement round below already timed out: no second wait
        T *wp = wpart[epoch & 1];
        gu64 *mine = slots + ((size_t)(epoch & 1) * W + wg) * slotG;
        if constexpr (WP) {
            if (W > 1) {
                const T ws = wave_sum(prod);
                if (lane == 0) gstore(mine + wave * GPV, epoch, ws);
            } else partials_store(wp, wave, lane, prod);      // one workgroup per rank (cluster): its total comes from LDS
        } else partials_store(wp, wave, lane, prod);
        if (!NR && W > 1 && active) {
            if (j == 0) gstore(mine + 16 + r_ * GPV, epoch, val);
            if (j == nk - 1) gstore(mine + 16 + (S + r_) * GPV, epoch, val);
        }
        if constexpr (MR && !NR) {          // the rank's edge blocks go straight into the neighbouring GPU's mirror
            if (active) {
                if (x_left && j == 0) XGr::store(xp_prev + (size_t)(xepoch & 1) * xslotG + xghR + r_ * GPV, xepoch, val);
                if (x_right && j == nk - 1) XGr::store(xp_next + (size_t)(xepoch & 1) * xslotG + xghL + r_ * GPV, xepoch, val);
            }
        }
        if (!WP || W == 1) __syncthreads();                                    // B1
        if constexpr (NR) {                 // boundary blocks of the vector just formed: from the product array (complete after B1)
            if (W > 1) {
                if (tid < S) gstore(mine + 16 + tid * GPV, epoch, xst[1][tid]);
                else if (tid < 2 * S) gstore(mine + 16 + tid * GPV, epoch, xst[1][(nk - 1) * S + (tid - S)]);
            }
            if constexpr (MR) {
                if (x_left && tid < S) XGr::store(xp_prev + (size_t)(xepoch & 1) * xslotG + xghR + tid * GPV, xepoch, xst[1][tid]);
                if (x_right && tid >= S && tid < 2 * S)
                    XGr::store(xp_next + (size_t)(xepoch & 1) * xslotG + xghL + (tid - S) * GPV, xepoch, xst[1][(nk - 1) * S + (tid - S)]);
            }
        }
        if (W == 1 && !(MR && R > 1)) {
            // one workgroup: every wave sums the per-wave partials itself (fixed order), no second barrier
            // (one LDS read per lane + a DPP sum: a serial loop over the partials would pay one LDS
            //  round trip per wave)
            total = partials_total<T, (MAXT <= 512 ? 8 : 16)>(wp, nwaves, lane);
            return;
        }
        if (wave == 0) {
            T tot = (T)0;
            if (!WP || W == 1) tot = partials_total<T, (MAXT <= 512 ? 8 : 16)>(wp, nwaves, lane);
            bool fail = false;
            if (W > 1) {
                if constexpr (!WP) {
                    if (lane == 0) gstore(mine, epoch, tot);
                }
                // sweep: partials of all workgroups + neighbours' halo blocks.  Every lane issues ALL its loads
                // back to back from clamped (always valid) addresses and waits once: predicated loads would each
                // get their own s_waitcnt, i.e. one L2 round trip after the other.
                gu64 *pbase = slots + (size_t)(epoch & 1) * W * slotG;
                // The per-lane addresses are re-derived from the lane id at every hand-off, behind an empty asm the compiler
                // cannot see through: as loop invariants it computes them once for both parities, runs out of registers
                // and re-loads them from scratch at the head of every hand-off (a memory round trip on the critical path).
                int ln = lane;
                asm volatile("" : "+v"(ln));
                const bool want_l = loc_left && ln < S;
                const bool want_r = loc_right && ln >= 32 && ln < 32 + S;
                gu64 *hptr = want_l ? pbase + (size_t)(wg - 1) * slotG + 16 + (S + ln) * GPV
                           : want_r ? pbase + (size_t)(wg + 1) * slotG + 16 + (ln - 32) * GPV
                                    : mine;
                // gathered form: entry e = workgroup e's total.  WP: entry e = wave (e & mask) of workgroup (e >> wsh); entries of
                // waves that do not exist read the workgroup's wave 0 and count as zero
                constexpr int PMX = WP ? WPM : Cfg::PM;
                gu64 *pptr[PMX];
                int pm_count = (W + 63) >> 6;                 // wave-uniform
                int wsh = 0;
                if constexpr (WP) {
                    wsh = nwaves <= 1 ? 0 : 32 - __builtin_clz((unsigned)(nwaves - 1));
                    pm_count = ((W << wsh) + 63) >> 6;
                }
#pragma unroll
                for (int m = 0; m < PMX; ++m) {
                    if constexpr (WP) {
                        const int e = ln + 64 * m, wi = e >> wsh, wv = e & ((1 << wsh) - 1);
                        pptr[m] = pbase + (size_t)min(wi, W - 1) * slotG + (wv < nwaves ? wv : 0) * GPV;
                    } else pptr[m] = pbase + (size_t)min(ln + 64 * m, W - 1) * slotG;
                }
                unsigned long long raw[PMX][GPV], hraw[GPV];
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                // Cross-XCD launches: the first poll can never hit (the publishers' stores need a fabric round
                // trip), and W*W early loads only queue in front of those stores.  ~0.35 us of sleep before the
                // first poll measured -5..-10 % per iteration for W > 32 and +6 % for one-XCD launches.
                if (W > 64) __builtin_amdgcn_s_sleep(12);
                else if (W > 32) __builtin_amdgcn_s_sleep(10);      // round 3 sweep: 32/16/1024 (W = 64) 10: 4.22 / 12: 4.32 us, 14/7/2048 (W = 57) 3.51 / 3.61
                for (unsigned spin = 0;; ++spin) {
#pragma unroll
                    for (int m = 0; m < PMX; ++m) {
                        if (m < pm_count) {
#pragma unroll
                            for (int g = 0; g < GPV; ++g)
                                raw[m][g] = __hip_atomic_load(pptr[m] + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
#pragma unroll
                    for (int g = 0; g < GPV; ++g)
                        hraw[g] = __hip_atomic_load(hptr + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    bool ok = true;
#pragma unroll
                    for (int m = 0; m < PMX; ++m) {
                        if (m < pm_count) {
#pragma unroll
                            for (int g = 0; g < GPV; ++g) ok &= (unsigned)(raw[m][g] >> 32) == epoch;
                        }
                    }
#pragma unroll
                    for (int g = 0; g < GPV; ++g) ok &= (unsigned)(hraw[g] >> 32) == epoch;   // own slot: always current
                    if (__all(ok)) break;
                    if ((spin & 255u) == 255u) {
                        const bool late = __builtin_amdgcn_s_memrealtime() - t0 > t_limit;
                        const bool other = __hip_atomic_load(g_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
                        if (late || other) { fail = true; break; }
                    }
                }
                T pv[PMX];
#pragma unroll
                for (int m = 0; m < PMX; ++m) {
                    bool on = m < pm_count && lane + 64 * m < W;
                    if constexpr (WP) {
                        const int e = lane + 64 * m;
                        on = m < pm_count && (e >> wsh) < W && (e & ((1 << wsh) - 1)) < nwaves;
                    }
                    pv[m] = on ? Gr::decode(raw[m]) : (T)0;
                }
                const T hv = Gr::decode(hraw);
                T acc = (T)0;
#pragma unroll
                for (int m = 0; m < PMX; ++m) acc += pv[m];
                tot = wave_sum(acc);
                if constexpr (RG) hv_reg = (want_l || want_r) ? hv : (T)0;
                else {
                    if (lane < S) gh[0][lane] = want_l ? hv : (T)0;
                    if (lane >= 32 && lane < 32 + S) gh[1][lane - 32] = want_r ? hv : (T)0;
                }
            } else {                       // one workgroup on this GPU (cluster launch): the ghosts come from level 2 only
                if constexpr (RG) hv_reg = (T)0;
                else {
                    if (lane < S) gh[0][lane] = (T)0;
                    if (lane >= 32 && lane < 32 + S) gh[1][lane - 32] = (T)0;
                }
            }
            if constexpr (MR) {
                if (R > 1 && !fail) {
                    // ---- level 2: across the GPUs of the node.  tot = this rank's total (identical in all its workgroups)
                    const size_t xo = (size_t)(xepoch & 1) * xslotG;
                    if (wg == 0 && lane < R) XGr::store((gu64 *)s_xpeer[lane] + xo + a.rank * 16, xepoch, tot);
                    gu64 *xl = (gu64 *)a.xslots + xo;                     // polls stay on THIS GPU's memory
                    int l2 = lane;
                    asm volatile("" : "+v"(l2));
                    const bool xw_l = x_left && l2 < S;
                    const bool xw_r = x_right && l2 >= 32 && l2 < 32 + S;
                    gu64 *tptr = xl + (size_t)min(l2, R - 1) * 16;
                    gu64 *xhp = xw_l ? xl + xghL + l2 * GPV : xw_r ? xl + xghR + (l2 - 32) * GPV : tptr;
                    unsigned long long traw[GPV], xraw[GPV];
                    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                    for (unsigned spin = 0;; ++spin) {
#pragma unroll
                        for (int g = 0; g < GPV; ++g) {
                            traw[g] = __hip_atomic_load(tptr + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            xraw[g] = __hip_atomic_load(xhp + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                        bool ok = true;
#pragma unroll
                        for (int g = 0; g < GPV; ++g) ok &= (unsigned)(traw[g] >> 32) == xepoch && (unsigned)(xraw[g] >> 32) == xepoch;
                        if (__all(ok)) break;
                        if ((spin & 255u) == 255u) {
                            const bool late = __builtin_amdgcn_s_memrealtime() - t0 > t_limit;
                            const bool other = __hip_atomic_load(g_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
                            if (late || other) { fail = true; break; }
                        }
                    }
                    tot = partials_sum(lane < R ? XGr::decode(traw) : (T)0);     // rank order, the same tree on every GPU
                    const T xv = XGr::decode(xraw);
                    if constexpr (RG) {
                        if (xw_l || xw_r) hv_reg = xv;
                    } else {
                        if (xw_l) gh[0][lane] = xv;
                        if (xw_r) gh[1][lane - 32] = xv;
                    }
                }
            }
            if (fail) {
                if (lane == 0) {
                    __hip_atomic_store(g_status, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_abort = 1;
                }
            }
            if (lane == 0) bc[epoch & 1] = tot;
        }
        __syncthreads();                                                       // B2
        total = bc[epoch & 1];
        aborted = s_abort != 0;
    };

    // Flat cluster exchange (MR, a.flat): ONE level across the node.  Every workgroup of every rank has a slot in every
    // mirror (global workgroup index gw = a.flat_base + wg of a.flat_groups); it stores its partial into ALL mirrors (lane r
    // -> rank r) and its boundary blocks into its own GPU's mirror and, at the rank's edges, the neighbour's; wave 0 polls
    // the partials of all workgroups and its two neighbours' blocks in ITS OWN GPU's mirror.  Same sum order on every
    // workgroup of every rank.  Against the two-level form this saves the wait for the rank's own gather before anything
    // crosses the fabric (a hand-off costs one fabric store + one poll instead of level 1 + that).
    auto allreduce_flat = [&](T val, T prod, T &total) {
        if constexpr (MR) {
            ++epoch; ++xepoch;
            T *wp = wpart[xepoch & 1];
            partials_store(wp, wave, lane, prod);
            const int WT = a.flat_groups, gw = a.flat_base + wg;
            const size_t so = a.flat_off + ((size_t)(xepoch & 1) * WT + gw) * slotG;       // this workgroup's slot in a mirror
            gu64 *fl = (gu64 *)a.xslots;
            if (!NR && active) {
                if (j == 0) {
                    XGr::store(fl + so + 16 + r_ * GPV, xepoch, val);
                    if (x_left) XGr::store(xp_prev + so + 16 + r_ * GPV, xepoch, val);
                }
                if (j == nk - 1) {
                    XGr::store(fl + so + 16 + (S + r_) * GPV, xepoch, val);
                    if (x_right) XGr::store(xp_next + so + 16 + (S + r_) * GPV, xepoch, val);
                }
            }
            __syncthreads();                                                   // B1
            if constexpr (NR) {
                if (tid < 2 * S) {
                    const T v2 = tid < S ? xst[1][tid] : xst[1][(nk - 1) * S + (tid - S)];
                    XGr::store(fl + so + 16 + tid * GPV, xepoch, v2);
                    if (tid < S && x_left) XGr::store(xp_prev + so + 16 + tid * GPV, xepoch, v2);
                    if (tid >= S && x_right) XGr::store(xp_next + so + 16 + tid * GPV, xepoch, v2);
                }
            }
            if (wave == 0) {
                T tot = partials_total<T, (MAXT <= 512 ? 8 : 16)>(wp, nwaves, lane);
                if (lane < R) XGr::store((gu64 *)s_xpeer[lane] + so, xepoch, tot);   // the partial goes into EVERY mirror
                gu64 *pbase = fl + a.flat_off + (size_t)(xepoch & 1) * WT * slotG;
                int ln = lane;                                 // re-derived at every hand-off (see allreduce_and_halo)
                asm volatile("" : "+v"(ln));
                const bool want_l = has_left && ln < S;
                const bool want_r = has_right && ln >= 32 && ln < 32 + S;
                gu64 *hptr = want_l ? pbase + (size_t)(gw - 1) * slotG + 16 + (S + ln) * GPV
                           : want_r ? pbase + (size_t)(gw + 1) * slotG + 16 + (ln - 32) * GPV
                                    : pbase + (size_t)gw * slotG;
                gu64 *pptr[Cfg::PM];
#pragma unroll
                for (int m = 0; m < Cfg::PM; ++m) pptr[m] = pbase + (size_t)min(ln + 64 * m, WT - 1) * slotG;
                const int pm_count = (WT + 63) >> 6;
                unsigned long long raw[Cfg::PM][GPV], hraw[GPV];
                // sleep before the first sweep as in the single-GPU launches (l_sleep below): the partials of WT workgroups cross
                // the XCDs' fabric at least; across GPUs the peers' stores take longer still
                if (WT > 32) {
                    const int sl = 10 + WT / 22;
                    for (int i = 0; i < sl; ++i) __builtin_amdgcn_s_sleep(1);
                }
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                bool fail = false;
                for (unsigned spin = 0;; ++spin) {
#pragma unroll
                    for (int m = 0; m < Cfg::PM; ++m) {
                        if (m < pm_count) {
#pragma unroll
                            for (int g = 0; g < GPV; ++g)
                                raw[m][g] = __hip_atomic_load(pptr[m] + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                    }
#pragma unroll
                    for (int g = 0; g < GPV; ++g) hraw[g] = __hip_atomic_load(hptr + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    bool ok = true;
#pragma unroll
                    for (int m = 0; m < Cfg::PM; ++m) {
                        if (m < pm_count) {
#pragma unroll
                            for (int g = 0; g < GPV; ++g) ok &= (unsigned)(raw[m][g] >> 32) == xepoch;
                        }
                    }
#pragma unroll
                    for (int g = 0; g < GPV; ++g) ok &= (unsigned)(hraw[g] >> 32) == xepoch;
                    if (__all(ok)) break;
                    if ((spin & 255u) == 255u) {
                        const bool late = __builtin_amdgcn_s_memrealtime() - t0 > t_limit;
                        const bool other = __hip_atomic_load(g_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
                        if (late || other) { fail = true; break; }
                    }
                }
                T acc = (T)0;
#pragma unroll
                for (int m = 0; m < Cfg::PM; ++m)
                    acc += (m < pm_count && lane + 64 * m < WT) ? XGr::decode(raw[m]) : (T)0;
                const T hv = XGr::decode(hraw);
                tot = wave_sum(acc);
                if constexpr (RG) hv_reg = (want_l || want_r) ? hv : (T)0;
                else {
                    if (lane < S) gh[0][lane] = want_l ? hv : (T)0;
                    if (lane >= 32 && lane < 32 + S) gh[1][lane - 32] = want_r ? hv : (T)0;
                }
                if (fail && lane == 0) {
                    __hip_atomic_store(g_status, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_abort = 1;
                }
                if (lane == 0) bc[xepoch & 1] = tot;
            }
            __syncthreads();                                                   // B2
            total = bc[xepoch & 1];
            aborted = s_abort != 0;
        }
    };
    // ---- LEAN hand-off: the plain single-GPU launches (RG forms).  Same protocol and same arithmetic as allreduce_and_halo,
    // with everything that does not change between hand-offs computed ONCE: per-lane 32-bit BYTE offsets inside a parity block
    // of the hand-off area (stores and loads take the uniform block base in SGPRs plus that offset - no 64-bit address
    // arithmetic per hand-off; the loads of one sweep differ by a uniform stride, so they share ONE offset register), the
    // predicates of the storing / decoding lanes, and the poll instantiated per number of loads.  FAST (workgroup-scope stores,
    // one-XCD launches that verified their placement) is a compile-time argument: the iteration loop exists twice instead of
    // branching at every store.  The stamps of a diagnostic build said why: of a hand-off's ~2 300 cycles at 15 workgroups
    // the poll itself was 970, the rest address arithmetic, scalar branches and two wave sums in the polling wave.
    constexpr bool LEAN = RG && !MR;
    // KEEP: the polling lanes' load offsets stay in registers for the whole solve; kernels whose matrix rows leave few registers
    // (fp64 at S = 14, fp32 at S = 32, the 768-thread bound) re-derive them from the lane id at every hand-off instead (a
    // dozen vector instructions in the polling wave; spilling them costs a memory round trip on the critical path)
    constexpr int REGCAP = MAXT <= 256 ? 512 : MAXT <= 512 ? 256 : MAXT <= 768 ? 168 : 128;
    constexpr bool KEEP = REGCAP - 6 * S * (int)(sizeof(T) / 4) >= 120;
    const int l_wsh = WP ? (nwaves <= 1 ? 0 : 32 - __builtin_clz((unsigned)(nwaves - 1))) : 0;
    const unsigned l_slotB = (unsigned)slotG * 8u;
    const unsigned l_st_part = (unsigned)wg * l_slotB + (WP ? (unsigned)__builtin_amdgcn_readfirstlane(wave) * (unsigned)GPV * 8u : 0u);   // uniform
    const unsigned l_st_halo = (unsigned)wg * l_slotB + (16u + (unsigned)r_ * (unsigned)GPV) * 8u;     // first block; the last block S values further
    const bool l_hl = LEAN && active && j == 0, l_hr = LEAN && active && j == nk - 1;
    // poll entry e = lane + 64 m: gathered form = workgroup e; WP = wave (e & mask) of workgroup (e >> wsh).  64 entries are a
    // whole number of workgroups, so load m reads at the lane's offset of load 0 plus m uniform strides.  Entries beyond the
    // launch read this workgroup's own granule instead (the other parity's block follows this one: its lines are being written)
    // and are masked out of the epoch test and of the sum.
    struct LeanLd { int wi0, wv0; unsigned part, halo; bool want_l, want_r; };
    auto l_derive = [&](int ln) {
        LeanLd d;
        d.wi0 = ln >> l_wsh; d.wv0 = ln & ((1 << l_wsh) - 1);
        d.part = (unsigned)d.wi0 * l_slotB + (unsigned)d.wv0 * (unsigned)GPV * 8u;
        d.want_l = loc_left && ln < S; d.want_r = loc_right && ln >= 32 && ln < 32 + S;
        d.halo = d.want_l ? (unsigned)(wg - 1) * l_slotB + (16u + (unsigned)(S + ln) * (unsigned)GPV) * 8u
               : d.want_r ? (unsigned)(wg + 1) * l_slotB + (16u + (unsigned)(ln - 32) * (unsigned)GPV) * 8u
                          : (unsigned)wg * l_slotB;                        // wave 0's own partial granule: always current
        return d;
    };
    const LeanLd l_kept = l_derive(lane);
    const unsigned l_ld_step = (unsigned)(64 >> l_wsh) * l_slotB;
    const int l_pm = ((W << l_wsh) + 63) >> 6;
    typedef __attribute__((address_space(1))) char gchar;
    auto l_at = [](gu64 *base, unsigned boff) { return (gu64 *)((gchar *)base + boff); };
    // one sweep of N loads per lane until every granule watched carries the epoch; false = gave up (time-out / another
    // workgroup reported one)
    // (returns the lane's sum of the partials it read - in load order, as allreduce_and_halo - and its halo entry)
    // Sleep before the first sweep (launches across XCDs; gathered form), in units of ~74 cycles (s_sleep 1 + the loop).  A
    // sweep that comes before the last publisher's store has crossed the fabric is wasted and the next one costs a whole
    // round trip more; a sweep that comes late wastes the difference.  Swept with this hand-off (tools/sleep_sweep.py on a scratch
    // build; us per iteration): 14/7/4096 f32 (W = 114) 12: 3.64, 14: 3.56, 16: 3.40, 18: 3.46; 14/7/2048 f32 (57) 12: 3.25,
    // 14: 3.13, 16: 3.22; 14/7/4096 f64 (128) 12: 4.40, 14: 4.18, 16: 4.24; 32/16/1024 f32 (64) 10: 3.71, 12: 3.60, 14: 3.69;
    // 32/16/2048 f32 (128) 12: 4.20, 14: 4.01, 16: 4.09 - the optimum grows with the number of workgroups (their skew).  A
    // controller in the polling wave (failed first sweep -> longer, a run of successes -> shorter) was tried and lost: one
    // workgroup's probe that fails delays everybody's next hand-off, so 114 independent probes keep the whole launch inflated
    // (3.58 against 3.40 with the fixed value).
    const int l_sleep = W > 32 ? 10 + W / 22 : 0;
    auto l_poll = [&](auto nc, const LeanLd &d, gu64 *pb, T &acc_out, T &hv_out) -> bool {
        constexpr int N = decltype(nc)::value;
        const unsigned l_ld_part = d.part, l_ld_halo = d.halo;
        unsigned long long raw[N][GPV], hraw[GPV];
        bool valid[N];
#pragma unroll
        for (int m = 0; m < N; ++m) valid[m] = d.wi0 + m * (64 >> l_wsh) < W && d.wv0 < nwaves;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (unsigned spin = 0;; ++spin) {
#pragma unroll
            for (int m = 0; m < N; ++m) {
                gu64 *pm = l_at(pb, valid[m] ? l_ld_part + (unsigned)m * l_ld_step : (unsigned)wg * l_slotB);
#pragma unroll
                for (int g = 0; g < GPV; ++g) raw[m][g] = __hip_atomic_load(pm + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            gu64 *ph = l_at(pb, l_ld_halo);
#pragma unroll
            for (int g = 0; g < GPV; ++g) hraw[g] = __hip_atomic_load(ph + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool ok = true;
#pragma unroll
            for (int m = 0; m < N; ++m) {
                bool okm = true;
#pragma unroll
                for (int g = 0; g < GPV; ++g) okm &= (unsigned)(raw[m][g] >> 32) == epoch;
                ok &= okm | !valid[m];
            }
#pragma unroll
            for (int g = 0; g < GPV; ++g) ok &= (unsigned)(hraw[g] >> 32) == epoch;
            bool stop = __all(ok), good = stop;
            if (!stop && (spin & 255u) == 255u) {
                const bool late = __builtin_amdgcn_s_memrealtime() - t0 > t_limit;
                const bool other = __hip_atomic_load(g_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
                stop = late || other;
            }
            if (stop) {
                T acc = (T)0;
#pragma unroll
                for (int m = 0; m < N; ++m) acc += valid[m] ? Gr::decode(raw[m]) : (T)0;
                acc_out = acc;
                hv_out = Gr::decode(hraw);
                return good;
            }
        }
    };
    auto handoff_lean = [&](auto fastc, T val, T prod, T &total) {
        constexpr bool FAST = decltype(fastc)::value;
        typedef typename std::conditional<FAST, LGr, Gr>::type SG;
        ++epoch;
        if constexpr (ABL) {
            if (abl & 4) { total = (T)1 + prod * (T)1e-30; return; }
        }
        if (aborted) { total = (T)0; return; }
        gu64 *pb = slots + (size_t)(epoch & 1) * W * slotG;                       // this parity's block (uniform)
        T *wp = wpart[epoch & 1];
        if constexpr (WP) {
            const T ws = wave_sum(prod);
            if (lane == 0) SG::store(l_at(pb, l_st_part), epoch, ws);
        } else partials_store(wp, wave, lane, prod);
        if (l_hl) SG::store(l_at(pb, l_st_halo), epoch, val);
        if (l_hr) SG::store(l_at(pb, l_st_halo + (unsigned)(S * GPV * 8)), epoch, val);
        if constexpr (!WP) __syncthreads();                                        // B1
        if (wave == 0) {
            if constexpr (!WP) {
                const T mine_tot = partials_total<T, (MAXT <= 512 ? 8 : 16)>(wp, nwaves, lane);
                if (lane == 0) SG::store(l_at(pb, l_st_part), epoch, mine_tot);
            }
            if constexpr (!WP) {
                for (int i = 0; i < l_sleep; ++i) __builtin_amdgcn_s_sleep(1);
            }
            LeanLd d = l_kept;
            if constexpr (!KEEP) {                   // re-derived behind an empty asm the compiler cannot hoist out of the loop
                int ln = lane;
                asm volatile("" : "+v"(ln));
                d = l_derive(ln);
            }
            bool done;
            T acc, hv;
            if (l_pm == 1) done = l_poll(std::integral_constant<int, 1>{}, d, pb, acc, hv);
            else if (l_pm == 2) done = l_poll(std::integral_constant<int, 2>{}, d, pb, acc, hv);
            else if (l_pm == 3) done = l_poll(std::integral_constant<int, 3>{}, d, pb, acc, hv);
            else done = l_poll(std::integral_constant<int, 4>{}, d, pb, acc, hv);
            const T tot = wave_sum(acc);
            hv_reg = (d.want_l || d.want_r) ? hv : (T)0;
            if (lane == 0) {
                if (!done) {
                    __hip_atomic_store(g_status, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_abort = 1;
                }
                bc[epoch & 1] = tot;
            }
        }
        __syncthreads();                                                           // B2
        total = bc[epoch & 1];
        aborted = s_abort != 0;
    };
    const bool flat = MR && a.flat != 0;
    auto exchange = [&](auto fastc, T val, T prod, T &total) {
        if constexpr (LEAN) handoff_lean(fastc, val, prod, total);
        else if (flat) allreduce_flat(val, prod, total);
        else allreduce_and_halo(val, prod, total);
    };
    // outside the iteration loop: the store scope as a run-time choice
    auto exchange_rt = [&](T val, T prod, T &total) {
        if constexpr (LEAN && WP) {
            if (fast_st) exchange(std::true_type{}, val, prod, total);
            else exchange(std::false_type{}, val, prod, total);
        } else exchange(std::false_type{}, val, prod, total);
    };

    // ---- one-XCD launches: are we really on one XCD?  One extra all-to-all round (agent scope) with the XCC id as payload;
    // every workgroup reads the same W ids, so all take the same decision.  ~0.7 us once per launch.
    if ((WP || !LEAN) && !MR && X > 0 && W > 1 && W <= 64 && !(abl & 4)) {      // (the lean gathered form keeps agent scope: no round)
        __shared__ int s_same;
        ++epoch;
        if (wave == 0) {
            unsigned id;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
            id &= 0xfu;
            gu64 *pb = slots + (size_t)(epoch & 1) * W * slotG;
            if (lane == 0) __hip_atomic_store(pb + (size_t)wg * slotG, ((unsigned long long)epoch << 32) | id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gu64 *pp = pb + (size_t)min(lane, W - 1) * slotG;
            unsigned long long raw = 0;
            bool fail = false;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            for (unsigned spin = 0;; ++spin) {
                raw = __hip_atomic_load(pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all((unsigned)(raw >> 32) == epoch)) break;
                if ((spin & 255u) == 255u) {
                    const bool late = __builtin_amdgcn_s_memrealtime() - t0 > t_limit;
                    const bool other = __hip_atomic_load(g_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.launch_id;
                    if (late || other) { fail = true; break; }
                }
            }
            const bool same = !fail && __all((unsigned)raw == id);
            if (lane == 0) {
                s_same = same ? 1 : 0;
                if (fail) {
                    __hip_atomic_store(g_status, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_abort = 1;
                }
            }
        }
        __syncthreads();
        fast_st = s_same != 0;
        aborted = s_abort != 0;
    }
    // ---- r~ = Pinv r ; p = r~ ; eta = r . r~   (gato_pcg.cuh:316-335) ------------------------
    // DR: the operand window of the lane's knot comes from registers - its own block sits in the lanes of its DPP row(s) (`own` =
    // this lane's entry), the neighbouring knots' entries of the lane's row index are read from the LDS window (two scalars;
    // written before the last barrier).  Lanes without a row clamp their index: in bounds, finite, times a zero matrix row.
    auto dpp_times = [&](const auto &mat, int w, T own) -> T {
        if constexpr (DR) {
            const T *xw = &xs[w][j * SP];
            T y;
            if constexpr (S <= 16) {
                const int rc = r_ < S ? r_ : S - 1;
                const T x3[3] = {xw[rc], own, xw[2 * SP + rc]};
                y = row_times_dpp<T, S>(mat, x3);
            } else {
                const int c = r_ & 15;
                const T x6[6] = {xw[c], xw[16 + c], xw[SP + c], xw[SP + 16 + c], xw[2 * SP + c], xw[2 * SP + 16 + c]};
                y = row_times_dpp<T, S>(mat, x6);
            }
            return active ? y : (T)0;
        } else return (T)0;
    };
    auto pinv_times = [&](const T *xw, T own) -> T {
        if constexpr (NR) return (T)0;
        else if constexpr (DR) return dpp_times(pm, 1, own);
        else if constexpr (NL > 0) return row_times_window_lds<T, S, SP, NL, MAXT>(pm, ptail, tid, xw);
        else return row_times_window<T, S, SP>(pm, xw);
    };
    // ---- optional true warm start (the reference accepts input_lambda but restarts from
    // zero, gato_pcg.cuh:303):  lambda = lambda0,  r = gamma - S lambda0.  The ghost blocks of r then come from the
    // neighbours through the ordinary hand-off.  A cluster rank of several reads lambda0 on its OWN rows only (k_begin..k_end-1
    // of its array: in one process per GPU the other rows of that array are whatever the rank's earlier solves left there):
    // the ghost blocks of lambda0 cross the ranks in one hand-off of their own before r0 is formed.  That is one epoch more
    // per warm launch, inside the 2 max_iters + 8 a cluster launch reserves (it uses at most 2 max_iters + 3).
    if (a.lambda0) {
        const T *__restrict__ dL0 = static_cast<const T *>(a.lambda0) + sys * S * K;
        const bool lam0_xchg = MR && R > 1;
        lam = active ? dL0[(size_t)k * S + r_] : (T)0;
        if (active) xs[0][(j + 1) * SP + r_] = lam;
#pragma unroll 1
        for (int e = 0; e < ne; ++e) {
            const int q = tid + e * (int)blockDim.x;
            if (q < n_ext_rows) {
                const T l0 = dL0[(size_t)(k0 + xk) * S + q];
                xst[0][q] = l0;
                xs[0][(xk + q / S + 1) * SP + q % S] = l0;
            }
        }
        if (lam0_xchg) {
            if constexpr (NR) {             // the hand-off publishes from the product array: lambda0's boundary blocks go there
                __syncthreads();
                if (tid < S) xst[1][tid] = xst[0][tid];
                else if (tid < 2 * S) xst[1][(nk - 1) * S + (tid - S)] = xst[0][(nk - 1) * S + (tid - S)];
            }
            T dummy;
            exchange_rt(lam, (T)0, dummy);
            if constexpr (RG) {
                if (g_lane) xs[0][gslot] = hv_reg;
            } else {
                if (tid < S) xs[0][tid] = gh[0][tid];
                else if (tid < 2 * S) xs[0][(nk + 1) * SP + (tid - S)] = gh[1][tid - S];
            }
        } else if (tid < S) {
            if (has_left) xs[0][tid] = dL0[(size_t)(k0 - 1) * S + tid];
        } else if (tid < 2 * S) {
            if (has_right) xs[0][(nk + 1) * SP + (tid - S)] = dL0[(size_t)(k0 + nk) * S + (tid - S)];
        }
        __syncthreads();
        if constexpr (DR) r -= dpp_times(sm, 0, lam);
        else if constexpr (!NR) r -= row_times_window<T, S, SP>(sm, &xs[0][j * SP]);
        if constexpr (XR > 0) (void)extra_rows(dS, 0);                       // product array <- S lambda0 on the extra rows
        __syncthreads();
        if (active) xs[1][(j + 1) * SP + r_] = r;
#pragma unroll 1
        for (int e = 0; e < ne; ++e) {
            const int q = tid + e * (int)blockDim.x;
            if (q < n_ext_rows) xs[1][(xk + q / S + 1) * SP + q % S] -= xst[1][q];
        }
        if constexpr (NR) {                 // the hand-off publishes from the product array: put r's boundary blocks there
            __syncthreads();
            if (tid < S) xst[1][tid] = xs[1][SP + tid];
            else if (tid < 2 * S) xst[1][(nk - 1) * S + (tid - S)] = xs[1][nk * SP + (tid - S)];
        }
        if (multi) {
            T dummy;
            exchange_rt(r, (T)0, dummy);
            if constexpr (RG) {
                g_r = hv_reg;
                if (g_lane) xs[1][gslot] = g_r;
            } else {
                if (tid < S) xs[1][tid] = gh[0][tid];
                else if (tid < 2 * S) xs[1][(nk + 1) * SP + (tid - S)] = gh[1][tid - S];
            }
        }
        // the p window is rebuilt from r~ below; clear what lambda0 left in its ghost slots
        if (tid < S) xs[0][tid] = (T)0;
        else if (tid < 2 * S) xs[0][(nk + 1) * SP + (tid - S)] = (T)0;
        __syncthreads();
    }
    rt = pinv_times(&xs[1][j * SP], r);
    {
        T prod0 = r * rt;
        if constexpr (XR > 0) prod0 += extra_rows(dP, 1);
        exchange_rt(rt, prod0, eta);
    }
    const bool rec_on = a.eta_hist != nullptr;                 // wave-uniform: one scalar branch when recording is off
    const bool rec = wg == 0 && tid == 0 && sys == 0;
    if (rec_on && rec) a.eta_hist[0] = (double)eta;
    if (!aborted) {
        p = rt;
        if (active) xs[0][(j + 1) * SP + r_] = p;
#pragma unroll 1
        for (int e = 0; e < ne; ++e) {
            const int q = tid + e * (int)blockDim.x;
            if (q < n_ext_rows) xs[0][(xk + q / S + 1) * SP + q % S] = xst[1][q];
        }
        if (multi) {
            if constexpr (RG) {
                g_p = hv_reg;
                if (g_lane) xs[0][gslot] = g_p;
            } else {
                if (tid < S) xs[0][tid] = gh[0][tid];
                else if (tid < 2 * S) xs[0][(nk + 1) * SP + (tid - S)] = gh[1][tid - S];
            }
        }
        __syncthreads();

        auto iterate = [&](auto fastc) {
        for (int it = 0; it < a.max_iters; ++it) {                              // gato_pcg.cuh:348
            // upsilon = S p ; v = p . upsilon                                     (:349-357)
            GATO_STAMP(5)
            if constexpr (NR) ups = (T)0;
            else if constexpr (DR) ups = (abl & 1) ? p * sm[0] : dpp_times(sm, 0, p);
            else ups = (abl & 1) ? p * sm[0] : row_times_window<T, S, SP>(sm, &xs[0][j * SP]);
            GATO_STAMP(0)
            T v;
            {
                T prod = p * ups;
                if constexpr (XR > 0) prod += extra_rows(dS, 0);
                exchange(fastc, ups, prod, v);
            }
            GATO_STAMP(1)
            if (aborted) break;
            const T alpha = quotient(eta, v);                                    // :364
            lam += alpha * p;                                                   // :373-377
            r -= alpha * ups;
            if (active) xs[1][(j + 1) * SP + r_] = r;
#pragma unroll 1
            for (int e = 0; e < ne; ++e) {
                const int q = tid + e * (int)blockDim.x;
                if (q < n_ext_rows) {
                    const int wi = (xk + q / S + 1) * SP + q % S;
                    xst[0][q] += alpha * xs[0][wi];
                    xs[1][wi] -= alpha * xst[1][q];
                }
            }
            if (multi) {   // ghost r advances with the neighbours' upsilon blocks
                if constexpr (RG) {
                    g_r -= alpha * hv_reg;
                    if (g_lane) xs[1][gslot] = g_r;
                } else {
                    if (tid < S) xs[1][tid] -= alpha * gh[0][tid];
                    else if (tid < 2 * S) xs[1][(nk + 1) * SP + (tid - S)] -= alpha * gh[1][tid - S];
                }
            }
            if (!(abl & 8)) __syncthreads();                                    // B3
            GATO_STAMP(2)
            // r~ = Pinv r ; eta' = r . r~                                        (:380-394)
            rt = (abl & 2) ? r * pm[0] : pinv_times(&xs[1][j * SP], r);
            GATO_STAMP(3)
            {
                T prod = r * rt;
                if constexpr (XR > 0) prod += extra_rows(dP, 1);
                exchange(fastc, rt, prod, eta_new);
            }
            GATO_STAMP(4)
            if (aborted) break;
            if (rec_on) {
                if (rec) a.eta_hist[it + 1] = (double)eta_new;
            }
            if (fabs(eta_new) < tol) { iters = it; break; }                     // :404-411
            const T beta = quotient(eta_new, eta);                               // :415
            p = rt + beta * p;                                                  // :416-419
            if (active) xs[0][(j + 1) * SP + r_] = p;
#pragma unroll 1
            for (int e = 0; e < ne; ++e) {
                const int q = tid + e * (int)blockDim.x;
                if (q < n_ext_rows) {
                    const int wi = (xk + q / S + 1) * SP + q % S;
                    xs[0][wi] = xst[1][q] + beta * xs[0][wi];
                }
            }
            if (multi) {
                if constexpr (RG) {
                    g_p = hv_reg + beta * g_p;
                    if (g_lane) xs[0][gslot] = g_p;
                } else {
                    if (tid < S) xs[0][tid] = gh[0][tid] + beta * xs[0][tid];
                    else if (tid < 2 * S) xs[0][(nk + 1) * SP + (tid - S)] = gh[1][tid - S] + beta * xs[0][(nk + 1) * SP + (tid - S)];
                }
            }
            eta = eta_new;                                                      // :420
            if (!(abl & 8)) __syncthreads();                                    // B6
        }
        };
        if constexpr (LEAN && WP) {                 // the loop twice: workgroup-scope stores (verified one-XCD placement) / agent scope
            if (fast_st) iterate(std::true_type{});
            else iterate(std::false_type{});
        } else iterate(std::false_type{});
    }
    if (active) dL[(size_t)k * S + r_] = lam;                                   // :433-435
#pragma unroll 1
    for (int e = 0; e < ne; ++e) {
        const int q = tid + e * (int)blockDim.x;
        if (q < n_ext_rows) dL[(size_t)(k0 + xk) * S + q] = xst[0][q];
    }
    if constexpr (MR) (void)cluster_lambda_ghost<T, S>(a, wg, W, dL, aborted);      // lambda_{k_end} for this rank's dz launch
    // ---- dz back-substitution in the same launch (one-workgroup launches: every lambda_k is here).  Same formulas and
    // accumulation order as dz_kernel (gato_assembly.hip; gato_schur.cuh:758-867, D2 fixed): bit-identical results.
    if constexpr (XR == 0 && !MR) {
        if (a.dz != nullptr && W == 1) {
            const int Cn = a.C, n = S + Cn;
            const size_t gs = (size_t)(S * S + Cn * Cn), cs = (size_t)(S * S + S * Cn), Nn = (size_t)n * K - Cn;
            const T *__restrict__ Gi = static_cast<const T *>(a.dz_Ginv) + msys * (gs * K - (size_t)Cn * Cn);
            const T *__restrict__ Cdn = static_cast<const T *>(a.dz_Cd) + msys * (cs * (K - 1));
            const T *__restrict__ gv = static_cast<const T *>(a.dz_g) + sys * Nn;
            T *__restrict__ dzo = static_cast<T *>(a.dz) + sys * Nn;
            const bool last = k == K - 1;
            __syncthreads();                                                // every wave has left the loop: the windows are free
            if (active) xs[0][(j + 1) * SP + r_] = lam;                     // lambda window
            __syncthreads();
            T tx = (T)0, tu = (T)0;
            if (active) {
                if (!last) {
                    const T *__restrict__ A = Cdn + (size_t)k * cs;
                    const T *lp = &xs[0][(j + 2) * SP];                    // lambda_{k+1}
                    T res = (T)0;
#pragma unroll
                    for (int t = 0; t < S; ++t) res = gato::fmaT(A[r_ * S + t], lp[t], res);      // A_k^T lambda_{k+1}   :833-838
                    tx = gv[(size_t)k * n + r_] - (lam + res);                                    // :841-852
                    if (r_ < Cn) {
                        const T *__restrict__ B = A + S * S;
                        T rb = (T)0;
#pragma unroll
                        for (int t = 0; t < S; ++t) rb = gato::fmaT(B[r_ * S + t], lp[t], rb);    // B_k^T lambda_{k+1}   :784-789
                        tu = gv[(size_t)k * n + S + r_] - rb;                                     // :792-796
                    }
                } else tx = gv[(size_t)k * n + r_] - lam;                                         // last state row (D2)
                xs[1][(j + 1) * SP + r_] = tx;
            }
            __syncthreads();                                                // lambda_{k+1} has been read everywhere
            if (active && !last && r_ < Cn) xs[0][(j + 1) * SP + r_] = tu;
            __syncthreads();
            if (active) {
                const T *__restrict__ Qi = Gi + (size_t)k * gs;
                const T *tv = &xs[1][(j + 1) * SP];
                T res = (T)0;
#pragma unroll
                for (int cc = 0; cc < S; ++cc) res = gato::fmaT(Qi[r_ + cc * S], tv[cc], res);   // Q_k^-1 (...)         :856-865
                dzo[(size_t)k * n + r_] = res;
                if (!last && r_ < Cn) {
                    const T *__restrict__ Ri = Qi + S * S;
                    const T *uv = &xs[0][(j + 1) * SP];
                    T ru = (T)0;
                    for (int cc = 0; cc < Cn; ++cc) ru = gato::fmaT(Ri[r_ + cc * Cn], uv[cc], ru);   // R_k^-1 (...)         :799-808
                    dzo[(size_t)k * n + S + r_] = ru;
                }
            }
        }
    }
    if (wg == 0 && tid == 0) {
        a.iters[sys] = aborted ? -1 : iters;      // in-band: a timed-out hand-off is visible without a second call
        if (a.final_eta && sys == 0) *a.final_eta = (double)eta_new;
        if (STAMP && a.stamps) {
            for (int i = 0; i < 8; ++i) a.stamps[i] = seg[i];
            a.stamps[8] = __builtin_amdgcn_s_memtime() - t_begin;
            a.stamps[9] = __builtin_amdgcn_s_memrealtime() - rt_begin;
        }
    }
}

}  // namespace
}  // namespace gato
