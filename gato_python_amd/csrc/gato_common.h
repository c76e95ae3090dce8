// Internal header of libgato_hip.so (gfx950 only).  Not part of the C ABI (include/gato_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/gato_hip.h"

// (S, C) instantiations compiled in.  The reference is compiled for exactly one triple
// (CMakeLists.txt:18); here K is a runtime value and (S, C) picks one of these.
// Add shapes at build time with  make EXTRA_SHAPES="X(12,6) X(6,3)"  (S <= 32, S even, C <= S).
#ifndef GATO_EXTRA_SHAPES
#define GATO_EXTRA_SHAPES(X)
#endif
// default build: pendulum (2/1, the reference's test), IIWA-14 (14/7, its default), 32/16 (BASELINE config 5) and a few
// common robot sizes (tools/devbuild.sh predefines GATO_SHAPES with fewer shapes for a quick A/B library)
#ifndef GATO_SHAPES
#define GATO_SHAPES(X) X(2, 1) X(14, 7) X(32, 16) X(4, 2) X(6, 3) X(12, 6) GATO_EXTRA_SHAPES(X)
#endif

#define GATO_MAX_RANKS 8     /* GPUs of one node a cluster launch spans (gato_cluster_*) */

namespace gato {

void set_error(const char *fmt, ...);

// fused multiply-add in the operand type (__builtin_fma alone would promote floats to double)
__device__ __forceinline__ float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }

#define GATO_HIP_CHECK(expr)                                                                  \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ::gato::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                              __LINE__);                                                      \
            return GATO_EHIP;                                                                 \
        }                                                                                     \
    } while (0)

// ---- wave64 sum on the DPP network (no LDS traffic): quad swaps, half-row / row mirrors, then the
// gfx9 row broadcasts; the total lands in lane 63 and is returned wave-uniform.  Fixed order, so the
// result is bitwise reproducible.  (A __shfl_xor butterfly compiles to six dependent ds_bpermute_b32,
// each an LDS-crossbar round trip.)
// FULL = every lane has a valid source and all rows take part (quad permutes, mirrors): the move is issued with
// bound_ctrl, which makes the `old` operand dead so that the compiler does not zero a register pair before every
// DPP move (matters for f64, which has no DPP add: 8 v_mov less per wave sum).  The row broadcasts keep old = 0.
template <int CTRL, int ROW_MASK, bool FULL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, FULL));
}
template <int CTRL, int ROW_MASK, bool FULL>
__device__ __forceinline__ double dpp_mov(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, FULL);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, FULL);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float lane63(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ double lane63(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float lane0(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
}
__device__ __forceinline__ double lane0(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 0);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 0);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// Sum of the values in lanes 0..15 (the per-wave partials of a workgroup: at most 16 waves), wave-uniform: the four
// intra-row steps only - the two row broadcasts of the full wave sum are a third of its dependent chain.
// every lane ends with the sum of its row of 16 lanes
template <typename T>
__device__ __forceinline__ T row_sums_dpp(T v)
{
    v += dpp_mov<0xB1, 0xf, true>(v);
    v += dpp_mov<0x4E, 0xf, true>(v);
    v += dpp_mov<0x141, 0xf, true>(v);
    v += dpp_mov<0x140, 0xf, true>(v);
    return v;
}
// N: how many of the lanes 0..15 can hold a value (the others are zero): 8 values need three steps, 4 need two
template <typename T, int N = 16>
__device__ __forceinline__ T row0_sum_dpp(T v)
{
    v += dpp_mov<0xB1, 0xf, true>(v);
    v += dpp_mov<0x4E, 0xf, true>(v);
    if constexpr (N > 4) v += dpp_mov<0x141, 0xf, true>(v);
    if constexpr (N > 8) v += dpp_mov<0x140, 0xf, true>(v);
    return lane0(v);
}
template <typename T>
__device__ __forceinline__ T wave_sum_dpp(T v)
{
    v += dpp_mov<0xB1, 0xf, true>(v);    // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E, 0xf, true>(v);    // quad_perm [2,3,0,1]
    v += dpp_mov<0x141, 0xf, true>(v);   // row_half_mirror
    v += dpp_mov<0x140, 0xf, true>(v);   // row_mirror      -> every lane holds its row's sum
    v += dpp_mov<0x142, 0xa, false>(v);  // row_bcast:15 into rows 1,3
    v += dpp_mov<0x143, 0xc, false>(v);  // row_bcast:31 into rows 2,3 -> lane 63 holds the wave sum
    return lane63(v);
}

// Device layout sizes in elements (gato_defines.h:32-37, gpu_library.cu:40-45).
// B > 1: a batch of B independent systems of the same shape and sparsity pattern.  Every
// per-system array is stored B times back to back (system stride = its single-system size); the CSR structure
// (indptr / indices) is shared, the value arrays have nnzG / nnzC entries per system.
struct Dims {
    int S, C, K;
    int B = 1;
    int nnzG = 0, nnzC = 0;
    // stage-level entries only: knots [k_lo, k_hi) to work on (k_hi = 0: all).  A rank of a multi-GPU solve assembles
    // just the block rows its PCG shard reads (gato_python_amd/dist.py: assemble_shard)
    int k_lo = 0, k_hi = 0;
    int stair_follows = 0;      // internal (whole-solve stage path): the Schur launch need not zero the blocks the stair launch writes
    int rhs = 0;                // > 1 (gato_solve_rhs): B counts right-hand sides, and rhs consecutive ones share one system's matrices
    __host__ __device__ int lo() const { return k_lo; }
    __host__ __device__ int hi() const { return k_hi > 0 ? k_hi : K; }
    __host__ __device__ int n() const { return S + C; }
    __host__ __device__ size_t N() const { return (size_t)(S + C) * K - C; }
    __host__ __device__ size_t g_dense() const { return (size_t)(S * S + C * C) * K - C * C; }
    __host__ __device__ size_t c_dense() const { return (size_t)(S * S + S * C) * (K > 0 ? K - 1 : 0); }
    __host__ __device__ size_t bd() const { return (size_t)3 * S * S * K; }
    __host__ __device__ size_t sk() const { return (size_t)S * K; }
};

struct BatchStride {
    size_t g, c, bd, sk, n, nnzG, nnzC;     // elements per system: G_dense, C_dense, S/Pinv, gamma/lambda, g/dz, CSR values
    int k_lo, k_hi;                         // knots the launch works on
    int stair_follows;
    int rhs;                                // > 1: system sysi reads the matrices (G_dense, Ginv, C_dense, S, Pinv) of system sysi / rhs
};
inline BatchStride batch_stride(const Dims &d)
{
    return BatchStride{d.g_dense(), d.c_dense(), d.bd(), d.sk(), d.N(), (size_t)d.nnzG, (size_t)d.nnzC, d.lo(), d.hi(), 0, d.rhs};
}

// ---- persistent (resident) PCG launch description ------------------------------------------
struct PcgLaunch {
    const void *S_bd, *P_bd, *gamma;
    // optional (one-workgroup two-rows-per-lane kernels, one system): the same matrices TRANSPOSED - entry (row R = k S + r of
    // the system, column c of its block row) at img[c * img_ld + R], rows beyond K S and the blocks a first / last block row
    // lacks are zero - written by assemble_kernel beside S_bd / P_bd, so that a lane's 3S loads are coalesced
    const void *imgS, *imgP;
    int img_ld;
    void *lambda;
    const void *lambda0;         // initial guess (true warm start, r0 = gamma - S lambda0) or nullptr = cold start
    int K;
    int max_iters;
    double exit_tol;
    int batch;                   // > 1: blockIdx.x = system index, one workgroup per system (groups must be 1)
    int pair;                    // fp32 one-workgroup kernel with two rows per lane
    int xcd_pack;                // 2..32 workgroups: place them on one XCD (grid 8x oversubscribed, 7 of 8 blocks exit)
    int xcd_sel;                 // 0..7: the XCD (blockIdx % 8) that hosts them
    int wave_pub;                // launches of 2..32 workgroups: every wave publishes its own partial (no gather barrier); 0 = gathered form
    int knots_per_wg;            // contiguous knots owned by each workgroup (last may own fewer)
    int split_extra;             // pcg_cg1 only, set by its launcher: > 0 = balanced split - the first split_extra workgroups own
                                 // knots_per_wg knots, the others one less (the even split would leave the last workgroup ONE knot)
    int groups;                  // W = gridDim.x
    int threads;                 // blockDim.x (multiple of 64, >= knots_per_wg * S unless semi)
    int dpp_rows;                // 1: DPP-row layout (a knot owns whole 16-lane rows; threads >= knots_per_wg * 16 or 32), plain and cluster launches
    int semi;                    // 1: semi-resident launch (knots_per_wg exceeds the lanes, the rest are extra rows); 2: no resident rows; 3: LDS-DMA ring (gato_pcg_dma.hip)
    unsigned long long *slots;   // hand-off granules: every 8-byte word {epoch, payload}; epochs only grow, so no re-zeroing
    unsigned epoch0;             // this launch uses epochs epoch0+1 .. (the solver hands out disjoint ranges)
    // knot range [k_begin, k_end) of the system this launch works on (single GPU: 0, K).  Multi-GPU cluster launch
    // (gato_cluster_pcg): rank r of nranks runs this kernel on ITS range; K stays the global knot count, S_bd / P_bd /
    // gamma / lambda are full-system arrays of which only the rows of the range are touched.
    int k_begin, k_end;
    int rank, nranks;            // nranks > 1: second hand-off level through the cross-GPU mirrors below
    unsigned long long *xslots;                    // this rank's mirror (fine-grained memory, written by the peers)
    unsigned long long *const *xpeer;              // DEVICE table [nranks]: every rank's mirror as mapped into this process (xpeer[rank] == xslots)
    // optional: dz back-substitution (compute_dz, gato_schur.cuh:758-867) in the epilogue of a ONE-workgroup launch (the
    // workgroup holds every lambda_k): Ginv / C_dense / g in the layouts of gato_compute_dz, C = CONTROL_SIZE
    const void *dz_Ginv, *dz_Cd, *dz_g;
    void *dz;
    int C;
    int dz_helpers;              // 1: the helper blocks of the one-workgroup fp64 launch do the dz back-substitution once *dz_flag == launch_id
    int *dz_flag;                // device word: the solving workgroup stores launch_id there when lambda is complete
    // flat variant of the cluster exchange (ranks x workgroups <= 256): every workgroup stores its partial straight into
    // every rank's mirror and its boundary blocks into its own and (at the rank's edges) the neighbour's - ONE level, no
    // wait for the rank's own gather first.  The flat area follows the two-level area in every mirror.
    int flat, flat_groups, flat_base;
    size_t flat_off;             // granules from the start of a mirror to its flat area
    unsigned xepoch0;            // cross-GPU epochs: in lock-step on all ranks (only cluster launches draw from this counter)
    // cluster launches, at exit: the rank's first lambda block goes into the LEFT neighbour's mirror (granules at lam_off, tag
    // lam_tag: unique per launch, the same on every rank) and the rank's last workgroup stores the right neighbour's block at
    // lambda[k_end] - dz of the rank's last knot needs lambda_{k_end} (gato_schur.cuh:833-838), so no lambda all-reduce stands
    // between the PCG and the dz launch of a sharded solve.  lam_tag = 0: off.
    size_t lam_off;
    unsigned lam_tag;
    int launch_id;               // > 0; a timed-out hand-off stores it into *status (stale ids of earlier launches are ignored)
    int *iters;                  // device
    int *status;                 // device, 0 ok / 1 timeout
    double *final_eta;           // device (optional)
    double *eta_hist;            // device (optional): eta after init [0] and after iteration i [i+1] (system 0 of a batch)
    unsigned long long timeout_ticks;  // s_memrealtime ticks (100 MHz)
    hipEvent_t ev_start, ev_stop;      // optional: recorded right around the kernel launch
    int ablate;                        // diagnostic: timing-only ablation mask (0 in production)
    unsigned long long *stamps;        // optional: diagnostic cycle stamps (16 words), selects the DIAG = 1 build
    int diag;                          // 2: the build with the timing-only switches (ablate) but no stamps
    int coop;                          // multi-workgroup persistent launches through hipLaunchCooperativeKernel (option coop_launch)
    int rhs;                           // > 1 (batches, gato_solve_rhs): workgroup b reads S / Pinv / dz_Ginv / dz_Cd of system b / rhs
                                       // and gamma / lambda / dz_g / dz / iters of b; 0 or 1: every workgroup its own system
};

// Cross-GPU mirror of a cluster launch, per epoch parity (granules): one 128-B line per rank for its total (written by
// that rank's workgroup 0 into EVERY rank's mirror), then the left and the right ghost S-block (written by the
// neighbouring rank's last / first workgroup).  Every line has exactly one writer.
// (two S-blocks per side: the single-reduction recurrence exchanges the first / last TWO blocks of w, gato_pcg_cg1.hip)
__host__ __device__ inline int pcg_xghost_granules(int S, int esz) { return ((2 * S * (esz / 4) + 15) / 16) * 16; }
__host__ __device__ inline int pcg_xslot_granules(int S, int esz) { return 16 * GATO_MAX_RANKS + 2 * pcg_xghost_granules(S, esz); }

// Granules (8 B: {epoch:32 | payload:32}) per workgroup and parity in the hand-off area.
// Line 0 (16 granules) holds the partial dot, then first-block and last-block halos.
__host__ __device__ inline int pcg_slot_granules(int S, int esz)
{
    int gpv = esz / 4;                       // granules per value
    int halo = 2 * S * gpv;
    return 16 + ((halo + 15) / 16) * 16;
}

// Hand-off slot of the single-reduction variant: line 0 = {gamma', delta}, then the first two and last two S-blocks of w.
__host__ __device__ inline int pcg_slot_granules_cg1(int S, int esz)
{
    int gpv = esz / 4;
    return 16 + ((4 * S * gpv + 15) / 16) * 16;
}

// A workgroup's slot in the FLAT area of a cluster mirror: room for either recurrence's slot.
__host__ __device__ inline int pcg_flat_slot_granules(int S, int esz)
{
    const int a = pcg_slot_granules(S, esz), b = pcg_slot_granules_cg1(S, esz);
    return a > b ? a : b;
}
// Granules of the lambda ghost block behind the flat area (one S-block, whole 128-B lines).
__host__ __device__ inline int pcg_lamghost_granules(int S, int esz) { return ((S * (esz / 4) + 15) / 16) * 16; }

struct PcgPlan {
    int max_threads;     // launch bound of the instantiation
    int max_knots_per_wg;
    int single_max_threads;   // > max_threads: a one-workgroup variant (Pinv rows partly in LDS) exists up to this size
    int pair_threads;         // > 0: fp32 one-workgroup kernel with two rows per lane, up to this many threads
    int mixed_rows, mixed_threads;   // > 0: fp64 one-workgroup kernel with two rows per lane in some waves (pcg_single_f64m_kernel)
    int semi_threads;         // > 0: semi-resident variant (extra rows re-read from memory): its workgroup size ...
    int semi_rows;            // ... and the extra rows a lane can take
    int nores_threads;        // > 0: variant without resident rows: workgroup size ...
    int nores_rows;           // ... and rows per lane
    int dpp_lanes;            // > 0: the plain and cluster launches exist in the DPP-row layout, with this many lanes per knot
};

// Per-(dtype, S, C) kernel launchers, defined in the .hip files and instantiated for GATO_SHAPES.
template <typename T, int S, int C>
int launch_convert(const Dims &d, const int *G_row, const int *G_col, const T *G_val, const int *C_row,
                   const int *C_col, const T *C_val, T rho, T *Gd, T *Cd, T *Ginv /* optional: also invert Q_k, R_k */,
                   hipStream_t st);
template <typename T, int S, int C>
int launch_add_rho(const Dims &d, const T *G_in, T rho, T *Gd, hipStream_t st);
template <typename T, int S, int C>
int launch_form_schur(const Dims &d, const T *Gd, const T *Cd, const T *g, const T *c, T *Sbd, T *Pbd,
                      T *gamma, T *Ginv, bool have_inverses, hipStream_t st);
// Fused assembly (A1 + A2 + A3) in one launch: see assemble_kernel in gato_assembly.hip.
struct AsmArgs {
    int mode;                        // 0: CSR in, G_dense/C_dense out; 1: G_dense/C_dense in; 2: G blocks in (+rho) -> G_dense, C_dense in
    const int *G_row, *G_col, *C_row, *C_col;
    const void *G_val, *C_val;       // mode 2: G_val = the caller's G blocks
    double rho;
    const void *g, *c;
    void *Gd, *Cd, *Ginv, *Sbd, *Pbd, *gamma;
    void *imgS, *imgP;               // optional (one system): S and Pinv also as column-major images over ALL rows (PcgLaunch::imgS), leading dimension img_ld
    int img_ld;
    unsigned long long *stamps;      // diagnostic (option stamp_asm): one workgroup's phase boundaries, 100 MHz ticks
};
template <typename T, int S, int C>
int launch_assemble(const Dims &d, const AsmArgs &a, hipStream_t st);

template <typename T, int S, int C>
int launch_form_ss(const Dims &d, const T *Sbd, T *Pbd, hipStream_t st);
template <typename T, int S, int C>
int launch_point_jacobi(const Dims &d, const T *Sbd, T *Pbd, hipStream_t st);
template <typename T, int S, int C>
int launch_compute_dz(const Dims &d, const T *Ginv, const T *Cd, const T *g, const T *lambda, T *dz,
                      hipStream_t st);
// gamma = c - C G^-1 g for R new right-hand sides per system from the blocks of the latest assembly (gato_rhs.hip):
// g [B][R][N], c [B][R][S K] -> gamma [B][R][S K]; Ginv, Cd, Sbd of B systems
template <typename T, int S, int C>
int launch_rhs_gamma(const Dims &d, int R, const T *Ginv, const T *Cd, const T *Sbd, const T *g, const T *c, T *gamma,
                     hipStream_t st);
// Gradients of a solve from dz, lambda and the adjoint (a, beta) of B systems (gato_grad.hip): G_bar [B][g_dense],
// C_bar [B][c_dense] (either may be null), or per CSR entry of a pattern the systems share, [B][nnz] (either may be null)
template <typename T, int S, int C>
int launch_grad_blocks(const Dims &d, const T *dz, const T *lam, const T *a, const T *beta, T *Gbar, T *Cbar, hipStream_t st);
template <typename T, int S, int C, bool CROSS = false>     // CROSS: gato_kkt_grad_csr_cross, a unit-local instantiation of gato_grad.hip
int launch_grad_csr(const Dims &d, const int *G_row, const int *G_col, int nnzG, const int *C_row, const int *C_col, int nnzC,
                    const T *dz, const T *lam, const T *a, const T *beta, T *Gbar, T *Cbar, hipStream_t st);
// Box-constrained QP by ADMM over the KKT re-solve (gato_qp.hip).  Per-system arrays [B][...]:
// vectors in the dz layout [B][N] unless noted.  `slots` [B][3][GATO_QP_NSLOT] rotating maxima (bit patterns of
// non-negative doubles), `status` [B] (-1 while the system runs), `ctr` {live systems, bad bound variables}.
#define GATO_QP_NSLOT 10
struct QpArgs {
    const void *G, *Cd, *g, *c, *lo, *hi;   // the caller's blocks (G without rho, C raw) and vectors; c [B][S K]
    void *Gp;                               // prepare: G + diag(sigma + rho_i) [B][G_dense]
    void *rho;                              // penalties rho_i
    const void *xr;                         // x^k (update: read; neighbours read it too)
    void *xw;                               // x^k+1 (update) / x^0 (prepare)
    void *x, *z, *y, *lam;                  // the caller's outputs (z, y, lam also the warm start of prepare); lam [B][S K]
    void *gt;                               // right-hand side of the next x-step
    const void *xt;                         // the x-step's solution: dz [B][N] ...
    void *lt;                               // ... and lambda [B][S K] (written only to zero it after a zero right-hand side)
    unsigned long long *slots;
    int *status, *iters, *ctr;
    double *res;                            // [B][2]
    const int *pcg_its;                     // update: PCG iterations of the x-step, one per system (nullptr: none)
    int *pcg_total;                         // [B] PCG iterations of all x-steps of a system so far
    double rho_reg, admm_rho, sigma, alpha, eps_abs, eps_rel;
    int warm;
};
template <typename T, int S, int C>
int launch_qp_prepare(const Dims &d, const QpArgs &a, hipStream_t st);
// iteration `it` of the loop; last = 1: only the convergence test of the iterate the previous launch wrote
template <typename T, int S, int C>
int launch_qp_update(const Dims &d, const QpArgs &a, int it, int last, hipStream_t st);
// Polish of an ADMM result and the bound gradients of a polished solution (gato_polish.hip, DESIGN.md sections 3.8, 3.10).
// `act` [B][N] int8: +1 at the upper bound, -1 at the lower one, 0 free.  `slots` [B][GATO_POLISH_NSLOT] maxima as in QpArgs.
#define GATO_POLISH_NSLOT 12
struct PolishArgs {
    const void *G, *Cd, *g, *c, *lo, *hi;   // the caller's blocks (G without rho, C raw) and vectors; never written
    const signed char *act;
    const void *w;                          // [B][N] soft-bound weights, 0 = a hard bound; nullptr = all hard
    const void *cap;                        // [B][N] caps of the penalty force, read where w > 0 (+inf: none); nullptr = no caps
    const void *Gd;                         // prepare: G + rho I (the solver's G_dense)
    void *Ginv;                             // prepare: the inverses with the active rows and columns zero (the solver's Ginv)
    void *gp, *cp;                          // prepare: the reduced system's right-hand side g' [B][N], c' [B][S K]
    const void *xt, *lt;                    // finish: the reduced solve's dz [B][N] and lambda [B][S K]
    void *xp, *zp, *yp;                     // finish: the polished point [B][N]
    unsigned long long *slots;              // zeroed before the finish
    int *bad;                               // prepare: the count of systems with an act that names an infinite bound or x_0
    void *x, *z, *y, *lam;                  // write-back: the caller's ADMM result, replaced where the polish is accepted
    int *status, *polish;
    double *res;                            // [B][2]
    double rho, eps_abs, eps_rel;
};
template <typename T, int S, int C>
int launch_qp_active(const Dims &d, const void *z, const void *y, const void *lo, const void *hi, signed char *act, hipStream_t st);
template <typename T, int S, int C>
int launch_polish_prepare(const Dims &d, const PolishArgs &a, hipStream_t st);
// the residuals of the polished point, then the acceptance test and the write-back (two launches)
template <typename T, int S, int C>
int launch_polish_finish(const Dims &d, const PolishArgs &a, hipStream_t st);
struct BoundGradArgs {
    const void *G, *Cd;                     // the caller's blocks (G without rho, C raw)
    const signed char *act;
    const void *w, *lo, *hi, *x;            // w may be nullptr (all hard): then lo, hi and x are not read
    const void *xbar, *adz, *beta;          // the upstream gradient and the adjoint [a; beta]
    void *lo_bar, *hi_bar, *w_bar;          // [B][N]; w_bar may be nullptr (not written)
    const void *cap;                        // the capped entry only: [B][N] caps; nullptr = none (no variable is saturated)
    void *cap_bar;                          // [B][N], the capped entry only; nullptr: not written
};
template <typename T, int S, int C>
int launch_qp_bound_grad(const Dims &d, const BoundGradArgs &a, hipStream_t st);
// Right-hand side of the tangent system of a solve or a converged box-QP point (gato_tangent.hip).
// Tangents [B][R][...], shared inputs [B][...]; every tangent may be nullptr (zero).
struct TangentArgs {
    const void *G_dot, *C_dot;              // [B][R][G_dense], [B][R][C_dense]
    const void *g_dot, *c_dot;              // [B][R][N], [B][R][S K]
    const void *lo_dot, *hi_dot, *w_dot, *m_dot;    // [B][R][N]
    const void *x, *lam;                    // the point [B][N], [B][S K]
    const void *G, *Cd;                     // the caller's blocks (G without rho, C raw); read with an act only
    const signed char *act;                 // nullptr: nothing active (a plain KKT solve)
    const void *w, *cap, *lo, *hi;          // as BoundGradArgs: w nullptr = all hard, then lo and hi are not read
    void *tg, *tc;                          // [B][R][N], [B][R][S K]
};
template <typename T, int S, int C>
int launch_kkt_tangent_rhs(const Dims &d, int R, const TangentArgs &a, hipStream_t st);
// Primal-dual active-set iteration over the polish path (gato_pdas.hip, DESIGN.md sections 3.9, 3.10).
struct PdasArgs {
    PolishArgs p;                           // p.act: the current act; p.slots [B][2][GATO_POLISH_NSLOT], set it % 2 of solve it
    signed char *act;                       // p.act again, written by the decision (the caller's: in the start, out the final act)
    signed char *act2;                      // act' [B][N]
    int *round;                             // [B][2][2] per set: {entries where act' differs from act, system frozen before the solve}
    int *ctr;                               // {live systems, waves that saw a bad bound, waves that saw a bad start act}
    int *iters;                             // [B] solves until the system froze
};
// the checks of the bounds, the weights and the start act (first launch of a call)
template <typename T, int S, int C>
int launch_pdas_check(const Dims &d, const PdasArgs &a, hipStream_t st);
// after reduced solve `it` (1, 2, ...): the point, act' and the maxima; launch_pdas_decide follows
template <typename T, int S, int C>
int launch_pdas_step(const Dims &d, const PdasArgs &a, int it, hipStream_t st);
// the decision of solve `it` (pdas_decide_kernel); last: no solve follows
template <typename T, int S, int C>
int launch_pdas_decide(const Dims &d, const PdasArgs &a, int it, int last, hipStream_t st);
// Exact line search of the soft active-set iteration (gato_pdas_ls.hip): along d = x+ - xc the slope
// phi'(alpha) = d^T (H (xc + alpha d) - g + f(xc + alpha d)), H = G + rho I, f the capped penalty force of section 3.11.
struct LineSearchArgs {
    const void *G, *g, *lo, *hi, *w, *cap;  // the caller's blocks (G without rho) and vectors [B][N]; cap may be nullptr (none)
    const void *xc, *xp;                    // the current iterate and the Newton point x+ [B][N]
    void *xout;                             // the stepped iterate [B][N] (the loop: xc itself); nullptr: not written
    double *part;                           // [B][K][2] per knot: d_k^T (H_k xc_k - g_k), d_k^T H_k d_k
    double *alpha;                          // step lengths, system sys at alpha[sys * alpha_stride]; nullptr: not written
    size_t alpha_stride;
    double *slope;                          // [B][2] phi'(0), phi'(1); nullptr: not written
    // the loop only (status == nullptr: the kernels alone, no system is skipped and no act is written)
    const int *status;                      // a system frozen before this solve (status >= 0) is skipped
    const unsigned long long *slots;        // the solve's maxima [B][2][GATO_POLISH_NSLOT]: an accepted or non-finite point takes no step
    const signed char *act;                 // the act of the solve
    signed char *act2;                      // act' from the stepped iterate
    int *round;                             // PdasArgs::round: the changed count of act' replaces the step kernel's
    int *bad;                               // the scope check: waves that saw a finite hard bound
    int *status_out;                        // the scope check marks BAD_BOUNDS here
    double rho, eps_abs, eps_rel;
    int it;                                 // the solve (1: the first of a call, xc <- x+ and alpha = 1)
};
// the scope of the option: a finite bound off x_0 without a weight marks the system BAD_BOUNDS (after launch_pdas_check)
template <typename T, int S, int C>
int launch_ls_scope(const Dims &d, const LineSearchArgs &a, hipStream_t st);
// the per-knot partial sums, then the per-system step length, stepped iterate and (the loop) act' and its changed count
template <typename T, int S, int C>
int launch_line_search(const Dims &d, const LineSearchArgs &a, hipStream_t st);
// Hard bounds by an augmented-Lagrangian outer loop over the line-search iteration (gato_alm.hip).
// ALM variables: a finite bound, no user weight, off the states of x_0.  The inner run solves the all-soft problem on lo2, hi2,
// w2 (cap2) from act; its point is xi, zi, yi, li with status_i, iters_i, res_i.
struct AlmArgs {
    const void *lo, *hi, *w, *cap;          // the caller's bounds, weights and caps [B][N]; w, cap may be nullptr
    const void *mu0;                        // check: the start multiplier [B][N]; nullptr: 0
    const signed char *act0;                // check: the caller's start act, copied to act; nullptr: act is not written
    const void *xi, *zi, *yi, *li;          // the inner point [B][N], li [B][S K]
    const int *status_i, *iters_i;          // the inner run's status and solves [B]
    const double *res_i;                    // and residuals [B][2]
    signed char *act;                       // the inner run's act [B][N] (in: its start, out: its last)
    void *lo2, *hi2, *w2, *cap2, *mu;       // the inner bounds, weights, caps (nullptr without caps) and the multiplier [B][N]
    double *state;                          // [B][2][2] per set {w, v_prev}: step k reads set k % 2 and writes the other
    unsigned long long *slots;              // [B][2][2] per set {v, |x|_inf} of step k % 2, as bit patterns
    int *flag;                              // [B] the system was frozen before this step (update writes, decide reads)
    int *tot;                               // [B] reduced solves of all steps so far
    int *ctr;                               // {live systems, waves that saw a bad bound, weight, cap or parameter}
    void *x, *z, *y, *lam;                  // the caller's outputs, written on acceptance only
    signed char *act_out;                   // the accepted act [B][N]; nullptr: not written
    int *iters, *status, *outer, *dec;      // [B]; outer, dec (GATO_ALM_*) may be nullptr
    double *res, *weight;                   // [B][2]; [B] the weight of the last step, may be nullptr
    double alm_weight, growth, weight_max, eps_abs, eps_rel;
};
enum { GATO_ALM_ACCEPT = 0, GATO_ALM_GROW = 1, GATO_ALM_KEEP = 2, GATO_ALM_LAST = 3, GATO_ALM_INNER = 4 };
// the checks of the parameters, bounds, weights and caps, and the inner inputs of the first step (first launch of a call)
template <typename T, int S, int C>
int launch_alm_check(const Dims &d, const AlmArgs &a, hipStream_t st);
// after the inner run of outer step `it` (1, 2, ...): v, |x|_inf and mu <- y, then the decision (last: no step follows)
template <typename T, int S, int C>
int launch_alm_update(const Dims &d, const AlmArgs &a, int it, int last, hipStream_t st);
template <typename T, int S>
int pcg_resident_plan(PcgPlan *plan);
template <typename T, int S>
int launch_pcg_resident(const PcgLaunch &a, hipStream_t st);
template <typename T, int S>
int launch_pcg_resident_dpp(const PcgLaunch &a, hipStream_t st);      // gato_pcg_resident_dpp.hip (DPP-row instantiations); called by launch_pcg_resident
template <typename T, int S>
int launch_pcg_single(const PcgLaunch &a, bool mr, hipStream_t st);   // gato_pcg_resident_single.hip (the one-workgroup kernels); called by launch_pcg_resident
template <typename T, int S> int pcg_dma_max_knots();          // knots per workgroup of the LDS-DMA variant (0: none for this shape)
template <typename T, int S>
int launch_pcg_dma(const PcgLaunch &a, hipStream_t st);
template <typename T, int S> int pcg_cg1_max_threads();
template <typename T, int S>
int launch_pcg_cg1(const PcgLaunch &a, hipStream_t st);

// Streaming PCG (two launches per iteration), gato_pcg_stream.hip
struct PcgStreamWork {
    void *vecs;                    // 6 consecutive S*K vectors: r[2], p[2], upsilon, r~
    void *partials;                // [4][max_groups] of T: eta' ring of 3 + v
    void *scalars;                 // final eta (double)
    int *done;                     // device flag
    int max_groups;
    int warm_start;                // lambda holds an initial guess on entry
    double *eta_hist;              // optional
};
// One launch of the streaming PCG on a shard of block rows (see gato_pcg_stream.hip).
struct StreamStep {
    const void *M;          // S_bd (phase A) or Pinv_bd (phase B), local block rows
    const void *a_old;      // p_old (A) / r_old (B) / gamma (init)
    const void *b;          // r~ (A) / upsilon (B)
    void *a_new;            // p_new (A) / r_new (B)
    void *y;                // upsilon (A) / r~ (B)
    void *lam;              // B and init
    const void *p_cur;      // B only: p of this iteration
    const void *part_num;   // coefficient = sum(num)/sum(den): partial arrays with element stride
    const void *part_den;
    int num_n, num_stride, den_n, den_stride;
    void *part_out;         // one slot per workgroup
    // ghosts of the neighbouring shards (multi-GPU): S-blocks of a_old and b, and where the advanced ghost goes
    const void *gh_a_left, *gh_a_right, *gh_b_left, *gh_b_right;
    void *gh_new_left, *gh_new_right;
    int first_global, last_global;
    int K;                  // local knots
    int it;
    int max_iters;
    double exit_tol;
    int *done;
    int *iters;
    double *eta_hist;       // optional history buffer (see PcgLaunch)
};
template <typename T, int S> int stream_grid(int K, int max_groups);
template <typename T, int S> int launch_stream_step(int phase, const StreamStep &a, int grid, hipStream_t st);
template <typename T, int S>
int launch_stream_pack(const void *slots, int nslots, const void *y, int K, void *send, hipStream_t st);
template <typename T, int S>
int launch_stream_finish(const void *part, int n, int stride, double exit_tol, int last_it, int *done, int *iters,
                         double *final_eta, double *eta_hist, hipStream_t st);

template <typename T, int S>
int launch_pcg_streaming(const Dims &d, const T *Sbd, const T *Pbd, const T *gamma, T *lambda,
                         T exit_tol, int max_iters, int *iters, const PcgStreamWork &w, hipStream_t st);

// Type-erased table used by the C ABI.
struct Ops {
    int S, C, dtype;
    int (*convert)(const Dims &, const int *, const int *, const void *, const int *, const int *,
                   const void *, double, void *, void *, void *, hipStream_t);
    int (*add_rho)(const Dims &, const void *, double, void *, hipStream_t);
    int (*form_schur)(const Dims &, const void *, const void *, const void *, const void *, void *, void *,
                      void *, void *, bool, hipStream_t);
    int (*form_ss)(const Dims &, const void *, void *, hipStream_t);
    int (*point_jacobi)(const Dims &, const void *, void *, hipStream_t);
    int (*assemble)(const Dims &, const AsmArgs &, hipStream_t);
    int (*compute_dz)(const Dims &, const void *, const void *, const void *, const void *, void *,
                      hipStream_t);
    int (*rhs_gamma)(const Dims &, int, const void *, const void *, const void *, const void *, const void *, void *,
                     hipStream_t);
    int (*grad_blocks)(const Dims &, const void *, const void *, const void *, const void *, void *, void *, hipStream_t);
    int (*grad_csr)(const Dims &, const int *, const int *, int, const int *, const int *, int, const void *, const void *,
                    const void *, const void *, void *, void *, hipStream_t);
    int (*qp_prepare)(const Dims &, const QpArgs &, hipStream_t);
    int (*qp_update)(const Dims &, const QpArgs &, int, int, hipStream_t);
    int (*qp_active)(const Dims &, const void *, const void *, const void *, const void *, signed char *, hipStream_t);
    int (*polish_prepare)(const Dims &, const PolishArgs &, hipStream_t);
    int (*polish_finish)(const Dims &, const PolishArgs &, hipStream_t);
    int (*qp_bound_grad)(const Dims &, const BoundGradArgs &, hipStream_t);
    int (*kkt_tangent_rhs)(const Dims &, int, const TangentArgs &, hipStream_t);
    int (*pdas_check)(const Dims &, const PdasArgs &, hipStream_t);
    int (*pdas_step)(const Dims &, const PdasArgs &, int, hipStream_t);
    int (*pdas_decide)(const Dims &, const PdasArgs &, int, int, hipStream_t);
    int (*ls_scope)(const Dims &, const LineSearchArgs &, hipStream_t);
    int (*line_search)(const Dims &, const LineSearchArgs &, hipStream_t);
    int (*alm_check)(const Dims &, const AlmArgs &, hipStream_t);
    int (*alm_update)(const Dims &, const AlmArgs &, int, int, hipStream_t);
    int (*pcg_plan)(PcgPlan *);
    int (*pcg_resident)(const PcgLaunch &, hipStream_t);
    int (*pcg_dma_max_knots)();
    int (*pcg_dma)(const PcgLaunch &, hipStream_t);
    int (*pcg_cg1_max_threads)();
    int (*pcg_cg1)(const PcgLaunch &, hipStream_t);
    int (*pcg_streaming)(const Dims &, const void *, const void *, const void *, void *, double, int, int *,
                         const PcgStreamWork &, hipStream_t);
    int (*stream_grid)(int, int);
    int (*stream_step)(int, const StreamStep &, int, hipStream_t);
    int (*stream_pack)(const void *, int, const void *, int, void *, hipStream_t);
    int (*stream_finish)(const void *, int, int, double, int, int *, int *, double *, double *, hipStream_t);
};
const Ops *find_ops(int S, int C, int dtype);

}  // namespace gato
