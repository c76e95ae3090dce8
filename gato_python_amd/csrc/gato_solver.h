// Internal to libgato_hip.so (not installed): the solver object behind the C ABI and what its host-only units share.
#pragma once
#include <mutex>

#include "gato_common.h"

using namespace gato;

#define GATO_ETA_HIST_MAX 4096

// ---- solver object -----------------------------------------------------------------------------
struct gato_solver {
    Dims d;
    int dtype, device;
    size_t esz;
    const Ops *ops;
    int num_cus;
    // options
    int pcg_mode, pcg_threads, pcg_groups;
    int wave_pub;                       // option: per-wave published partials in launches of up to 32 workgroups (default 1)
    // arena
    char *arena;
    size_t arena_bytes;
    void *G_dense, *C_dense, *Ginv, *Sbd, *Pbd, *gamma, *lambda, *dz;
    int *iters, *status;
    double *final_eta;
    unsigned long long *slots;
    PcgStreamWork sw;
    PcgPlan plan;
    // device copies of host CSR inputs for gato_linsys_solve_* (sized on first use)
    char *in_arena;
    size_t in_bytes;
    char *pin;            // pinned host staging (inputs, then iters | lambda | dz)
    size_t pin_bytes;
    int last_groups, last_threads, last_mode, last_variant, last_semi, last_pair, last_dpp;   // the latest PCG launch
    int time_pcg, stamp_pcg, ablate, xcd_sel, no_single_lds, true_warm_start, no_pair, pcg_variant, xcd_pack;
    hipEvent_t ev_pcg0, ev_pcg1;
    hipEvent_t ev_cal0, ev_cal1;         // XCD calibration of the one-XCD launches
    long long xcd_cal_key;              // geometry the choice below was measured for (0 = none yet)
    int xcd_cal_best, last_xcd_sel;
    int *tune_iters, *tune_status;      // scratch words of the trial launches (never the caller's, never the sticky status)
    double *tune_eta;
    // knot-sharded PCG state (gato_shard_pcg_*)
    struct {
        int rank, nranks, k0, k1, grid, max_iters;
        double exit_tol;
        const char *S_full, *P_full, *gamma_full;
    } sh;
    char *ghosts;   // [r|p][ping-pong][left|right][S]
    int pcg_semi;              // option: semi-resident launch (-1 auto, 0 off)
    int dpp_rows;              // option: DPP-row layout (-1 auto, 0 never, 1 wherever a plain launch fits)
    unsigned pcg_epoch;        // next free hand-off epoch (resident kernels)
    int pcg_launch_id;
    size_t slots_bytes;
    int asm_mode;       // option: 0 = auto, 1 = stage kernels one by one (convert / invert / schur / stair), 2 = fused launch (workgroup per knot)
    int last_asm_fused, stamp_asm, last_image;
    double *eta_hist;   // eta after init and after every iteration (option record_eta), GATO_ETA_HIST_MAX + 1 entries
    int record_eta;
    // hand-off time-outs: the status word holds the id of the most recent launch that timed out (never cleared by a
    // kernel); ids only grow, so "status differs from the last acknowledged value" = a time-out since the last check
    int status_ack;
    hipStream_t last_stream;          // stream of the most recent PCG launch (gato_pcg_status synchronises it)
    int timeout_ms;                   // option: bound of every in-kernel spin (default 2000)
    int precon_mode;                  // option: GATO_PRECON_* (whole-solve entries)
    int time_stages;                  // option: hipEvents around assembly / PCG / dz of the whole-solve entries
    hipEvent_t ev_stage[4];
    int cluster_flat;                 // option: 1 (default) = flat cluster exchange where it applies, 0 = always two levels
    int max_workgroups;               // option: CUs a persistent launch may count on (0 = all; ranks sharing one GPU in tests)
    int last_fallback;                // the most recent gato_solver_recover re-ran the PCG through the streaming kernels
    struct {                          // arguments of the most recent whole solve, for gato_solver_recover
        int valid;
        const void *S, *P, *gamma, *Cd, *g;
        void *lam, *dz;
        double exit_tol;
        int max_iters;
        int rhs;                      // > 0: it was a re-solve (gato_solve_rhs) of this many right-hand sides per system
        int *its;                     // its iteration counts [B][rhs]
    } lc;
    // multi-GPU cluster (gato_cluster_*): this rank's mirror, the peers' mirrors as mapped here
    struct {
        int on, rank, nranks, k0, k1;
        unsigned long long *local;
        unsigned long long *peer[GATO_MAX_RANKS];
        bool opened[GATO_MAX_RANKS];
        size_t bytes, flat_off, lam_off;
        unsigned xepoch;
        int last_flat;
        int mem_kind;                 // 0 uncached, 1 fine-grained, 2 plain hipMalloc
        size_t alloc_bytes;           // size of the allocation behind local (>= bytes: recycled mirrors, mirror_take)
    } cl;
    struct { const void *Ginv, *Cd, *g; void *dz; } fz;   // set by the whole-solve entries: dz may ride in the PCG launch
    void *imgS, *imgP;                // column-major images of S and Pinv over all rows (one system; nullptr: none), see PcgLaunch::imgS
    int img_ld;
    int img_fresh;                    // the fused assembly launch of the whole solve in progress has just written them
    int no_image;                     // option: the one-workgroup kernels load from S_bd / P_bd as every other kernel
    int coop_launch;                  // option: multi-workgroup persistent launches through hipLaunchCooperativeKernel
    hipEvent_t host_ev[2];            // the host-pointer drop-in's timing events, kept across calls
    int dz_fused;                     // the most recent PCG launch also did the dz back-substitution (1: in the solving workgroup, 2: in helper blocks)
    int *dz_flag;                     // device word for the helper blocks of the one-workgroup fp64 launch
    int no_fuse_dz;                   // option
    unsigned long long **cl_tab;      // device copy of cl.peer (the kernel reads the peers' mirror addresses from it)
    struct {                          // the most recent whole-solve assembly, for gato_solve_rhs
        int valid;                    // S / Pinv / Ginv hold it (cleared by a stage entry that writes the workspace, a cluster set-up)
        const void *Cd;               // the C blocks it read: the solver's C_dense, or the caller's d_C_blocks of _blocks
        int img;                      // the fused launch also wrote the transposed images imgS / imgP
        unsigned long long gen;       // assemblies so far
    } as;
    char *rhs_ws;                     // re-solve work area: gamma [B][rhs_R][S K] (buffer 11) | iters [B][rhs_R]
    size_t rhs_ws_bytes;
    int rhs_R;                        // right-hand sides per system it has room for
    char *qp_ws;                      // box-QP work area (gato_box_qp_solve): G' | rho | x ping-pong | g~ | dz | lambda~ | slots | ...
    size_t qp_ws_bytes;               // only grows
    int *qp_pcg_total;                // in qp_ws: PCG iterations of every x-step of the latest QP solve, per system [B]
    char *pol_ws;                     // polish work area (gato_box_qp_polish; pdas_loop for every active-set entry; layouts: PolishWs, AlmWs in gato_qp_host.hip): g' | c' | dz' | lambda' | x, z, y polished | [act'] | [line search: xc | knot partials] | slots | counts | [gato_box_qp_alm: the inner runs' inputs and point, mu, its state and counts]
    size_t pol_ws_bytes;              // only grows
    char *cross_ws;                   // cross-term work area (gato_cross_host.hip): G' [B][G_dense] | C' [B][C_dense] | W [B][(K-1) S C] | g' [B][N]
    size_t cross_ws_bytes;            // only grows
    char *cross_rhs_ws;               // g' of the cross re-solves [B][R][N], apart from cross_ws: a growing R must not move the C' a live assembly reads
    size_t cross_rhs_ws_bytes;        // only grows
    struct {                          // the most recent cross whole solve, for gato_solve_rhs_cross
        int valid;
        unsigned long long gen;       // its as.gen: another assembly since then is not a cross one
    } cross;
    int qp_cross_unfused;             // option (measurement, tests): gato_box_qp_solve_cross runs cross_rhs and cross_finish as launches of their own around every re-solve and gives the update kernel W = 0
    int cross_csr_threads;            // option (measurement, tests): threads per workgroup of cross_prepare_csr_kernel, 64 or 256; 0: by the size of the launch; same bits
    int cross_tangent_form;           // option (measurement, tests): gato_kkt_tangent_rhs_cross stages the tangent blocks in LDS (1) or reads them in place (2); 0: by the size of the launch
};

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

inline bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    return cap != hipStreamCaptureStatusNone;
}

// false (error set): null solver, or a cluster rank asked for `unsupported` ("QP solves", "gradients": no sharded form)
bool solver_usable(const gato_solver *s, const char *entry, const char *unsupported);

// ---- launch planning (gato_plan.hip): the solver is only read, nothing is written -----------------------------------------
struct PcgGeometry { int groups, threads, kpw, pair, semi, dpp; bool cg1; };
// What one run of the internal PCG path takes in place of the options pcg_mode / true_warm_start / stamp_pcg (the public entries
// pass the options: pcg_opts).  warm is also a planner input: it rules out the ring and the single-reduction recurrence.
struct PcgOpts { int mode, warm, stamp; };
inline PcgOpts pcg_opts(const gato_solver &s) { return PcgOpts{s.pcg_mode, s.true_warm_start, s.stamp_pcg}; }
// K = knots the launch works on (the system's, or one rank's shard of it); batch = systems that would each want a workgroup of
// their own; plain_only = no one-workgroup special kernels (they have no cross-GPU level)
bool plan_resident(const gato_solver &s, const PcgOpts &o, int K, int batch, bool plain_only, PcgGeometry *geo);
bool plan_cg1(const gato_solver &s, int K, PcgGeometry *geo);
bool plan_one_wg_each(const gato_solver &s, const PcgOpts &o, int n);
bool cluster_plan(const gato_solver &s, const PcgOpts &o, int rank, PcgGeometry *geo);
bool cluster_plan_cg1(const gato_solver &s, const PcgOpts &o, PcgGeometry *geo, int *flat_total, int *flat_base);
bool cluster_plan_flat(const gato_solver &s, const PcgOpts &o, int *flat_total, int *flat_base);

// ---- PCG dispatch (gato_pcg_host.hip) ----------------------------------------------------------------------------------------
namespace gato {
extern std::mutex g_launch_mu;
int gate_before(int device, int num_cus, int need, hipStream_t st);
int gate_after(int device, int need, hipStream_t st);
}
// how a PCG over `batch` systems in one launch would run (mode: streaming or resident; g), or why it is refused; reads only
enum PcgRefusal { PCG_GO = 0, PCG_NO_FIT, PCG_NO_CAPTURE };
struct PcgDecision { int mode; PcgGeometry g; PcgRefusal refusal; };
PcgDecision pcg_decide(const gato_solver &s, const PcgOpts &o, int batch, bool capturing);
int pcg_one(gato_solver *s, const PcgOpts &o, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
            double exit_tol, int max_iters, int *d_iters, int batch, hipStream_t st, int rhs = 1);
int pcg_systems(gato_solver *s, const PcgOpts &o, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
                double exit_tol, int max_iters, int *d_iters, hipStream_t st);

// ---- whole solve and re-solve (gato_solve.hip) -------------------------------------------------------------------------------
// Assembly input of a whole solve: CSR (mode 0), dense blocks (mode 2), or dense blocks whose inverses are already in Ginv
struct AsmInput {
    int mode;
    const int *G_row, *G_col; const void *G_val; const int *C_row, *C_col; const void *C_val;
    const void *C_dense;              // the C blocks the Schur stage, the PCG's dz and a later re-solve read
    bool have_inv;                    // stage kernels only, G_dense and Ginv already written (gato_box_qp_polish)
};
int whole_solve(gato_solver *s, const PcgOpts &o, const AsmInput &in, const void *d_g, const void *d_c, double exit_tol,
                int max_iters, double rho, void *lam, void *dz, hipStream_t st);
int solve_rhs(gato_solver *s, const PcgOpts &o, int R, const void *d_g, const void *d_c, double exit_tol, int max_iters,
              void *d_lambda, void *d_dz, int *d_iters, hipStream_t st);
int pcg_rhs(gato_solver *s, const PcgOpts &o, int R, const void *gam, void *lam, double exit_tol, int max_iters, int *its, hipStream_t st);
int dz_rhs(gato_solver *s, int R, const void *g, const void *lam, void *dz, hipStream_t st);
int *rhs_iters(gato_solver *s);

// ---- cross term in the stage cost (gato_cross.hip; host side gato_cross_host.hip) ---------------------------------------------
struct CrossArgs {
    const void *G, *M, *Cd, *g;       // the caller's blocks (G without rho, C raw), M [B][(K-1) S C] and g [B][N]; never written
    void *Gp, *Cp, *W, *gp;           // the work area: G' (Q'' | R), C' (A^' | B^), W and g'
    double rho;
};
int cross_prepare(const Dims &d, int dtype, const CrossArgs &a, hipStream_t st);
int cross_rhs(const Dims &d, int dtype, int R, const void *W, const void *g, void *gp, hipStream_t st);      // g, gp [B][R][N]
int cross_finish(const Dims &d, int dtype, int R, const void *W, void *dz, hipStream_t st);                  // dz [B][R][N], in place
int cross_grad(const Dims &d, int dtype, const void *dz, const void *a, void *Mbar, hipStream_t st);
// The parts of cross_ws, as byte offsets: G' | C' | W | g'.  (gato_solver_buffer 13 .. 16 names them by the same sums.)
struct CrossWs { size_t G, C, W, g, bytes; };
// cross_prepare into the solver's work area (grown if need be; *o: its parts).  A recorded cross assembly is forgotten, and the
// assembly that read the area's C' (if any) is no longer the solver's.  who names the entry in errors.
int cross_prepare_ws(gato_solver *s, const char *who, const void *d_G, const void *d_M, const void *d_C, const void *d_g, double rho,
                     CrossWs *o, hipStream_t st);

// ---- CSR entry to the cross solve (gato_cross_csr.hip) ---------------------------------------------------
struct CrossCsrArgs {
    const int *G_row, *G_col, *C_row, *C_col;   // the pattern the B systems share; d.nnzG / d.nnzC values per system
    const void *G_val, *C_val, *g;          // never written
    void *Gp, *Cp, *W, *gp;                 // the work area, as CrossArgs
    void *G_out, *M_out, *C_out;            // optional: the scattered blocks [B][G_dense] (without rho), [B][(K-1) S C], [B][C_dense]
    double rho;
};
// threads: 64 or 256 per workgroup (same bits).  gato_cross_prepare_csr / gato_linsys_device_cross take 64 from
// CROSS_CSR_WAVE_KNOTS knots per compute unit on where S + C <= CROSS_CSR_WAVE_N (14/7, the largest shape at which one wave was
// measured the faster; 32/16 is not, nothing between them was measured) (option cross_csr_threads: 64 or 256 always).
constexpr int CROSS_CSR_WAVE_KNOTS = 8;
constexpr int CROSS_CSR_WAVE_N = 21;
int cross_prepare_csr(const Dims &d, int dtype, const CrossCsrArgs &a, int threads, hipStream_t st);
// gato_kkt_grad_csr with the cross entries of G (gato_grad.hip): a kept state-row entry carries M_bar at its slot
int grad_csr_cross(const Dims &d, int dtype, const int *G_row, const int *G_col, int nnzG, const int *C_row, const int *C_col, int nnzC,
                   const void *dz, const void *lam, const void *a, const void *beta, void *Gbar, void *Cbar, hipStream_t st);

// ---- tangent right-hand side of a cross solve (gato_tangent_cross.hip) ----------------------------------
struct CrossTangentArgs {
    const void *G_dot, *M_dot, *C_dot;      // [B][R][G_dense], [B][R][(K-1) S C], [B][R][C_dense]; nullptr: zero
    const void *g_dot, *c_dot;              // [B][R][N], [B][R][S K]; nullptr: zero
    const void *x, *lam;                    // the point [B][N], [B][S K], original variables
    const void *W;                          // the stored W of cross_ws [B][(K-1) S C]; read for gp only (K = 1: nullptr)
    void *tg, *gp, *tc;                     // t_g and the transformed g' [B][R][N] (either may be nullptr), t_c [B][R][S K]
};
// in_place: the tangent blocks are read where they lie instead of through LDS; same bits.  gato_kkt_tangent_rhs_cross stages them
// from CROSS_TANGENT_STAGE_WAVES waves per compute unit on (option cross_tangent_form: 1 always staged, 2 always in place).
constexpr int CROSS_TANGENT_STAGE_WAVES = 3;
int cross_tangent_rhs(const Dims &d, int dtype, int R, const CrossTangentArgs &a, bool in_place, hipStream_t st);

// ---- ADMM update of a box QP with a cross term (gato_qp_cross.hip) -------------------------------------
struct QpCrossArgs {
    QpArgs q;                         // as qp_update_kernel takes it: G, Cd the caller's; xt the x-step's solution in (x, v); gt is written transformed
    const void *M, *W;                // the caller's M and the stored W of cross_ws, [B][(K-1) S C] each
};
int qp_update_cross(const Dims &d, int dtype, const QpCrossArgs &a, int it, int last, hipStream_t st);
