/* gato_hip.h - C ABI of the MI355X-native gato PCG / Schur hot path (libgato_hip.so).
 *
 * Drop-in boundary: these entry points are what the reference's binding layer would call
 * instead of its CUDA driver.  Every function cites the reference interface it replaces
 * (file:line relative to the reference checkout).  Plain pointers and sizes only; no torch
 * or pybind11 types.  All functions return 0 on success or a negative GATO_E* code, and
 * gato_last_error() gives the message (the reference prints "GPUassert" and exit()s,
 * include/gato_defines.h:42-51).
 *
 * Conventions:  S = STATE_SIZE, C = CONTROL_SIZE, K = KNOT_POINTS (runtime here; compile-time
 * macros in the reference, CMakeLists.txt:18), n = S+C, N = n*K - C.
 * dtype: GATO_F32 (the reference's only arithmetic type) or GATO_F64.  `void*` data pointers
 * are float* or double* according to the solver's dtype.  Device layouts are the reference's:
 *   G_dense : per knot [Q_k S*S | R_k C*C] col-major, last knot Q only  ((S*S+C*C)*K - C*C elems, gato_defines.h:36)
 *   C_dense : per knot k<K-1 [A_k S*S | B_k S*C] col-major              ((S*S+S*C)*(K-1) elems, gato_defines.h:37)
 *   S, Pinv : per block-row [left|main|right], each S*S col-major       (3*S*S*K elems, gato_utils.cuh:44-73)
 *   gamma, lambda : S*K ; g, dz : N ; c : S*K
 * `stream` is a hipStream_t passed as void* (NULL = default stream, as the reference uses,
 * gato_defines.h:22).
 */
#ifndef GATO_HIP_H
#define GATO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GATO_F32 0
#define GATO_F64 1

#define GATO_OK 0
#define GATO_EINVAL (-1)   /* bad argument / shape mismatch */
#define GATO_ESHAPE (-2)   /* (S,C) has no compiled instantiation */
#define GATO_EHIP (-3)     /* HIP runtime error */
#define GATO_ENODEV (-4)   /* no usable GPU */
#define GATO_ETIMEOUT (-5) /* in-kernel hand-off timed out (persistent PCG) */

/* PCG kernel selection (gato_pcg.cuh:505-553 picks K4 vs K5 by co-residency, check_sms) */
#define GATO_PCG_AUTO 0
#define GATO_PCG_RESIDENT 1  /* A5: matrices register-resident for the whole solve, one persistent launch */
#define GATO_PCG_STREAMING 2 /* A6: matrices re-read from HBM every iteration, two launches per iteration */

/* Preconditioner of the whole-solve entries = the reference's compile switches BLOCK_J_PRECON / SS_PRECON
 * (include/gato_defines.h:9-10; src/gato_schur.cuh:407-429,965-970), a runtime option here ("precon_mode"). */
#define GATO_PRECON_STAIR 0        /* both 1 (the reference's setting): 3-band symmetric stair */
#define GATO_PRECON_BLOCK_JACOBI 1 /* SS_PRECON 0: main blocks -theta^-1 only */
#define GATO_PRECON_POINT_JACOBI 2 /* both 0: diag(1 / S.main_ii) */

/* Threads: a gato_solver is used by one host thread at a time (its plan, counters and work buffers are per solver); different
 * solvers may be driven from different threads and streams concurrently - the process-wide state (the admission of persistent
 * multi-workgroup launches to the chip, the cached solver of gato_linsys_solve_*, the mirror pool) is locked, gato_last_error is
 * per thread. */
typedef struct gato_solver gato_solver;

/* ---- library / device ------------------------------------------------------------------- */
const char *gato_last_error(void);
int gato_version(void);
/* Number of (S,C) instantiations compiled in, and the i-th one. */
int gato_num_shapes(void);
int gato_shape(int i, int *S, int *C);
/* Replaces check_sms (gato_utils.cuh:829-854): device properties needed to size the grids. */
int gato_device_info(int device, int *num_cus, int *lds_bytes, char *name, int name_len);

/* Infers (S,C,K) from the lengths of the linsys_solve arguments (the reference gets them from
 * -DSTATE_SIZE/-DCONTROL_SIZE/-DKNOT_POINTS, install.bash:6-16): S*K = len_c, N = len_g, and
 * S = number of leading single-entry identity rows of C (row-block 0 of C, gato_schur.cuh:725). */
int gato_infer_shape(const int *C_row, int len_C_row, int len_g, int len_c, int *S, int *C, int *K);

/* ---- solver object: owns the device workspace the reference allocates per call
 * (gpu_library.cu:36-45, gato_pcg.cuh:486-492) -------------------------------------------- */
int gato_solver_create(int S, int C, int K, int dtype, int device, gato_solver **out);
/* Batch of B independent systems of one shape and one sparsity pattern (new - the
 * reference solves one system per call, its `testiters` loop re-solves the same one, gpu_library.cu:169).
 * Every per-system device array of the stage-level calls is then B arrays back to back; the CSR structure
 * (indptr/indices) is shared, G_val / C_val hold nnz entries per system.  All stages run the whole batch
 * in one launch each (grid.y = system); the PCG runs one workgroup per system when a system fits one CU. */
int gato_solver_create_batched(int S, int C, int K, int B, int dtype, int device, gato_solver **out);
int gato_solver_destroy(gato_solver *s);
/* Workspace device pointers (valid for the solver's lifetime), for stage-level tests:
 * which: 0 G_dense, 1 C_dense, 2 Ginv_dense, 3 S, 4 Pinv, 5 gamma, 6 lambda, 7 dz, 8 iters(int),
 * 10 eta history (double[max_iters+1]: eta = r.Pinv r after the initial step and after every iteration; filled when
 * option record_eta = 1 and max_iters <= 4096 - the reference only prints it under DEBUG_MODE, gato_pcg.cuh:397-400),
 * 11 gamma of the re-solves (gato_solve_rhs: its first B*R*S*K entries are [B][R][S*K] of the latest re-solve of R
 * right-hand sides; NULL before gato_solver_reserve_rhs or the first re-solve),
 * 13 .. 16 the cross-term work area (gato_linsys_device_blocks_cross): G' [B][G_dense], C' [B][C_dense], W [B][(K-1)*S*C],
 * g' [B][N]; NULL before the first cross call */
void *gato_solver_buffer(gato_solver *s, int which);
/* Options: pcg_mode (GATO_PCG_*), pcg_threads (0 = auto; threads per workgroup of the resident
 * kernel), pcg_groups (0 = auto; workgroups of the resident kernel), true_warm_start (0 = the
 * reference's behaviour: lambda restarts from zero, gato_pcg.cuh:303; 1 = d_lambda of gato_pcg /
 * gato_linsys_device is read as the initial guess, r0 = gamma - S lambda0), pcg_variant (0 = the reference's PCG
 * recurrence; 1 = opt-in single-reduction Chronopoulos-Gear recurrence of the multi-workgroup and the cluster launches: one
 * inter-workgroup / cross-GPU exchange per iteration instead of two, same solution to solver tolerance, different rounding),
 * coop_launch (1 = the multi-workgroup resident / semi-resident launches through hipLaunchCooperativeKernel - what the
 * reference does, gato_pcg.cuh:502-526 - so that the runtime guarantees their co-residency beside kernels of other streams
 * and processes; +17 us per launch, default 0; the single-reduction kernel and the LDS-DMA ring keep the plain launch),
 * xcd_pack (-1 auto:
 * launches of up to 32 workgroups are placed on one XCD - a placement hint, never needed for correctness; 0 off),
 * xcd_sel (which of the eight XCDs hosts such a launch: -1 = measured once per solver and geometry with a millisecond of
 * trial launches before the first one, 0..7 fixed; read-only last_xcd_sel),
 * asm_mode (whole-solve entries: 0 = auto - convert + Schur + stair as ONE fused launch when K*B <= 2 x CUs, the
 * stage kernels otherwise; 1 = stage kernels; 2 = fused; both give bit-identical buffers), pcg_semi (-1 = auto: K
 * beyond the register file runs as one persistent launch - semi-resident, or with the block rows streamed through an
 * LDS-DMA ring once the matrices one launch streams are far beyond the Infinity Cache (measured cross-overs: 450 MB of S + Pinv
 * in fp32, 550 MB in fp64, 700 MB at STATE_SIZE 32); 0 = the streaming kernels; 1 / 2 / 3 force the
 * semi-resident launch with / without resident rows / the LDS-DMA ring), time_pcg (record
 * hipEvents around the PCG launch), time_stages (hipEvents around assembly / PCG / dz of the whole-solve entries),
 * precon_mode (GATO_PRECON_*), knot_lo / knot_hi (the stage-level entries gato_convert / gato_form_schur / gato_form_ss /
 * gato_compute_dz then work on the knots [knot_lo, knot_hi) only - a rank of a multi-GPU solve assembles just what its
 * PCG shard reads; reset by every whole-solve call), timeout_ms (bound of every in-kernel spin, default 2000), max_workgroups (CUs a
 * persistent launch may count on; 0 = all of the device), no_single_lds / stamp_pcg (1 = kernel build with cycle stamps and the
 * timing-only switches of `ablate`, 2 = the switches alone) / stamp_asm / ablate (diagnostics). */
int gato_solver_set_option(gato_solver *s, const char *name, int value);
int gato_solver_get_option(gato_solver *s, const char *name, int *value);

/* ---- stage-level entry points on DEVICE pointers (one per reference launch wrapper) ------ */
/* A1  form_schur's first launch, gato_convert_kkt_format (gato_schur.cuh:745-756, :902).
 * Zeroes G_dense/C_dense itself (the reference relies on cuda_calloc, gpu_library.cu:36-37). */
int gato_convert(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val,
                 const int *d_C_row, const int *d_C_col, const void *d_C_val, double rho,
                 void *d_G_dense, void *d_C_dense, void *stream);
/* A2  gato_form_schur_jacobi (gato_schur.cuh:462-494, :942).  Writes S (left, main, right),
 * Pinv.main, gamma and the inverses Q^-1,R^-1 into d_Ginv_dense (separate buffer; the
 * reference overwrites d_G_dense in place, :238-259, racing with its neighbours - D3). */
int gato_form_schur(gato_solver *s, const void *d_G_dense, const void *d_C_dense, const void *d_g,
                    const void *d_c, void *d_S, void *d_Pinv, void *d_gamma, void *d_Ginv_dense,
                    void *stream);
/* A3  gato_form_ss (gato_schur.cuh:652-670, :967): Pinv.left / Pinv.right. */
int gato_form_ss(gato_solver *s, const void *d_S, void *d_Pinv, void *stream);
/* A4-A8  solve_pcg<T> (gato_pcg.cuh:476-567).  lambda is reset to 0 (D5: warm_start is a no-op in
 * the reference, gato_pcg.cuh:303).  d_iters receives the reference's iteration count (index of
 * the iteration that met |eta| < exit_tol, else max_iters; gato_pcg.cuh:311-313,:406-408; -1 = a hand-off of a
 * persistent launch timed out, see gato_pcg_status).  Asynchronous on `stream`: enqueue only - no host wait, no
 * trial launches, nothing but d_lambda / d_iters written for the caller (checked by
 * tests/test_gpu_parity.py::test_pcg_entry_is_enqueue_only). */
int gato_pcg(gato_solver *s, const void *d_S, const void *d_Pinv, const void *d_gamma,
             void *d_lambda, double exit_tol, int max_iters, int *d_iters, void *stream);
/* Placement of the one-XCD persistent launches (2..32 workgroups; replaces nothing in the reference - its cooperative
 * launch, gato_pcg.cuh:502-526, has no notion of placement): measures once which of the eight XCDs hosts the geometry the
 * solver's CURRENT options plan (16 short trial launches on solver-owned scratch buffers, each waited for: BLOCKING,
 * ~1 ms).  gato_solver_create calls it for the default geometry (env GATO_NO_TUNE=1 skips that); call it again after
 * changing pcg_threads / pcg_groups / pcg_variant / max_workgroups / xcd_pack.  A geometry that was never measured runs
 * on XCD 0; results never depend on the placement.  No-op for batches, cluster ranks and other geometries. */
int gato_solver_tune(gato_solver *s, void *stream);
/* Hand-off time-outs (the workgroups of a persistent launch were not co-resident - the case the reference excludes
 * with cudaLaunchCooperativeKernel + check_sms, gato_pcg.cuh:502-526, gato_utils.cuh:829-854): the launch writes
 * iters = -1 (in-band, no second call needed) and the id of the launch into the solver's status word, which no kernel
 * ever clears.  gato_pcg_status synchronises the stream of the latest PCG launch and returns GATO_ETIMEOUT if ANY
 * launch timed out since the previous call (*status = 1), else GATO_OK.  Option timeout_ms bounds every spin (2000). */
int gato_pcg_status(gato_solver *s, int *status);
/* The fallback: if a persistent launch of the most recent gato_linsys_device / _blocks call timed out, re-run its PCG
 * through the streaming kernels (no in-launch hand-off, any residency) and recompute dz into the same output buffers -
 * a slower correct answer instead of an error.  Synchronises `stream`; *recovered = 1 if that happened.  Multi-
 * workgroup launches of one process never get there by themselves: a launch that does not fit beside those still in
 * flight on other streams waits for them (per-device CU budget). */
int gato_solver_recover(gato_solver *s, int *recovered, void *stream);
/* Device time of the most recent PCG launch(es) of gato_pcg, measured with hipEvents recorded on the
 * launch stream immediately around the kernel launch(es) (the reference times whole solves with
 * cudaEvents, gpu_library.cu:167-187).  Enabled by option "time_pcg" = 1; synchronises on the stop event. */
int gato_pcg_last_ms(gato_solver *s, float *ms);
/* Stage times of the most recent gato_linsys_device / _blocks call as data (the reference prints them:
 * "Forming Schur took", gato_schur.cuh:907-913,972-982; solve time gpu_library.cu:186-198): ms[0] = scatter + Schur +
 * preconditioner, ms[1] = PCG, ms[2] = dz.  Enabled by option "time_stages" = 1. */
int gato_last_stage_ms(gato_solver *s, float *ms);
/* A9  compute_dz (gato_schur.cuh:1012-1022) with d_Ginv_dense = inverses from gato_form_schur. */
int gato_compute_dz(gato_solver *s, const void *d_Ginv_dense, const void *d_C_dense, const void *d_g,
                    const void *d_lambda, void *d_dz, void *stream);

/* ---- A13  gato_linsys (gpu_library.cu:25-83) on DEVICE CSR inputs: convert, Schur, stair,
 * PCG, dz, all on `stream`, into the solver's workspace; d_lambda/d_dz may be NULL (results stay
 * in the workspace, gato_solver_buffer 6/7).  Asynchronous. */
int gato_linsys_device(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val,
                       const int *d_C_row, const int *d_C_col, const void *d_C_val,
                       const void *d_g, const void *d_c, double exit_tol, int max_iters, double rho,
                       void *d_lambda, void *d_dz, void *stream);

/* Batched gato_linsys_device (solver from gato_solver_create_batched): d_G_val[B][nnz_G], d_C_val[B][nnz_C],
 * d_g[B][N], d_c[B][S*K] -> d_lambda[B][S*K], d_dz[B][N], d_iters[B]. */
int gato_linsys_device_batched(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, int nnz_G,
                               const int *d_C_row, const int *d_C_col, const void *d_C_val, int nnz_C,
                               const void *d_g, const void *d_c, double exit_tol, int max_iters, double rho,
                               void *d_lambda, void *d_dz, int *d_iters, void *stream);

/* ---- L4  main_call (gpu_library.cu:85-234) on HOST pointers: H2D of the CSR, `testiters`
 * timed repeats of the whole solve, D2H of lambda and dz.  ms_out[testiters] (may be NULL)
 * receives the per-repeat time the reference prints (gpu_library.cu:186-198).
 * lambda_in is read only when warm_start != 0 and then ignored by the PCG exactly as the
 * reference does (D5). */
int gato_linsys_solve_f32(const int *G_row, int len_G_row, const int *G_col, const float *G_val, int nnz_G,
                          const int *C_row, int len_C_row, const int *C_col, const float *C_val, int nnz_C,
                          const float *g, int len_g, const float *c, int len_c, const float *lambda_in,
                          int S, int C, int K, int testiters, float exit_tol, int max_iters,
                          int warm_start, float rho, float *lambda_out, float *dz_out,
                          int *iters_out, float *ms_out);
/* The host entries keep the solver and staging buffers of the most recent (S, C, K, dtype) for the next call;
 * gato_release_cache() frees them (optional; e.g. before unloading the library). */
int gato_release_cache(void);
int gato_linsys_solve_f64(const int *G_row, int len_G_row, const int *G_col, const double *G_val, int nnz_G,
                          const int *C_row, int len_C_row, const int *C_col, const double *C_val, int nnz_C,
                          const double *g, int len_g, const double *c, int len_c, const double *lambda_in,
                          int S, int C, int K, int testiters, double exit_tol, int max_iters,
                          int warm_start, double rho, double *lambda_out, double *dz_out,
                          int *iters_out, float *ms_out);

/* ---- knot-sharded PCG across GPUs (NEW work: the reference is single-device, gato_utils.cuh:831,
 * and has no communication library).  One process per GPU; rank r owns block
 * rows [k0,k1) of S / Pinv (contiguous, in rank order) and keeps the full gamma.  Per PCG iteration each
 * rank runs two launches of the streaming kernel on its shard and exchanges one fixed-size RECORD after
 * each:  record = [partial dot | first S-block | last S-block] of the vector just produced (2S+1
 * elements of the solver dtype).  The caller all-gathers the records of all ranks (RCCL
 * all_gather over xGMI; gloo in the CPU tests) and hands the gathered array [nranks][2S+1] to the next
 * call - that one collective carries both the global dot (summed in rank order: deterministic) and the
 * neighbour halos.  Ghost blocks of r and p are advanced locally from the neighbours' upsilon / r~
 * blocks, so there are exactly two collectives per iteration and no host synchronisation.
 *   init    : r = gamma, lambda = 0, r~ = Pinv r                       -> send = record(r.r~ , r~)
 *   phase_a : p = r~ + beta p, upsilon = S p      (needs gathered B records of it-1 and it-2 / init)
 *                                                                      -> send = record(p.upsilon, upsilon)
 *   phase_b : lambda += alpha p, r -= alpha upsilon, r~ = Pinv r  (needs gathered B record of it-1 / init
 *             and the gathered A record of this iteration)              -> send = record(r.r~, r~)
 *   finish  : last exit test; d_lambda_full_out (S*K_total) = own slice of lambda, zero elsewhere
 *             (sum-all-reduce it to assemble lambda); d_iters as gato_pcg.
 * S/Pinv/gamma pointers are FULL-system arrays (block row 0 first); all pointers are device pointers. */
int gato_shard_pcg_init(gato_solver *s, int rank, int nranks, int k0, int k1, const void *d_S, const void *d_Pinv,
                        const void *d_gamma, double exit_tol, int max_iters, void *d_send, void *stream);
int gato_shard_pcg_phase_a(gato_solver *s, int it, const void *d_recvB_cur, const void *d_recvB_prev, void *d_send,
                           void *stream);
int gato_shard_pcg_phase_b(gato_solver *s, int it, const void *d_recvB_cur, const void *d_recvA, void *d_send,
                           void *stream);
int gato_shard_pcg_finish(gato_solver *s, const void *d_recvB_last, void *d_lambda_full_out, int *d_iters,
                          void *stream);
/* Host-side convergence poll between iterations (synchronises `stream`): *done = 1 once the exit test has fired.
 * Every rank computes the same sums, so every rank reads the same value. */
int gato_shard_pcg_done(gato_solver *s, int *done, void *stream);

/* ---- multi-GPU cluster: the persistent PCG launch with a device-initiated cross-GPU hand-off (NEW work, SURVEY.md
 * section 8e; replaces the reference's grid barriers gato_pcg.cuh:363,378,393,428 across GPUs).  One process per
 * GPU.  Rank r owns the balanced contiguous knot range gato_cluster_knot_range gives and a MIRROR (a few KB of
 * fine-grained device memory) that the peers write with system-scope stores over xGMI: per hand-off the rank's total
 * goes into every rank's mirror and the rank's boundary blocks into the neighbours'; a rank polls only its own
 * mirror.  Two hand-offs per iteration, no host involvement, no collective library inside the loop.  While the cluster
 * has at most 256 workgroups in all the exchange is flat (every workgroup's partial straight into every mirror, option
 * cluster_flat = 1, default); larger clusters gather inside each GPU first, then across GPUs.
 *   gato_cluster_create   allocates and zeroes the mirror, returns its 64-byte hipIpcMemHandle_t in ipc_handle_out
 *   gato_cluster_connect  ipc_handles = nranks x 64 bytes in rank order (all-gathered by the caller), and / or
 *                         ptrs[r] = the mirror of a rank living in THIS process (gato_cluster_local_mirror);
 *                         afterwards every rank must pass a host barrier before the first gato_cluster_pcg
 *   gato_cluster_pcg      this rank's part of one solve: full-system S / Pinv / gamma / lambda arrays, of which only
 *                         the rows of the rank's range are read / written; same exit_tol and max_iters on every
 *                         rank; asynchronous; d_iters as gato_pcg (-1: a hand-off timed out, on every rank alike).
 *                         Option pcg_variant = 1 on EVERY rank: the single-reduction recurrence - ONE cross-GPU exchange per
 *                         iteration instead of the reference's two reductions (gato_pcg.cuh:353-394); the ranks then also
 *                         read Pinv on the knots k0-1, k1 and gamma on k0-2..k1+1.  On return lambda also holds the right
 *                         neighbour's first block at row k1 (it arrives inside the launch): what dz of knot k1-1 needs
 *                         (gato_schur.cuh:833-838).  Option true_warm_start = 1: lambda0 is read from the rank's OWN rows of
 *                         d_lambda only (k0..k1-1); the neighbouring ranks' boundary blocks of lambda0 cross inside the launch
 *                         (one hand-off more), so the other rows may hold anything, NaN included
 *   gato_cluster_linsys   this rank's part of a WHOLE solve (gato_linsys, gpu_library.cu:25-83): stage kernels on the knots
 *                         its shard reads, gato_cluster_pcg, dz on its range - nothing crosses the host or a collective in
 *                         between; inputs replicated, d_lambda / d_dz full-length arrays of which the rank's rows are written;
 *                         with true_warm_start lambda0 is read from rows k0..k1-1 of d_lambda only, as in gato_cluster_pcg */
int gato_cluster_knot_range(int K, int rank, int nranks, int *k0, int *k1);
int gato_cluster_create(gato_solver *s, int rank, int nranks, void *ipc_handle_out);
void *gato_cluster_local_mirror(gato_solver *s);
int gato_cluster_connect(gato_solver *s, const void *ipc_handles, void *const *ptrs);
/* Workgroups x threads this rank's launch would use; 0 x 0: its knots do not fit one persistent launch on this GPU
 * (the caller then takes the gato_shard_pcg_* schedule on every rank). */
int gato_cluster_fits(gato_solver *s, int *groups, int *threads);
int gato_cluster_pcg(gato_solver *s, const void *d_S, const void *d_Pinv, const void *d_gamma, void *d_lambda,
                     double exit_tol, int max_iters, int *d_iters, void *stream);
int gato_cluster_linsys(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, const int *d_C_row,
                        const int *d_C_col, const void *d_C_val, const void *d_g, const void *d_c, double exit_tol,
                        int max_iters, double rho, void *d_lambda, void *d_dz, int *d_iters, void *stream);
int gato_cluster_destroy(gato_solver *s);
/* The hand-off epochs of a cluster only grow (32 bits; a launch takes 2 max_iters + 8 on every rank alike: about ten million
 * 200-iteration solves).  gato_cluster_launches_left: how many launches with this max_iters still fit (the same number on every
 * rank).  When it reaches 0 the caller renews the epoch space on EVERY rank at the same solve: wait for the rank's own launches,
 * host barrier over the ranks, gato_cluster_rewind (zeroes the mirror and the level-1 slots, counters back to 0), second barrier.
 * gato_cluster_pcg / gato_cluster_linsys refuse a launch that does not fit (GATO_EINVAL). */
int gato_cluster_launches_left(gato_solver *s, int max_iters, long long *left);
int gato_cluster_rewind(gato_solver *s);

/* ---- re-solve for new right-hand sides (new; the reference rebuilds the system on every call): the matrices of the most
 * recent whole solve stay in the workspace - Ginv, S, Pinv, the transposed images - and a re-solve takes R new (g, c) per
 * system against them: gamma = c - C G^-1 g (one launch), the PCG, dz.  No gather, inversion, Schur, stair or point-Jacobi
 * kernel runs, and no matrix buffer of the solver is written.
 * What counts as an assembly: a successful gato_linsys_device / _blocks / _batched (and gato_linsys_solve_* through it).
 * After _blocks the re-solve reads the caller's d_C_blocks again: keep them unchanged until the next whole solve.
 * What invalidates it: gato_convert / gato_form_schur / gato_form_ss given any of the solver's own buffers
 * (gato_solver_buffer) as an output, and gato_cluster_create.  The preconditioner is the one the assembly built. */
/* Read-only options: assembly_valid (1 while a re-solve has an assembly to read), assembly_gen (whole-solve assemblies so far,
 * one per successful whole solve, none per re-solve; an int that wraps - compare for equality only).
 * gato_box_qp_solve assembles its own x-step matrix once per call: a re-solve after it re-solves that matrix. */
/* Reserve the re-solve work area (gamma, iters) for up to R right-hand sides per system.  Blocking (waits for the device
 * when it grows); only grows. */
int gato_solver_reserve_rhs(gato_solver *s, int R);
/* Re-solve the most recent whole-solve assembly of `s` for R new right-hand sides per system.
 * Layouts (B = batch): d_g [B][R][N], d_c [B][R][S*K] -> d_lambda [B][R][S*K], d_dz [B][R][N], d_iters [B][R] (NULL: the
 * work area's).  Option true_warm_start = 1: d_lambda is also the initial guess.  Asynchronous on `stream`, enqueue only;
 * beyond the reserved R it first grows the work area (blocking) - under stream capture that is refused, as is a persistent
 * launch of several workgroups (see gato_pcg).  Returns GATO_EINVAL, enqueueing nothing, without a valid assembly, for
 * R < 1, B*R > 65535 and on a cluster rank.  Options time_stages (ms[0] = gamma, ms[1] = PCG, ms[2] = dz), last_image,
 * last_dz_fused report the re-solve; gato_solver_recover re-runs its PCGs through the streaming kernels. */
int gato_solve_rhs(gato_solver *s, int R, const void *d_g, const void *d_c, double exit_tol, int max_iters,
                   void *d_lambda, void *d_dz, int *d_iters, void *stream);
/* List-level face: re-solve the system of the most recent gato_linsys_solve_f32 / _f64 (the cached solver, same precision)
 * for a new g (len N) and c (len S*K); blocking, host pointers.  GATO_EINVAL if there is no such system (none yet, released,
 * the other precision) or the lengths differ. */
int gato_linsys_resolve_f32(const float *g, int len_g, const float *c, int len_c, float exit_tol, int max_iters,
                            float *lambda_out, float *dz_out, int *iters_out);
int gato_linsys_resolve_f64(const double *g, int len_g, const double *c, int len_c, double exit_tol, int max_iters,
                            double *lambda_out, double *dz_out, int *iters_out);

/* ---- gradients of a solve (new): the backward pass of M [dz; lambda] = [g; c], M = [[G + rho I, C^T],
 * [C, 0]].  The caller has the forward's dz, lambda and the adjoint [a; beta] = M^-1 [dz_bar; lambda_bar] - a re-solve of the
 * same assembly (gato_solve_rhs with g = dz_bar, c = lambda_bar: M is symmetric); g_bar = a, c_bar = beta.  These entries form
 * the matrix gradients from the four vectors alone (no assembly is read, none is needed), asynchronously on `stream`:
 *   Q_bar_k = -1/2 (a_x,k dz_x,k^T + dz_x,k a_x,k^T), R_bar_k likewise on the u-parts (the gradient for symmetric perturbations
 *   of Q_k, R_k - the solver treats them as symmetric),  A_bar_k = -(beta_k+1 dz_x,k^T + lambda_k+1 a_x,k^T),
 *   B_bar_k = -(beta_k+1 dz_u,k^T + lambda_k+1 a_u,k^T)  (A_k, B_k as stored in C_dense: the raw values of C).
 * Layouts (B = batch): d_dz, d_adz [B][N]; d_lam, d_alam [B][S*K].  GATO_EINVAL for a NULL vector, both outputs NULL, and on a
 * cluster rank. */
/* d_Gbar [B][G_dense] and d_Cbar [B][C_dense] in the dense layouts; either may be NULL (skipped). */
int gato_kkt_grad_blocks(gato_solver *s, const void *d_dz, const void *d_lam, const void *d_adz, const void *d_alam,
                         void *d_Gbar, void *d_Cbar, void *stream);
/* The same gradient per value of a CSR pattern the B systems share (as gato_linsys_device_batched takes them): d_Gbar_val
 * [B][nnz_G], d_Cbar_val [B][nnz_C], either may be NULL.  The exact chain rule through the scatter: an entry gets the block
 * gradient of the dense slot it is written into - bit for bit what gato_kkt_grad_blocks gives there - and 0 when the scatter
 * drops it (block row 0 of C, C columns beyond the block row) or a later entry of its row writes the same slot. */
int gato_kkt_grad_csr(gato_solver *s, const int *d_G_row, const int *d_G_col, int nnz_G, const int *d_C_row, const int *d_C_col,
                      int nnz_C, const void *d_dz, const void *d_lam, const void *d_adz, const void *d_alam, void *d_Gbar_val,
                      void *d_Cbar_val, void *stream);

/* ---- box-constrained QP solves (new): per system b of the batch
 *     min 1/2 x^T H x - g^T x   s.t.  C x = c,  lo <= x <= hi,      H = G + rho I
 * by ADMM (the OSQP splitting, the dynamics kept as hard equality constraints) over the re-solve.  The x-step matrix
 * [[H + sigma I + diag(rho_i), C^T], [C, 0]] is assembled ONCE per call: gato_linsys_device_blocks on G + diag(sigma + rho_i),
 * with rho_i = 0 on free variables (both bounds infinite), 1e3 admm_rho where lo_i == hi_i, admm_rho otherwise.  Every later
 * iteration is one gato_solve_rhs with lambda warm from the previous x-step plus one update launch (relaxation alpha,
 * projection onto the box, dual update, next right-hand side and the true QP residuals).  With all bounds infinite the
 * solution is the dz / lambda of gato_linsys_device_blocks.
 * Inputs: d_G_blocks [B][G_dense] WITHOUT rho and d_C_blocks [B][C_dense] (raw values, as _blocks takes them), d_g, d_lo, d_hi
 * [B][N] (dz layout; +-inf allowed), d_c [B][S*K].  Outputs: d_x, d_z, d_y [B][N], d_lambda [B][S*K], d_iters, d_status [B],
 * d_res [B][2] = (r_prim, r_dual) of the returned iterate:
 *     r_prim = max(|x - z|inf, |C x - c|inf),   r_dual = |H x - g + C^T lambda + y|inf
 * converged when r_prim <= eps_abs + eps_rel max(|x|, |z|, |c|) and r_dual <= eps_abs + eps_rel max(|H x|, |C^T lambda|, |y|, |g|).
 * y is the multiplier of the box: > 0 at an active upper bound, < 0 at an active lower bound.  iters = the x-steps whose result
 * is returned.  Status: GATO_QP_CONVERGED, _MAX_ITERS, _NONFINITE (a residual is NaN or inf); there is no infeasibility
 * detection (an infeasible box ends in MAX_ITERS).  warm = 1: d_z, d_y, d_lambda are also read as the start (z0 = clip(z),
 * y0 = y with 0 on free variables, lambda seeds the first PCG); warm = 0: z0 = clip(0), y0 = 0, a cold first PCG.
 * Blocking: the host reads the count of live systems every check_every iterations; a converged system is frozen - never
 * written again - so the results are bit-identical for every check_every.  The solver's true_warm_start option is set for the
 * call's own solves and restored.  GATO_EINVAL, nothing enqueued, for a captured stream, a cluster rank, a NULL pointer or a
 * parameter out of range; GATO_EINVAL after the prepare launch if a bound is NaN or lo > hi (d_status = GATO_QP_BAD_BOUNDS
 * names those systems; the other outputs are undefined).
 * Side effect: afterwards the solver's assembly is the QP's x-step matrix - assembly_gen advances by exactly one per call and a
 * later gato_solve_rhs re-solves that matrix, not the caller's G + rho I.  Buffer 12 (gato_solver_buffer) holds the PCG
 * iterations of all x-steps of the latest call, per system [B] (int). */
#define GATO_QP_CONVERGED 0
#define GATO_QP_MAX_ITERS 1
#define GATO_QP_NONFINITE 2
#define GATO_QP_BAD_BOUNDS 3
typedef struct {
    double rho, admm_rho, sigma, alpha, eps_abs, eps_rel, exit_tol;
    int max_iters, max_admm_iters, check_every, warm;
} gato_box_qp_params;
/* admm_rho 0.1, sigma 1e-6, alpha 1.6, eps_abs = eps_rel = 1e-6, max_admm_iters 4000, check_every 25, warm 0; rho 0 and
 * PCG exit_tol 1e-6 / max_iters 100 (set them as for a whole solve) */
void gato_box_qp_default_params(gato_box_qp_params *p);
int gato_box_qp_solve(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                      const void *d_lo, const void *d_hi, const gato_box_qp_params *p, void *d_x, void *d_z, void *d_y,
                      void *d_lambda, int *d_iters, int *d_status, double *d_res /* [B][2] */, void *stream);

/* ---- solution polishing of a box QP and gradients through the polished solution (new) ----------
 * The active set of an ADMM result (OSQP's rule): d_act [B][N] int8, +1 where hi - z < y (upper bound), -1 where
 * z - lo < -y (lower bound) and wherever lo == hi, 0 otherwise and always on the S states of x_0.  An infinite bound is never
 * active.  Asynchronous on `stream`.  GATO_EINVAL for a NULL pointer and on a cluster rank. */
int gato_box_qp_active_set(gato_solver *s, const void *d_z, const void *d_y, const void *d_lo, const void *d_hi, signed char *d_act,
                           void *stream);
/* Polish: the exact KKT solution of the QP with the variables of d_act fixed at their bounds (x_A = the bounds bit for bit,
 * x_F from the reduced system [[H_FF, C_F^T], [C_F, 0]] - one assembly on the stage kernels, one PCG, one dz - and the bound
 * multipliers y_A = (g - H x - C^T lambda)_A, y_F = 0).  The polished point (x, z = clip(x, lo, hi), y, lambda) is accepted
 * iff every value is finite, it passes the termination test of gato_box_qp_solve with p's eps_abs and eps_rel, and every
 * active multiplier has its sign within the dual tolerance (y >= -tol at an upper bound, <= tol at a lower one, any sign
 * where lo == hi).  An accepted system's d_x, d_z, d_y, d_lambda and d_res are replaced and d_status becomes
 * GATO_QP_CONVERGED; a rejected one is not written, bit for bit.  d_polish [B] gets the GATO_QP_POLISH_* code per system.
 * Inputs as gato_box_qp_solve takes them (G without rho); of p only rho, exit_tol, max_iters (the PCG), eps_abs and eps_rel
 * are read.  The reduced system needs C_F of full row rank (LICQ): a degenerate active set ends in NONFINITE or REJECTED.
 * Blocking.  GATO_EINVAL, nothing enqueued, for a captured stream, a cluster rank, a NULL pointer or a parameter out of range;
 * GATO_EINVAL after the prepare launch if an act is not -1, 0 or 1, names an infinite bound or a state of x_0 (d_polish =
 * GATO_QP_POLISH_BAD_ACTIVE names those systems, -1 the others; no output is written and the solver has no assembly).
 * Side effect: a whole-solve assembly - assembly_valid = 1, assembly_gen advances by one - of the REDUCED system: a later
 * gato_solve_rhs re-solves it (its dz is 0 on the active set), which is the adjoint of the backward pass.  The solver's
 * true_warm_start option is set to 0 for the call's PCG and restored. */
#define GATO_QP_POLISH_ACCEPTED 0
#define GATO_QP_POLISH_REJECTED 1
#define GATO_QP_POLISH_NONFINITE 2
#define GATO_QP_POLISH_BAD_ACTIVE 3
int gato_box_qp_polish(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                       const void *d_lo, const void *d_hi, const signed char *d_act, const gato_box_qp_params *p, void *d_x, void *d_z,
                       void *d_y, void *d_lambda, int *d_status, double *d_res /* [B][2] */, int *d_polish, void *stream);
/* Bound gradients of a polished solution: with the adjoint [a; beta] of the reduced system (gato_solve_rhs after the polish
 * with g = x_bar, c = lambda_bar; a is 0 on the active set), b_bar_i = x_bar_i - (H a + C^T beta)_i on the active set goes to
 * d_hi_bar where act = +1 and to d_lo_bar where act = -1 (lo == hi: to lo; a shift of both bounds together gets b_bar);
 * 0 in both elsewhere.  g_bar = a, c_bar = beta and the block gradients are gato_kkt_grad_blocks(x, lambda, a, beta).
 * d_xbar, d_a, d_lo_bar, d_hi_bar [B][N], d_beta [B][S*K].  Asynchronous.  GATO_EINVAL for a NULL pointer (d_C_blocks may be
 * NULL only for K = 1) and on a cluster rank. */
int gato_box_qp_bound_grad(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act, const void *d_xbar,
                           const void *d_a, const void *d_beta, void *d_lo_bar, void *d_hi_bar, void *stream);
/* Primal-dual active-set iteration: the polish iterated.  From the start act in d_act, per system: the reduced
 * solve of gato_box_qp_polish on act; if the polished point passes the polish's acceptance test it is written to d_x, d_z,
 * d_y, d_lambda, d_res, d_status = GATO_QP_CONVERGED and d_iters = the number of reduced solves; a non-finite maximum ends
 * the system in GATO_QP_NONFINITE.  Otherwise the next act is 0 on the states of x_0, -1 where lo == hi, for a free variable +1
 * where x > hi, -1 where x < lo, for an active one kept while its multiplier has the bound's sign (y > 0 upper, y < 0 lower)
 * and 0 otherwise - exact comparisons.  GATO_QP_MAX_ITERS after max_pdas_iters solves, or at once when the next act equals
 * the current one (d_iters = the solves done).  A system that does not end CONVERGED has none of d_x, d_z, d_y, d_lambda, d_res
 * written.  A system that has ended is not written again and no system's result depends on its batch neighbours.  d_act
 * [B][N] int8: in the start (all 0: a cold start), out the act of every system's last reduced solve.  No penalty parameter:
 * of p only rho, exit_tol, max_iters (the PCG), eps_abs and eps_rel are read.  Exact and finite for bounds on the controls
 * alone (the reduced matrix is never singular); with many active state bounds it may cycle or meet a singular reduced
 * system, which ends in MAX_ITERS or NONFINITE, never in a wrong answer.  Blocking: the live count is read once per solve.
 * GATO_EINVAL, nothing enqueued, for a captured stream, a cluster rank, a NULL pointer or a parameter out of range;
 * GATO_EINVAL after the first launches for a NaN bound or lo > hi (d_status = GATO_QP_BAD_BOUNDS) and for a start act that is
 * not -1, 0 or 1, names an infinite bound or a state of x_0 (d_status = GATO_QP_BAD_ACTIVE); -1 on the other systems, no
 * output written, the solver has no assembly.  Side effect: one whole-solve assembly per solve (assembly_gen advances by the
 * number of solves); the last one is the polish assembly of the returned d_act, so gato_solve_rhs is the adjoint of the
 * backward pass exactly as after gato_box_qp_polish. */
#define GATO_QP_BAD_ACTIVE 4
int gato_box_qp_pdas(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                     const void *d_lo, const void *d_hi, signed char *d_act, const gato_box_qp_params *p, int max_pdas_iters,
                     void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status, double *d_res /* [B][2] */,
                     void *stream);
/* gato_box_qp_pdas with soft bounds: d_soft_w [B][N] holds a weight w_i >= 0 per variable (dz layout; NULL: all
 * 0).  w_i = 0 is the hard bound of gato_box_qp_pdas; w_i > 0 replaces the bound of variable i by the penalty
 * (w_i / 2) dist(x_i, [lo_i, hi_i])^2.  A soft variable that violates its bound is active (+1 above hi, -1 below lo, -1 where
 * lo == hi: a tracking term) but stays in the reduced system: the diagonal of Q_k or R_k gains w_i, g gains w_i b_i; d_x holds
 * the reduced solution there, d_z = d_x and d_y = w_i (x_i - b_i), the penalty force.  The acceptance test is that of
 * gato_box_qp_polish with the dual residual H x - g + C^T lambda + y (H without the weights); the sign test covers the
 * soft-active variables too.  The next act of a soft variable is decided from x alone (+1 where x > hi, -1 where x < lo, -1
 * where lo == hi, else 0), that of a hard one as in gato_box_qp_pdas.  The states of x_0 are never active and a variable with
 * both bounds infinite never is, whatever their weights.  Soft-active variables cannot make a reduced system singular; the
 * iteration is undamped, so for large weights (1e4 on the synthetic state boxes) it may cycle and end in MAX_ITERS as the hard
 * one does.  With d_soft_w NULL or all 0 every output is bit for bit that of gato_box_qp_pdas.  Refusals, blocking behaviour
 * (one host read per solve) and side effects are those of gato_box_qp_pdas; a weight that is NaN, negative or +inf marks its
 * system GATO_QP_BAD_BOUNDS and the call returns GATO_EINVAL with no output written.  The last assembly is that of the returned
 * d_act with the weights of its soft-active variables on the diagonal, so gato_solve_rhs is the adjoint of the backward pass. */
int gato_box_qp_pdas_soft(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                          const void *d_lo, const void *d_hi, const void *d_soft_w /* [B][N], NULL = all hard */,
                          signed char *d_act, const gato_box_qp_params *p, int max_pdas_iters, void *d_x, void *d_z, void *d_y,
                          void *d_lambda, int *d_iters, int *d_status, double *d_res /* [B][2] */, void *stream);
/* Bound and weight gradients of a converged gato_box_qp_pdas_soft point, one launch: with the adjoint [a; beta] of its last
 * assembly (gato_solve_rhs with g = x_bar masked to 0 on the hard-active set, c = lambda_bar), a hard-active variable gets
 * gato_box_qp_bound_grad's b_bar_i = x_bar_i - (H a + C^T beta)_i, a soft-active one b_bar_i = w_i a_i and d_w_bar_i =
 * a_i (b_i - x_i); b_bar goes to d_hi_bar where act = +1 and to d_lo_bar where act = -1 (lo == hi: to lo); every other entry
 * of the three outputs is 0.  g_bar = a, c_bar = beta and the block gradients are gato_kkt_grad_blocks(x, lambda, a, beta).
 * All vectors [B][N] but d_beta [B][S*K]; d_soft_w may be NULL (all hard).  Asynchronous.  GATO_EINVAL for another NULL pointer
 * (d_C_blocks may be NULL only for K = 1) and on a cluster rank. */
int gato_box_qp_soft_grad(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act,
                          const void *d_soft_w, const void *d_lo, const void *d_hi, const void *d_x, const void *d_xbar,
                          const void *d_a, const void *d_beta, void *d_lo_bar, void *d_hi_bar, void *d_w_bar, void *stream);
/* gato_box_qp_pdas_soft with capped penalty forces: d_soft_cap [B][N] holds a cap m_i >= 0 per variable (dz
 * layout; +inf: no cap; NULL: every cap +inf), read only where w_i > 0.  The penalty of a soft variable becomes the Huber
 * function h_i(d) = (w_i / 2) d^2 while w_i d <= m_i and m_i d - m_i^2 / (2 w_i) beyond, d = dist(x_i, [lo_i, hi_i]): the force
 * is clamp(w_i (x_i - clip(x_i)), -m_i, m_i).  act takes two more values: +2 (-2) names a variable saturated above hi (below
 * lo; where lo == hi the sign is that of the force).  A saturated variable is free in the reduced system - no diagonal term,
 * g_i loses s m_i, s the sign of its act - and has d_x the reduced solution, d_z = d_x and d_y = s m_i bit for bit.  The
 * acceptance test is that of gato_box_qp_pdas_soft, and also fails (within the dual tolerance) where |y_i| > m_i on a soft
 * variable with act +-1 or where s w_i (x_i - b_i) < m_i on a saturated one.  The next act of a soft variable with a finite cap,
 * from x alone with exact comparisons on the product f = w_i (x_i - hi_i): +2 where f > m_i, else +1 where x_i > hi_i; mirrored
 * below lo_i; lo == hi: +2 where f > m_i, -2 where -f > m_i, else -1; every other variable as in gato_box_qp_pdas_soft.  A start
 * act of +-2 is taken only on a variable with w_i > 0, a finite cap, a finite bound and off x_0 (else GATO_QP_BAD_ACTIVE); a
 * cap that is NaN or negative marks its system GATO_QP_BAD_BOUNDS.  A cap of 0 removes the bound.  With d_soft_cap NULL or all
 * +inf every output is bit for bit that of gato_box_qp_pdas_soft.  The iteration is still undamped: it may cycle and end in
 * MAX_ITERS.  Refusals, blocking behaviour and side effects are those of gato_box_qp_pdas_soft; the last assembly is that of
 * the returned d_act (saturated variables free), so gato_solve_rhs is the adjoint of the backward pass. */
int gato_box_qp_pdas_huber(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                           const void *d_lo, const void *d_hi, const void *d_soft_w /* [B][N], NULL = all hard */,
                           const void *d_soft_cap /* [B][N], NULL = no cap */, signed char *d_act, const gato_box_qp_params *p,
                           int max_pdas_iters, void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status,
                           double *d_res /* [B][2] */, void *stream);
/* gato_box_qp_soft_grad for a converged gato_box_qp_pdas_huber point, one launch: a saturated variable i (act = +-2, s its
 * sign, a finite cap) gets d_cap_bar_i = -s a_i and 0 in d_lo_bar, d_hi_bar and d_w_bar; every other variable gets what
 * gato_box_qp_soft_grad gives it and d_cap_bar_i = 0.  d_soft_cap may be NULL (no caps: d_cap_bar = 0).  Asynchronous. */
int gato_box_qp_huber_grad(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act,
                           const void *d_soft_w, const void *d_soft_cap, const void *d_lo, const void *d_hi, const void *d_x,
                           const void *d_xbar, const void *d_a, const void *d_beta, void *d_lo_bar, void *d_hi_bar, void *d_w_bar,
                           void *d_cap_bar, void *stream);
/* gato_box_qp_pdas_huber with an exact line search, for problems whose every bound is soft: every variable off
 * x_0 with a finite bound must have w_i > 0 (else d_status = GATO_QP_BAD_BOUNDS and GATO_EINVAL, found by the first host read);
 * d_soft_w is required, d_soft_cap may be NULL.  The problem is then the minimisation of the C1, strongly convex, piecewise-
 * quadratic phi(x) = 1/2 x^T H x - g^T x + sum h_i(dist(x_i, [lo_i, hi_i])) on C x = c, and the reduced solve on the act named by an
 * iterate xc is the Newton point x+ of phi at xc.  Per system the loop keeps xc: the first solve of a call (on the start act)
 * sets xc = x+; every later one moves xc to the exact minimiser of phi along d = x+ - xc, the root alpha in (0, 1) of the
 * non-decreasing piecewise-linear slope phi'(alpha) = d^T (H (xc + alpha d) - g + f(xc + alpha d)), f the capped force of 3.11,
 * or takes the full step xc = x+ (bit for bit) where phi'(1) <= 0 or phi'(0) >= 0.  The next act is that of the soft rule on
 * xc, not on x+.  The acceptance test, the outcomes, the stall rule, max_pdas_iters and the outputs are those of
 * gato_box_qp_pdas_huber: the accepted point is the x+ of its act.  In exact arithmetic the iteration ends after finitely many
 * solves.  d_alpha [B][max_pdas_iters] (may be NULL): the step length of every solve - 1 for the first and for a full step, 0
 * where no step was taken (the accepted or non-finite solve and the solves a system did not run).  Two more launches per solve;
 * a run repeats bit for bit.  Refusals, blocking behaviour and side effects are those of gato_box_qp_pdas_huber. */
int gato_box_qp_pdas_ls(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                        const void *d_lo, const void *d_hi, const void *d_soft_w /* [B][N] */,
                        const void *d_soft_cap /* [B][N], NULL = no cap */, signed char *d_act, const gato_box_qp_params *p,
                        int max_pdas_iters, void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status,
                        double *d_res /* [B][2] */, double *d_alpha /* [B][max_pdas_iters], may be NULL */, void *stream);
/* The line search of gato_box_qp_pdas_ls alone, two launches: from d_xc and the Newton point d_xplus [B][N], d_slope [B][2] =
 * phi'(0), phi'(1), d_alpha [B] = the step length and, where d_x is given, d_x [B][N] = xc + alpha (x+ - xc) (x+ bit for bit
 * where alpha = 1).  The weights on the states of x_0 are not read.  d_soft_cap may be NULL.  Asynchronous.  GATO_EINVAL for
 * another NULL pointer, a rho that is negative or not finite, and on a cluster rank. */
int gato_box_qp_line_search(gato_solver *s, const void *d_G_blocks, const void *d_g, const void *d_lo, const void *d_hi,
                            const void *d_soft_w, const void *d_soft_cap, double rho, const void *d_xc, const void *d_xplus,
                            double *d_alpha, double *d_slope, void *d_x, void *stream);

/* ---- hard bounds by an augmented-Lagrangian outer loop (new) --------------------------------------------
 * The box QP of gato_box_qp_solve with HARD bounds on states and controls, by the method of multipliers over
 * gato_box_qp_pdas_ls.  An ALM variable is one off x_0 with a finite bound and no weight (d_soft_w NULL or w_i = 0); a variable
 * with w_i > 0 stays the soft bound of gato_box_qp_pdas_huber (its weight, its cap, no multiplier).  Per system: a multiplier
 * mu [N] (0, or d_mu0), a weight w (alm_weight) and an act (d_act: in the start act, out the accepted one).  Outer step k = 1 ..
 * max_alm_iters: the inner run is gato_box_qp_pdas_ls's loop, launch for launch, on the bounds lo - mu / w, hi - mu / w with
 * weight w and no cap on the ALM variables (the caller's elsewhere), from the act the step before ended on, at most
 * max_pdas_iters solves.  An inner run that ends MAX_ITERS or NONFINITE ends the system with that status and nothing else
 * written.  On its converged point: v = max over the ALM variables of dist(x_i, [lo_i, hi_i]), mu <- y on them, and the point is
 * accepted iff v <= eps_abs + eps_rel |x|_inf: d_x; d_z = clip(x, lo, hi) on the ALM variables; d_y (mu on them, the soft force
 * elsewhere); d_lambda; d_res = {max(v, |C x - c|_inf), the inner run's dual residual}; d_status CONVERGED; d_iters = the reduced
 * solves of all steps; d_outer = k; d_weight = w.  Otherwise w <- alm_growth w where v > v_prev / 4 and w < alm_weight_max (never
 * after the first step).  After max_alm_iters steps: MAX_ITERS with d_res[0] = the last v, d_iters, d_outer and d_weight - an
 * infeasible box ends so.  d_soft_w, d_soft_cap, d_mu0, d_outer, d_weight may be NULL.  Systems the outer loop froze keep running
 * in the batch's inner runs; nothing of theirs is written again and every system has the bits of its solo run.  Blocking; one
 * host read per outer step beyond the inner loop's.  GATO_EINVAL as gato_box_qp_pdas_ls, and (d_status = GATO_QP_BAD_BOUNDS) for
 * an alm_weight that is not finite and positive, alm_growth <= 1 or alm_weight_max < alm_weight.  After a start act the first
 * inner run refuses d_status holds its marks; after an error at a later step (GATO_EHIP, GATO_ETIMEOUT) d_status is -1 on the
 * systems that were still running, their outputs are not written, and the frozen systems keep theirs. */
int gato_box_qp_alm(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                    const void *d_lo, const void *d_hi, const void *d_soft_w, const void *d_soft_cap, signed char *d_act,
                    const gato_box_qp_params *p, int max_pdas_iters, double alm_weight, double alm_growth, double alm_weight_max,
                    int max_alm_iters, const void *d_mu0, void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters,
                    int *d_status, double *d_res /* [B][2] */, int *d_outer, double *d_weight, void *stream);
/* The update and the decision of one outer step alone, two launches, on given converged inner points d_x, d_y [B][N], d_lambda
 * [B][S*K] with the multipliers d_mu [B][N] (in, out), the weights d_w [B] and the violations of the step before d_v_prev [B]
 * (doubles; +inf: the first step): d_v, d_xinf [B] = v and |x|_inf, d_dec [B] = the decision (0 accept, 1 the weight grows, 2 it
 * stays, 3 the last step; 4, an inner run that did not converge, does not occur here), and for a system that goes on d_lo2, d_hi2, d_w2 [B][N] = the next inner bounds and weights on its ALM
 * variables (other entries are not written); d_z [B][N] is written for an accepted system.  d_soft_w [B][N] (may be NULL) names
 * the soft variables, which are no ALM variables; caps are not read.  Asynchronous. */
int gato_box_qp_alm_update(gato_solver *s, const void *d_x, const void *d_y, const void *d_lambda, void *d_mu, const double *d_w,
                           const double *d_v_prev, const void *d_lo, const void *d_hi, const void *d_soft_w,
                           double eps_abs, double eps_rel, double alm_growth, double alm_weight_max,
                           int last, double *d_v, double *d_xinf, int *d_dec, void *d_lo2, void *d_hi2, void *d_w2, void *d_z,
                           void *stream);

/* ---- forward-mode sensitivities (new): the right-hand side of the tangent system, one launch --------
 * For R directions per system, from the returned point (d_x [B][N], d_lambda [B][S*K]) and the input tangents (a dot):
 *     t_g = g. - G. x - C.^T lambda,   t_c = c. - C. x            (C's identity blocks carry no tangent; rho drops out)
 *     soft-active i (act = +-1, w_i > 0):  t_g,i += w._i (b_i - x_i) + w_i b._i;   saturated i (act = +-2):  t_g,i -= sign(act_i) m._i
 *     t_g -= G b._A,  t_c -= C b._A   (b._A = b. on the hard-active set A - act != 0 and w_i = 0 or no weights - and 0 elsewhere;
 *                                      C's identity blocks included; b. = hi. where act > 0, lo. where act < 0)
 * gato_solve_rhs(R, d_tg, d_tc) on the point's assembly (the whole solve's, or the last one of a box-QP call) then gives the
 * tangent [x.'; lambda.]: x. = x.' off A and b. on A.  Rows of d_tg on A hold what the sums give; the reduced system ignores them.
 * Tangents: d_G_dot [B][R][G_dense], d_C_dot [B][R][C_dense] (the layouts of d_G_blocks / d_C_blocks; Q. and R. are used as
 * given: symmetric perturbations), d_g_dot, d_lo_dot, d_hi_dot, d_w_dot, d_m_dot [B][R][N], d_c_dot [B][R][S*K]; each may be NULL
 * (zero), and a NULL one is not read.  Shared by the R directions: d_x, d_lambda, d_G_blocks (WITHOUT rho), d_C_blocks, d_act
 * [B][N] int8 (NULL: nothing active, the tangent of a plain solve - then the blocks, bounds and weights are not read), d_soft_w,
 * d_soft_cap (NULL as in gato_box_qp_huber_grad), d_lo, d_hi (read on the soft-active set only).  Outputs d_tg [B][R][N],
 * d_tc [B][R][S*K], the layouts gato_solve_rhs takes.  No atomics and a fixed order of the sums: a run repeats bit for bit.
 * Touches no solver state and no assembly.  Asynchronous.  GATO_EINVAL for R < 1, a NULL d_x, d_lambda, d_tg or d_tc, an act
 * without its blocks (d_C_blocks may be NULL only for K = 1), weights without d_lo and d_hi, and on a cluster rank. */
int gato_kkt_tangent_rhs(gato_solver *s, int R, const void *d_G_dot, const void *d_C_dot, const void *d_g_dot, const void *d_c_dot,
                         const void *d_lo_dot, const void *d_hi_dot, const void *d_w_dot, const void *d_m_dot, const void *d_x,
                         const void *d_lambda, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act,
                         const void *d_soft_w, const void *d_soft_cap, const void *d_lo, const void *d_hi, void *d_tg, void *d_tc,
                         void *stream);

/* ---- direct block input (new): the caller already holds the per-knot blocks in the
 * reference's dense layouts - d_G_blocks as G_dense WITHOUT rho, d_C_blocks as C_dense - so the CSR scatter is
 * skipped; rho is added to the diagonals of Q_k, R_k on the way into the solver's workspace.  Otherwise identical
 * to gato_linsys_device (batched solvers take B systems back to back). */
int gato_linsys_device_blocks(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g,
                              const void *d_c, double exit_tol, int max_iters, double rho, void *d_lambda, void *d_dz,
                              void *stream);

/* ---- a state-control cross term in the stage cost (new) ------------------------------------------------
 * G_k = [[Q_k, M_k], [M_k^T, R_k]] for k < K-1 (the last knot has no M; K = 1 has none at all): the term x_k^T M_k u_k that the
 * block-diagonal inputs cannot express (the CSR scatter drops such entries).  d_M_blocks is [B][(K-1)*S*C], per knot M_k S x C
 * column-major, as B_k lies in C_dense.  Every G_k + rho I must be positive definite (documented, not checked - as an
 * indefinite Q_k is not checked today).
 * The cross term is removed by the per-knot change of variables u_k = v_k - W_k x_k, W_k = (R_k + rho I)^-1 M_k^T (C x S):
 *     Q''_k = Q_k - M_k W_k,   A^'_k = A^_k - B^_k W_k,   g'_x,k = g_x,k - W_k^T g_u,k;   R_k, B^_k, g_u, c, lambda unchanged
 * (A^, B^: the raw values of C_dense).  One launch writes the transformed blocks and W into a work area of the solver's own
 * (the caller's arrays are never written), the unchanged path of gato_linsys_device_blocks solves the transformed problem, one
 * launch maps dz back in place.  lambda is that of the original problem.  Asynchronous as gato_linsys_device_blocks is, but
 * for the first call of a solver, which allocates the work area (so: once before a graph capture).  The call records that
 * the solver's current assembly is a cross one.  K = 1: d_M_blocks may be NULL and the call is the plain solve.
 * After a cross solve the solver's assembly is the TRANSFORMED system: plain gato_solve_rhs solves that one, in the variables
 * (x, v) for a right-hand side in g' form; gato_solver_recover does not apply (it reports the time-out). */
int gato_linsys_device_blocks_cross(gato_solver *s, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks,
                                    const void *d_g, const void *d_c, double exit_tol, int max_iters, double rho,
                                    void *d_lambda, void *d_dz, void *stream);
/* gato_solve_rhs for the original problem of the latest cross solve: R right-hand sides per system, d_g [B][R][N] -> g' (one
 * launch, from the stored W), the re-solve, dz mapped back in place (one launch).  Arguments as gato_solve_rhs.  GATO_EINVAL
 * when the solver's current assembly is not the cross one recorded (another whole solve, a box-QP call or a stage entry
 * replaced it).  A larger R than any before allocates (not while capturing). */
int gato_solve_rhs_cross(gato_solver *s, int R, const void *d_g, const void *d_c, double exit_tol, int max_iters,
                         void *d_lambda, void *d_dz, int *d_iters, void *stream);
/* The gradient of a cross solve with respect to M from dz and the adjoint's a (gato_solve_rhs_cross with g = dz_bar, c =
 * lambda_bar), both in the original variables: M_bar_k = -(a_x,k dz_u,k^T + dz_x,k a_u,k^T), [B][(K-1)*S*C] in M's layout - the
 * gradient for M_k and M_k^T perturbed together.  Q_bar, R_bar, A_bar, B_bar are gato_kkt_grad_blocks on the same vectors;
 * g_bar = a, c_bar = beta.  Reads no assembly.  K = 1: nothing to write. */
int gato_kkt_grad_cross(gato_solver *s, const void *d_dz, const void *d_adz, void *d_Mbar, void *stream);
/* The three stages alone (tests, and callers that run the solve between them themselves): the transformed blocks, W and g'
 * into the work area (buffers 13 .. 16; a cross assembly recorded before is forgotten); g' [B][R][N] of R right-hand sides from
 * the stored W; u <- v - W x in place on d_dz [B][R][N]. */
int gato_cross_prepare(gato_solver *s, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks, const void *d_g,
                       double rho, void *stream);
int gato_cross_rhs(gato_solver *s, int R, const void *d_g, void *d_gp, void *stream);
int gato_cross_finish(gato_solver *s, int R, void *d_dz, void *stream);

/* ---- CSR entry to the cross solve (new) ---------------------------------------------------------------
 * gato_linsys_device / _batched for a G whose state rows hold control columns: the term x_k^T M_k u_k of a non-separable stage
 * cost, which every other CSR entry drops (as the reference does).  Opt-in: no other entry changes.
 * SCATTER RULE.  Addressing is that of gato_convert: knot = row / n, in-knot column = col % n (n = S + C), the last entry in
 * storage order wins a slot written twice, explicit zeros are values.  New: a G entry with in-knot row isr < S and in-knot
 * column isc >= S in a knot k < K-1 lands in M_k[isr + (isc - S)*S] (S x C column-major, the layout of d_M_blocks above).  The
 * mirror entries (isr >= S, isc < S) are NOT read: G is taken as symmetric, and where the two triangles disagree the state-row
 * one counts (upper-only storage is fine; lower-only storage loses M).  State rows of the last knot have no M: a control column
 * there is dropped.  rho is not added while gathering: the solve adds it to EVERY diagonal entry of G, where gato_linsys_device
 * adds it to the diagonal entries the CSR stores - the two differ exactly on a diagonal entry that is not stored.
 * gato_cross_prepare_csr is the stage alone: ONE launch gathers the CSR values into per-knot blocks and writes what
 * gato_cross_prepare writes (buffers 13 .. 16), bit for bit gato_cross_prepare on the blocks the rule gives.  d_G_out
 * [B][G_dense] (without rho), d_M_out [B][(K-1)*S*C], d_C_out [B][C_dense]: each NULL or written whole - the scattered blocks,
 * for callers that go on to gato_box_qp_solve_cross and the like.  The batch shares the index arrays; d_G_val [B][nnz_G],
 * d_C_val [B][nnz_C].  The indices are trusted, as gato_convert trusts them.
 * gato_linsys_device_cross: that launch, the whole solve of the transformed problem and the map back - three launches where the
 * one-workgroup solve applies, as gato_linsys_device_blocks_cross.  It records a cross assembly, so gato_solve_rhs_cross,
 * gato_kkt_tangent_rhs_cross and gato_kkt_grad_cross follow it unchanged; gato_solver_recover does not apply.  One entry for
 * B = 1 and batched solvers.  K = 1: the plain gato_linsys_device / _batched call.  GATO_EINVAL: a NULL array, nnz <= 0, a
 * cluster rank, a capturing stream on a solver's first call (the work area must grow).  The caller's arrays are never written. */
int gato_cross_prepare_csr(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, int nnz_G,
                           const int *d_C_row, const int *d_C_col, const void *d_C_val, int nnz_C, const void *d_g, double rho,
                           void *d_G_out, void *d_M_out, void *d_C_out, void *stream);
int gato_linsys_device_cross(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, int nnz_G,
                             const int *d_C_row, const int *d_C_col, const void *d_C_val, int nnz_C, const void *d_g,
                             const void *d_c, double exit_tol, int max_iters, double rho, void *d_lambda, void *d_dz,
                             void *stream);
/* gato_kkt_grad_csr through the scatter rule above: a kept cross entry carries M_bar_k (gato_kkt_grad_cross) at its slot, bit for
 * bit; a mirror entry, a cross entry of the last knot and an overwritten entry get 0.  Arguments and NULL rules of
 * gato_kkt_grad_csr. */
int gato_kkt_grad_csr_cross(gato_solver *s, const int *d_G_row, const int *d_G_col, int nnz_G, const int *d_C_row,
                            const int *d_C_col, int nnz_C, const void *d_dz, const void *d_lam, const void *d_adz,
                            const void *d_alam, void *d_Gbar_val, void *d_Cbar_val, void *stream);

/* ---- forward-mode sensitivities of a cross solve (new): the right-hand side of its tangent system ------
 * gato_kkt_tangent_rhs for a plain solve with the cross term, one launch.  For R directions per system, from the point of the
 * latest cross solve (d_x [B][N], d_lambda [B][S*K], original variables) and the input tangents (a dot; NULL: zero, not read):
 *     t_g = g. - G. x - C.^T lambda,   (G. x)_x,k = Q._k x_k + M._k u_k,  (G. x)_u,k = M._k^T x_k + R._k u_k   (the last knot has no M)
 *     t_c = c. - C. x
 * d_M_dot [B][R][(K-1)*S*C] in M's layout is used as given: M_k and M_k^T perturbed together, the convention of
 * gato_kkt_grad_cross.  d_tg [B][R][N] receives t_g, d_gp [B][R][N] the transformed g'_x,k = t_g,x,k - W_k^T t_g,u,k, g'_u = t_g,u
 * from the W the cross solve stored (value for value gato_cross_rhs of d_tg); either may be NULL, not both.  d_tc [B][R][S*K].
 * [x.'; lambda.] = gato_solve_rhs(d_gp, d_tc) on the transformed assembly and gato_cross_finish on x.' give the tangent: W is part
 * of how the inverse is applied and carries no tangent of its own.  The other argument checks are gato_kkt_tangent_rhs's.
 * GATO_EINVAL when the solver's current assembly is not the cross one recorded, as gato_solve_rhs_cross refuses.  Writes no solver
 * state.  K = 1: d_M_dot may be NULL (it is not read) and the result is the plain right-hand side. */
int gato_kkt_tangent_rhs_cross(gato_solver *s, int R, const void *d_G_dot, const void *d_M_dot, const void *d_C_dot,
                               const void *d_g_dot, const void *d_c_dot, const void *d_x, const void *d_lambda, void *d_tg,
                               void *d_gp, void *d_tc, void *stream);

/* ---- box-constrained QP by ADMM with the cross term in the stage cost (new) ------------------------------
 * gato_box_qp_solve for H = G + rho I with G_k = [[Q_k, M_k], [M_k^T, R_k]]: arguments, checks, outputs, status codes and blocking
 * behaviour are gato_box_qp_solve's, plus d_M_blocks [B][(K-1)*S*C] in the layout of gato_linsys_device_blocks_cross.  The x-step
 * matrix [[H + sigma I + diag(rho_i), C^T], [C, 0]] is assembled once in the variables (x, v), u_k = v_k - W_k x_k with W_k =
 * (R_k + diag(sigma + rho_i) + rho I)^-1 M_k^T; the projection onto the box, x, z, y, lambda and the residuals (H with M) are in
 * the original variables, so the bounds on u are the caller's.  Every iteration is one gato_solve_rhs on the transformed assembly
 * plus one update launch, as without M.  Every G_k + rho I must be positive definite (not checked).  The caller's arrays are never
 * written.  K = 1: d_M_blocks may be NULL and the call is gato_box_qp_solve; K > 1 with a NULL d_M_blocks: GATO_EINVAL.
 * Side effect: afterwards the solver's assembly is the TRANSFORMED x-step matrix (assembly_gen advances by one), no cross assembly
 * is recorded - gato_solve_rhs_cross refuses - and gato_solver_recover does not apply. */
int gato_box_qp_solve_cross(gato_solver *s, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks, const void *d_g,
                            const void *d_c, const void *d_lo, const void *d_hi, const gato_box_qp_params *p, void *d_x, void *d_z,
                            void *d_y, void *d_lambda, int *d_iters, int *d_status, double *d_res /* [B][2] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GATO_HIP_H */
