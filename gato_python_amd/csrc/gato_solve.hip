// Whole solve, re-solve of its assembly for new right-hand sides, gradients of a solve.
#include "gato_solver.h"

// A1 + A2 + A3 for the whole-solve entries: ONE fused launch (assemble_kernel) where launch latency is what
// counts, the stage kernels one by one where throughput does (the fused workgroup recomputes its left neighbour's
// Schur block; option asm_mode: 0 = auto, 1 = stage kernels, 2 = fused).
// in.have_inv (polish): always the stage kernels, from the Schur launch on - G_dense and the inverses in Ginv are the caller's.
static int assemble(gato_solver *s, const AsmInput &in, const void *d_g, const void *d_c, double rho, hipStream_t st)
{
    int rc;
    const int mode = in.mode;
    s->d.k_lo = s->d.k_hi = 0;              // whole solves work on every knot: the knot-range option is for the stage entries
    // the fused launch always forms the stair blocks: the other preconditioner modes take the stage kernels
    const long long knots = (long long)s->d.K * s->d.B;
    // option asm_mode: 0 auto (2 while one round of workgroups covers the solve, else 1 - measured crossover),
    // 1 stage kernels, 2 one launch with a workgroup per knot (three-fold recomputation)
    const bool stair = s->precon_mode == GATO_PRECON_STAIR;
    const bool fused = !in.have_inv && stair && (s->asm_mode == 2 || (s->asm_mode == 0 && knots <= 2ll * s->num_cus));
    s->last_asm_fused = fused;
    s->img_fresh = 0;
    s->as.valid = 0;                        // until the whole solve around this assembly has been enqueued
    s->as.img = 0;
    if (!fused) {
        if (in.have_inv) rc = GATO_OK;
        else if (mode == 0) {            // CSR: the gather launch also inverts Q_k, R_k while they sit in LDS
            if (s->d.B > 1 && (s->d.nnzG <= 0 || s->d.nnzC <= 0)) return gato_convert(s, in.G_row, in.G_col, in.G_val, in.C_row, in.C_col, in.C_val, rho, s->G_dense, s->C_dense, st);
            rc = s->ops->convert(s->d, in.G_row, in.G_col, in.G_val, in.C_row, in.C_col, in.C_val, rho, s->G_dense, s->C_dense, s->Ginv, st);
        } else rc = s->ops->add_rho(s->d, in.G_val, rho, s->G_dense, st);
        if (rc) return rc;
        s->d.stair_follows = s->precon_mode == GATO_PRECON_STAIR;
        rc = s->ops->form_schur(s->d, s->G_dense, in.C_dense, d_g, d_c, s->Sbd, s->Pbd, s->gamma, s->Ginv, mode == 0 || in.have_inv, st);
        s->d.stair_follows = 0;
        if (rc) return rc;
        // preconditioner (gato_defines.h:9-10): the Schur stage leaves the block-Jacobi one (main blocks, zeros beside them)
        if (s->precon_mode == GATO_PRECON_BLOCK_JACOBI) return GATO_OK;                       // SS_PRECON = 0 (gato_schur.cuh:965-970)
        if (s->precon_mode == GATO_PRECON_POINT_JACOBI) return s->ops->point_jacobi(s->d, s->Sbd, s->Pbd, st);   // both 0 (:424-428)
        return gato_form_ss(s, s->Sbd, s->Pbd, st);
    }
    if (mode == 0 && s->d.B > 1 && (s->d.nnzG <= 0 || s->d.nnzC <= 0)) {
        set_error("a batched solver needs the per-system nnz (gato_linsys_device_batched, or options batch_nnz_G / batch_nnz_C)");
        return GATO_EINVAL;
    }
    AsmArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = mode;
    a.G_row = in.G_row; a.G_col = in.G_col; a.G_val = in.G_val; a.C_row = in.C_row; a.C_col = in.C_col; a.C_val = in.C_val;
    a.rho = rho; a.g = d_g; a.c = d_c;
    a.Gd = s->G_dense; a.Cd = const_cast<void *>(in.C_dense); a.Ginv = s->Ginv; a.Sbd = s->Sbd; a.Pbd = s->Pbd; a.gamma = s->gamma;
    a.stamps = s->stamp_asm ? (unsigned long long *)s->sw.scalars + 8 : nullptr;
    if (s->imgS && !s->no_image && s->d.B == 1) {        // the workgroup-per-knot launch also writes the PCG images
        a.imgS = s->imgS; a.imgP = s->imgP; a.img_ld = s->img_ld;
        s->img_fresh = 1;
        s->as.img = 1;
    }
    return s->ops->assemble(s->d, a, st);
}

// The whole solve on an assembly input: time-stamp, assemble, note what a recover (lc) and a dz riding in the PCG launch (fz) need,
// PCG, dz unless fused, note the assembly for the re-solve (as).  time_stages = false: the stage events are left alone.
int whole_solve(gato_solver *s, const PcgOpts &o, const AsmInput &in, const void *d_g, const void *d_c, double exit_tol,
                int max_iters, double rho, void *lam, void *dz, hipStream_t st)
{
    int rc;
    const bool ts = s->time_stages != 0 && !in.have_inv;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[0], st));
    if ((rc = assemble(s, in, d_g, d_c, rho, st))) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[1], st));
    s->lc = {1, s->Sbd, s->Pbd, s->gamma, in.C_dense, d_g, lam, dz, exit_tol, max_iters};
    s->fz = {s->Ginv, in.C_dense, d_g, dz};
    rc = pcg_systems(s, o, s->Sbd, s->Pbd, s->gamma, lam, exit_tol, max_iters, s->iters, st);
    s->fz = {nullptr, nullptr, nullptr, nullptr};
    s->img_fresh = 0;
    if (rc) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[2], st));
    if (!s->dz_fused && (rc = gato_compute_dz(s, s->Ginv, in.C_dense, d_g, lam, dz, st))) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[3], st));
    s->as = {1, in.C_dense, s->as.img, s->as.gen + 1};
    return GATO_OK;
}

extern "C" int gato_linsys_device(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val,
                                  const int *d_C_row, const int *d_C_col, const void *d_C_val, const void *d_g,
                                  const void *d_c, double exit_tol, int max_iters, double rho, void *d_lambda,
                                  void *d_dz, void *stream)
{
    const AsmInput in{0, d_G_row, d_G_col, d_G_val, d_C_row, d_C_col, d_C_val, s->C_dense, false};
    return whole_solve(s, pcg_opts(*s), in, d_g, d_c, exit_tol, max_iters, rho, d_lambda ? d_lambda : s->lambda, d_dz ? d_dz : s->dz,
                       (hipStream_t)stream);
}

extern "C" int gato_linsys_device_blocks(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g,
                                         const void *d_c, double exit_tol, int max_iters, double rho, void *d_lambda,
                                         void *d_dz, void *stream)
{
    const AsmInput in{2, nullptr, nullptr, d_G_blocks, nullptr, nullptr, nullptr, d_C_blocks, false};
    return whole_solve(s, pcg_opts(*s), in, d_g, d_c, exit_tol, max_iters, rho, d_lambda ? d_lambda : s->lambda, d_dz ? d_dz : s->dz,
                       (hipStream_t)stream);
}

extern "C" int gato_linsys_device_batched(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val,
                                          int nnz_G, const int *d_C_row, const int *d_C_col, const void *d_C_val,
                                          int nnz_C, const void *d_g, const void *d_c, double exit_tol, int max_iters,
                                          double rho, void *d_lambda, void *d_dz, int *d_iters, void *stream)
{
    s->d.nnzG = nnz_G; s->d.nnzC = nnz_C;
    int rc = gato_linsys_device(s, d_G_row, d_G_col, d_G_val, d_C_row, d_C_col, d_C_val, d_g, d_c, exit_tol, max_iters,
                                rho, d_lambda, d_dz, stream);
    if (rc) return rc;
    if (d_iters && d_iters != s->iters)
        GATO_HIP_CHECK(hipMemcpyAsync(d_iters, s->iters, sizeof(int) * s->d.B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GATO_OK;
}

// ---- re-solve: the latest whole-solve assembly for new right-hand sides ("factor once, solve many") ----------------------
// Reads Ginv, S (its left blocks are -phi), Pinv, the images and the C blocks of that assembly; writes none of them.

int *rhs_iters(gato_solver *s)
{
    return (int *)(s->rhs_ws + align_up((size_t)s->d.B * s->rhs_R * s->d.sk() * s->esz));
}

extern "C" int gato_solver_reserve_rhs(gato_solver *s, int R)
{
    if (!s) { set_error("solver_reserve_rhs: null solver"); return GATO_EINVAL; }
    if (R < 1 || (long long)R * s->d.B > 65535) {
        set_error("solver_reserve_rhs: R = %d must be >= 1 and batch x R <= 65535 (batch %d)", R, s->d.B);
        return GATO_EINVAL;
    }
    if (R <= s->rhs_R) return GATO_OK;
    const size_t n = (size_t)s->d.B * R;
    const size_t bytes = align_up(n * s->d.sk() * s->esz) + align_up(sizeof(int) * n);
    GATO_HIP_CHECK(hipSetDevice(s->device));
    char *p = nullptr;
    GATO_HIP_CHECK(hipMalloc((void **)&p, bytes));
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();          // re-solves still queued may read the old area
    if (e != hipSuccess) {
        (void)hipFree(p);
        set_error("solver_reserve_rhs: %s", hipGetErrorString(e));
        return GATO_EHIP;
    }
    if (s->rhs_ws) (void)hipFree(s->rhs_ws);
    if (s->lc.rhs > 0) s->lc.valid = 0;                        // its gamma lived in the old area
    s->rhs_ws = p; s->rhs_ws_bytes = bytes; s->rhs_R = R;
    return GATO_OK;
}

// The PCGs of a re-solve: n = B R right-hand sides, gamma / lambda / iters as [B][R] arrays, the R of system b on its S / Pinv.
// ONE launch with a workgroup per right-hand side where a system fits one workgroup (planned as a batch of n systems is),
// otherwise a launch per right-hand side on its system's matrices (as gato_pcg runs a batch system by system).
int pcg_rhs(gato_solver *s, const PcgOpts &o, int R, const void *gam, void *lam, double exit_tol, int max_iters, int *its, hipStream_t st)
{
    const int B = s->d.B, n = B * R;
    int rc;
    if (n == 1 || plan_one_wg_each(*s, o, n)) return pcg_one(s, o, s->Sbd, s->Pbd, gam, lam, exit_tol, max_iters, its, n, st, R);
    s->fz.dz = nullptr;                      // launch by launch: dz is a launch of its own
    const size_t e = s->esz, bd = s->d.bd() * e, sk = s->d.sk() * e;
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < R; ++r) {
            const size_t i = (size_t)b * R + r;
            if ((rc = pcg_one(s, o, (const char *)s->Sbd + b * bd, (const char *)s->Pbd + b * bd, (const char *)gam + i * sk,
                              (char *)lam + i * sk, exit_tol, max_iters, its + i, 1, st)))
                return rc;
        }
    return GATO_OK;
}

// dz of a re-solve: one dz_kernel launch over all B R right-hand sides, R consecutive ones on one system's Ginv / C blocks
int dz_rhs(gato_solver *s, int R, const void *g, const void *lam, void *dz, hipStream_t st)
{
    Dims d = s->d;
    d.B = s->d.B * R; d.rhs = R; d.k_lo = d.k_hi = 0;
    return s->ops->compute_dz(d, s->Ginv, s->as.Cd, g, lam, dz, st);
}

int solve_rhs(gato_solver *s, const PcgOpts &o, int R, const void *d_g, const void *d_c, double exit_tol, int max_iters,
              void *d_lambda, void *d_dz, int *d_iters, hipStream_t st)
{
    if (!s) { set_error("solve_rhs: null solver"); return GATO_EINVAL; }
    if (s->cl.on) { set_error("solve_rhs: the solver is a cluster rank; a sharded re-solve is not supported"); return GATO_EINVAL; }
    if (!s->as.valid) {
        set_error("solve_rhs: no assembly to re-solve: run a whole solve (gato_linsys_device, _blocks, _batched) first; a stage "
                  "entry that wrote into the solver's workspace or a cluster set-up since then invalidates it");
        return GATO_EINVAL;
    }
    if (R < 1 || (long long)R * s->d.B > 65535) {
        set_error("solve_rhs: R = %d must be >= 1 and batch x R <= 65535 (batch %d)", R, s->d.B);
        return GATO_EINVAL;
    }
    if (!d_g || !d_c || !d_lambda || !d_dz) { set_error("solve_rhs: d_g, d_c, d_lambda and d_dz are required"); return GATO_EINVAL; }
    const bool capturing = stream_is_capturing(st);
    if (R > s->rhs_R) {
        if (capturing) {
            set_error("solve_rhs: R = %d is beyond the %d reserved right-hand sides and the stream is being captured; call "
                      "gato_solver_reserve_rhs before the capture", R, s->rhs_R);
            return GATO_EINVAL;
        }
        const int rc = gato_solver_reserve_rhs(s, R);
        if (rc) return rc;
    }
    const int n = s->d.B * R;
    if (n == 1 || !plan_one_wg_each(*s, o, n)) {          // refuse before the gamma launch is enqueued, not after
        const PcgDecision d = pcg_decide(*s, o, 1, capturing);
        if (d.refusal == PCG_NO_FIT) {
            set_error("solve_rhs: K=%d does not fit the resident kernel on %d CUs", s->d.K, s->num_cus);
            return GATO_EINVAL;
        }
        if (d.refusal == PCG_NO_CAPTURE) {
            set_error("solve_rhs: a persistent launch of %d workgroups cannot be captured into a graph (its hand-off epochs "
                      "are launch arguments); capture the streaming kernels (option pcg_mode = 2) or a system that fits "
                      "one workgroup", d.g.groups);
            return GATO_EINVAL;
        }
    }
    int rc;
    s->d.k_lo = s->d.k_hi = 0;
    void *gam = s->rhs_ws;
    int *its = d_iters ? d_iters : rhs_iters(s);
    const bool ts = s->time_stages != 0;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[0], st));
    if ((rc = s->ops->rhs_gamma(s->d, R, s->Ginv, s->as.Cd, s->Sbd, d_g, d_c, gam, st))) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[1], st));
    s->lc = {1, s->Sbd, s->Pbd, gam, s->as.Cd, d_g, d_lambda, d_dz, exit_tol, max_iters, R, its};
    s->fz = {s->Ginv, s->as.Cd, d_g, d_dz};
    s->img_fresh = s->as.img;                // the assembly's transposed images still hold S and Pinv
    rc = pcg_rhs(s, o, R, gam, d_lambda, exit_tol, max_iters, its, st);
    s->fz = {nullptr, nullptr, nullptr, nullptr};
    s->img_fresh = 0;
    if (rc) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[2], st));
    if (!s->dz_fused && (rc = dz_rhs(s, R, d_g, d_lambda, d_dz, st))) return rc;
    if (ts) GATO_HIP_CHECK(hipEventRecord(s->ev_stage[3], st));
    return GATO_OK;
}

extern "C" int gato_solve_rhs(gato_solver *s, int R, const void *d_g, const void *d_c, double exit_tol, int max_iters,
                              void *d_lambda, void *d_dz, int *d_iters, void *stream)
{
    return solve_rhs(s, s ? pcg_opts(*s) : PcgOpts{}, R, d_g, d_c, exit_tol, max_iters, d_lambda, d_dz, d_iters, (hipStream_t)stream);
}

// ---- gradients of a solve (gato_grad.hip): vectors in, no assembly read ------------------------------------------------
extern "C" int gato_kkt_grad_blocks(gato_solver *s, const void *d_dz, const void *d_lam, const void *d_adz, const void *d_alam,
                                    void *d_Gbar, void *d_Cbar, void *stream)
{
    if (!solver_usable(s, "kkt_grad_blocks", "gradients")) return GATO_EINVAL;
    if (!d_dz || !d_lam || !d_adz || !d_alam) { set_error("kkt_grad_blocks: d_dz, d_lam, d_adz and d_alam are required"); return GATO_EINVAL; }
    if (!d_Gbar && !d_Cbar) { set_error("kkt_grad_blocks: both outputs are NULL"); return GATO_EINVAL; }
    Dims d = s->d;
    d.k_lo = d.k_hi = 0; d.rhs = 0;
    return s->ops->grad_blocks(d, d_dz, d_lam, d_adz, d_alam, d_Gbar, d_Cbar, (hipStream_t)stream);
}

extern "C" int gato_kkt_grad_csr(gato_solver *s, const int *d_G_row, const int *d_G_col, int nnz_G, const int *d_C_row,
                                 const int *d_C_col, int nnz_C, const void *d_dz, const void *d_lam, const void *d_adz,
                                 const void *d_alam, void *d_Gbar_val, void *d_Cbar_val, void *stream)
{
    if (!solver_usable(s, "kkt_grad_csr", "gradients")) return GATO_EINVAL;
    if (!d_dz || !d_lam || !d_adz || !d_alam) { set_error("kkt_grad_csr: d_dz, d_lam, d_adz and d_alam are required"); return GATO_EINVAL; }
    if (!d_Gbar_val && !d_Cbar_val) { set_error("kkt_grad_csr: both outputs are NULL"); return GATO_EINVAL; }
    if ((d_Gbar_val && (!d_G_row || !d_G_col || nnz_G < 0)) || (d_Cbar_val && (!d_C_row || !d_C_col || nnz_C < 0))) {
        set_error("kkt_grad_csr: an output needs its row pointers, column indices and nnz >= 0");
        return GATO_EINVAL;
    }
    Dims d = s->d;
    d.k_lo = d.k_hi = 0; d.rhs = 0;
    return s->ops->grad_csr(d, d_G_row, d_G_col, nnz_G, d_C_row, d_C_col, nnz_C, d_dz, d_lam, d_adz, d_alam, d_Gbar_val,
                            d_Cbar_val, (hipStream_t)stream);
}

