// Host side of the stage-cost cross term (gato_cross.hip): the transformed problem in a work area of the
// solver's own, the unchanged whole solve and re-solve on it, and the map back.
#include "gato_solver.h"

// The parts of cross_ws (CrossWs, gato_solver.h)
static CrossWs cross_layout(const gato_solver *s)
{
    const size_t e = s->esz, nb = (size_t)s->d.B;
    CrossWs o;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t at = off; off += align_up(bytes); return at; };
    o.G = take(s->d.g_dense() * e * nb);
    o.C = take(s->d.c_dense() * e * nb);
    o.W = take((size_t)(s->d.K - 1) * s->d.S * s->d.C * e * nb);
    o.g = take(s->d.N() * e * nb);
    o.bytes = off ? off : 256;
    return o;
}

// Grow-only: the first call of a solver (and the first re-solve of a larger R) allocates, no later one does.  Never while the
// stream is being captured.
static int grow(const char *who, char **ws, size_t *have, size_t bytes, hipStream_t st)
{
    if (bytes <= *have) return GATO_OK;
    if (stream_is_capturing(st)) {
        set_error("%s: the cross-term work area must grow and the stream is being captured; run the call once before the capture", who);
        return GATO_EINVAL;
    }
    char *w = nullptr;
    GATO_HIP_CHECK(hipStreamSynchronize(st));           // a call still queued may use the old area
    GATO_HIP_CHECK(hipDeviceSynchronize());
    GATO_HIP_CHECK(hipMalloc((void **)&w, bytes));
    if (*ws) (void)hipFree(*ws);
    *ws = w; *have = bytes;
    return GATO_OK;
}

static Dims kernel_dims(const gato_solver *s)
{
    Dims d = s->d;
    d.k_lo = d.k_hi = 0; d.rhs = 0;
    return d;
}

// "R >= 1 and batch x R <= 65535": the right-hand sides of a batch are the y of one grid
static int check_R(const gato_solver *s, const char *who, int R)
{
    if (R >= 1 && (long long)R * s->d.B <= 65535) return GATO_OK;
    set_error("%s: R = %d must be >= 1 and batch x R <= 65535 (batch %d)", who, R, s->d.B);
    return GATO_EINVAL;
}

static int check_cross_assembly(const gato_solver *s, const char *who)
{
    if (s->cross.valid && s->as.valid && s->cross.gen == s->as.gen) return GATO_OK;
    set_error("%s: the solver's current assembly is not that of a cross solve: run gato_linsys_device_blocks_cross first; any "
              "other whole solve, box-QP call or stage entry since then replaces it", who);
    return GATO_EINVAL;
}

// The work area, laid out (*o) and grown if need be, about to be written: a recorded cross assembly is forgotten, and the
// assembly that read the area's C' (if any) is no longer the solver's.
static int cross_ws_begin(gato_solver *s, const char *who, CrossWs *o, hipStream_t st)
{
    *o = cross_layout(s);
    int rc;
    if ((rc = grow(who, &s->cross_ws, &s->cross_ws_bytes, o->bytes, st))) return rc;
    s->cross.valid = 0;
    if (s->as.Cd == s->cross_ws + o->C) s->as.valid = 0;
    return GATO_OK;
}

// The whole solve of the problem prepared in the work area and the map back: the tail of both whole-solve entries (K > 1)
static int cross_solve_ws(gato_solver *s, const CrossWs &o, const void *d_c, double exit_tol, int max_iters, double rho, void *d_lambda,
                          void *d_dz, hipStream_t st)
{
    char *w = s->cross_ws;
    void *dz = d_dz ? d_dz : s->dz;
    const AsmInput in{2, nullptr, nullptr, w + o.G, nullptr, nullptr, nullptr, w + o.C, false};
    int rc;
    if ((rc = whole_solve(s, pcg_opts(*s), in, w + o.g, d_c, exit_tol, max_iters, rho, d_lambda ? d_lambda : s->lambda, dz, st))) return rc;
    s->lc.valid = 0;                                                         // a recover would leave dz in the transformed variables
    if ((rc = cross_finish(kernel_dims(s), s->dtype, 1, w + o.W, dz, st))) return rc;
    s->cross = {1, s->as.gen};
    return GATO_OK;
}

// prepare into the work area
int cross_prepare_ws(gato_solver *s, const char *who, const void *d_G, const void *d_M, const void *d_C, const void *d_g, double rho,
                     CrossWs *o, hipStream_t st)
{
    int rc;
    if ((rc = cross_ws_begin(s, who, o, st))) return rc;
    char *w = s->cross_ws;
    CrossArgs a{d_G, d_M, d_C, d_g, w + o->G, w + o->C, w + o->W, w + o->g, rho};
    return cross_prepare(kernel_dims(s), s->dtype, a, st);
}

extern "C" int gato_cross_prepare(gato_solver *s, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks,
                                  const void *d_g, double rho, void *stream)
{
    if (!solver_usable(s, "cross_prepare", "cross-term solves")) return GATO_EINVAL;
    if (!d_G_blocks || !d_g || (s->d.K > 1 && (!d_M_blocks || !d_C_blocks))) {
        set_error("cross_prepare: d_G_blocks and d_g are required, d_M_blocks and d_C_blocks too unless K = 1");
        return GATO_EINVAL;
    }
    CrossWs o;
    return cross_prepare_ws(s, "cross_prepare", d_G_blocks, d_M_blocks, d_C_blocks, d_g, rho, &o, (hipStream_t)stream);
}

static int check_stage(gato_solver *s, const char *who, int R, const void *p0, const void *p1)
{
    if (!solver_usable(s, who, "cross-term solves")) return GATO_EINVAL;
    if (check_R(s, who, R)) return GATO_EINVAL;
    if (!p0 || !p1) { set_error("%s: every pointer is required", who); return GATO_EINVAL; }
    if (!s->cross_ws) { set_error("%s: no W yet: run gato_linsys_device_blocks_cross or gato_cross_prepare first", who); return GATO_EINVAL; }
    return GATO_OK;
}

extern "C" int gato_cross_rhs(gato_solver *s, int R, const void *d_g, void *d_gp, void *stream)
{
    int rc;
    if ((rc = check_stage(s, "cross_rhs", R, d_g, d_gp))) return rc;
    return cross_rhs(kernel_dims(s), s->dtype, R, s->cross_ws + cross_layout(s).W, d_g, d_gp, (hipStream_t)stream);
}

extern "C" int gato_cross_finish(gato_solver *s, int R, void *d_dz, void *stream)
{
    int rc;
    if ((rc = check_stage(s, "cross_finish", R, d_dz, d_dz))) return rc;
    return cross_finish(kernel_dims(s), s->dtype, R, s->cross_ws + cross_layout(s).W, d_dz, (hipStream_t)stream);
}

extern "C" int gato_linsys_device_blocks_cross(gato_solver *s, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks,
                                               const void *d_g, const void *d_c, double exit_tol, int max_iters, double rho,
                                               void *d_lambda, void *d_dz, void *stream)
{
    const char *who = "linsys_device_blocks_cross";
    if (!solver_usable(s, who, "cross-term solves")) return GATO_EINVAL;
    const int K = s->d.K;
    if (!d_G_blocks || !d_g || !d_c || (K > 1 && (!d_M_blocks || !d_C_blocks))) {
        set_error("%s: d_G_blocks, d_g and d_c are required, d_M_blocks and d_C_blocks too unless K = 1", who);
        return GATO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (K == 1) {                                                            // no M at all: the plain solve
        if ((rc = gato_linsys_device_blocks(s, d_G_blocks, d_C_blocks, d_g, d_c, exit_tol, max_iters, rho, d_lambda, d_dz, stream))) return rc;
        s->cross = {1, s->as.gen};
        return GATO_OK;
    }
    CrossWs o;
    if ((rc = cross_prepare_ws(s, who, d_G_blocks, d_M_blocks, d_C_blocks, d_g, rho, &o, st))) return rc;
    return cross_solve_ws(s, o, d_c, exit_tol, max_iters, rho, d_lambda, d_dz, st);
}

extern "C" int gato_solve_rhs_cross(gato_solver *s, int R, const void *d_g, const void *d_c, double exit_tol, int max_iters,
                                    void *d_lambda, void *d_dz, int *d_iters, void *stream)
{
    const char *who = "solve_rhs_cross";
    if (!solver_usable(s, who, "cross-term solves")) return GATO_EINVAL;
    if (check_cross_assembly(s, who) || check_R(s, who, R)) return GATO_EINVAL;
    if (!d_g || !d_c || !d_lambda || !d_dz) { set_error("%s: d_g, d_c, d_lambda and d_dz are required", who); return GATO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (s->d.K == 1) return solve_rhs(s, pcg_opts(*s), R, d_g, d_c, exit_tol, max_iters, d_lambda, d_dz, d_iters, st);
    int rc;
    if ((rc = grow(who, &s->cross_rhs_ws, &s->cross_rhs_ws_bytes, (size_t)s->d.B * R * s->d.N() * s->esz, st))) return rc;
    const void *W = s->cross_ws + cross_layout(s).W;
    const Dims d = kernel_dims(s);
    if ((rc = cross_rhs(d, s->dtype, R, W, d_g, s->cross_rhs_ws, st))) return rc;
    if ((rc = solve_rhs(s, pcg_opts(*s), R, s->cross_rhs_ws, d_c, exit_tol, max_iters, d_lambda, d_dz, d_iters, st))) return rc;
    s->lc.valid = 0;                                                         // as in the whole solve
    return cross_finish(d, s->dtype, R, W, d_dz, st);
}

// ---- right-hand side of the tangent system of a cross solve (gato_tangent_cross.hip) -------------------
extern "C" int gato_kkt_tangent_rhs_cross(gato_solver *s, int R, const void *d_G_dot, const void *d_M_dot, const void *d_C_dot,
                                          const void *d_g_dot, const void *d_c_dot, const void *d_x, const void *d_lambda,
                                          void *d_tg, void *d_gp, void *d_tc, void *stream)
{
    const char *who = "kkt_tangent_rhs_cross";
    if (!solver_usable(s, who, "tangents")) return GATO_EINVAL;
    if (R < 1) { set_error("%s: R = %d: at least one direction", who, R); return GATO_EINVAL; }
    if (!d_x || !d_lambda || !d_tc || (!d_tg && !d_gp)) {
        set_error("%s: d_x, d_lambda, d_tc and one of d_tg and d_gp are required", who);
        return GATO_EINVAL;
    }
    if (check_cross_assembly(s, who)) return GATO_EINVAL;
    const bool one = s->d.K == 1;                                             // no M and no W at all: the plain right-hand side
    const CrossTangentArgs a{d_G_dot, one ? nullptr : d_M_dot, d_C_dot, d_g_dot, d_c_dot, d_x, d_lambda,
                             one ? nullptr : s->cross_ws + cross_layout(s).W, d_tg, d_gp, d_tc};
    // Staging the tangent blocks in LDS pays once the launch is bound by memory traffic and costs a round trip through LDS on
    // every knot while it is bound by latency (DESIGN.md section 3.17 has both measurements): in place below CROSS_TANGENT_STAGE_WAVES
    // waves per compute unit.  Both forms give the same bits.
    const long long waves = (long long)s->d.B * (s->d.K < 8192 ? s->d.K : 8192);
    const bool in_place = s->cross_tangent_form ? s->cross_tangent_form == 2 : waves < (long long)CROSS_TANGENT_STAGE_WAVES * s->num_cus;
    return cross_tangent_rhs(kernel_dims(s), s->dtype, R, a, in_place, (hipStream_t)stream);
}

extern "C" int gato_kkt_grad_cross(gato_solver *s, const void *d_dz, const void *d_adz, void *d_Mbar, void *stream)
{
    if (!solver_usable(s, "kkt_grad_cross", "gradients")) return GATO_EINVAL;
    if (s->d.K == 1) return GATO_OK;                                         // no M at all
    if (!d_dz || !d_adz || !d_Mbar) { set_error("kkt_grad_cross: d_dz, d_adz and d_Mbar are required"); return GATO_EINVAL; }
    return cross_grad(kernel_dims(s), s->dtype, d_dz, d_adz, d_Mbar, (hipStream_t)stream);
}

// ---- CSR entry (gato_cross_csr.hip) -----------------------------------------------------------------------
static int check_csr(gato_solver *s, const char *who, const int *G_row, const int *G_col, const void *G_val, int nnz_G, const int *C_row,
                     const int *C_col, const void *C_val, int nnz_C, const void *d_g)
{
    if (!solver_usable(s, who, "cross-term solves")) return GATO_EINVAL;
    if (!G_row || !G_col || !G_val || !C_row || !C_col || !C_val || !d_g) {
        set_error("%s: the six CSR arrays and d_g are required", who);
        return GATO_EINVAL;
    }
    if (nnz_G <= 0 || nnz_C <= 0) { set_error("%s: nnz_G = %d and nnz_C = %d must be positive (values per system)", who, nnz_G, nnz_C); return GATO_EINVAL; }
    return GATO_OK;
}

// the fused gather and prepare into the work area; as cross_prepare_ws
static int cross_prepare_csr_ws(gato_solver *s, const char *who, const int *G_row, const int *G_col, const void *G_val, int nnz_G,
                                const int *C_row, const int *C_col, const void *C_val, int nnz_C, const void *d_g, double rho,
                                void *G_out, void *M_out, void *C_out, CrossWs *o, hipStream_t st)
{
    int rc;
    if ((rc = cross_ws_begin(s, who, o, st))) return rc;
    char *w = s->cross_ws;
    Dims d = kernel_dims(s);
    d.nnzG = nnz_G; d.nnzC = nnz_C;
    const CrossCsrArgs a{G_row, G_col, C_row, C_col, G_val, C_val, d_g, w + o->G, w + o->C, w + o->W, w + o->g, G_out, M_out, C_out, rho};
    // Four waves gather a knot's entries faster than one while the launch is bound by latency; once the workgroups queue for the
    // compute units one wave per knot wastes fewer lanes in the transform - at the shapes up to 14/7, whose knot one wave gathers in
    // a dozen rounds; at 32/16 (61 rounds) four waves win at every size (DESIGN.md section 3.18 has the measurements).  Same bits.
    const long long knots = (long long)s->d.B * (s->d.K < 8192 ? s->d.K : 8192);
    const bool one_wave = s->d.S + s->d.C <= CROSS_CSR_WAVE_N && knots >= (long long)CROSS_CSR_WAVE_KNOTS * s->num_cus;
    const int threads = s->cross_csr_threads ? (s->cross_csr_threads == 64 ? 64 : 256) : one_wave ? 64 : 256;
    return cross_prepare_csr(d, s->dtype, a, threads, st);
}

extern "C" int gato_cross_prepare_csr(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, int nnz_G,
                                      const int *d_C_row, const int *d_C_col, const void *d_C_val, int nnz_C, const void *d_g,
                                      double rho, void *d_G_out, void *d_M_out, void *d_C_out, void *stream)
{
    const char *who = "cross_prepare_csr";
    int rc;
    if ((rc = check_csr(s, who, d_G_row, d_G_col, d_G_val, nnz_G, d_C_row, d_C_col, d_C_val, nnz_C, d_g))) return rc;
    CrossWs o;
    return cross_prepare_csr_ws(s, who, d_G_row, d_G_col, d_G_val, nnz_G, d_C_row, d_C_col, d_C_val, nnz_C, d_g, rho, d_G_out, d_M_out,
                                d_C_out, &o, (hipStream_t)stream);
}

extern "C" int gato_linsys_device_cross(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val, int nnz_G,
                                        const int *d_C_row, const int *d_C_col, const void *d_C_val, int nnz_C, const void *d_g,
                                        const void *d_c, double exit_tol, int max_iters, double rho, void *d_lambda, void *d_dz,
                                        void *stream)
{
    const char *who = "linsys_device_cross";
    int rc;
    if ((rc = check_csr(s, who, d_G_row, d_G_col, d_G_val, nnz_G, d_C_row, d_C_col, d_C_val, nnz_C, d_g))) return rc;
    if (!d_c) { set_error("%s: d_c is required", who); return GATO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (s->d.K == 1) {                                                       // no M at all: the plain CSR solve
        rc = s->d.B > 1 ? gato_linsys_device_batched(s, d_G_row, d_G_col, d_G_val, nnz_G, d_C_row, d_C_col, d_C_val, nnz_C, d_g, d_c,
                                                     exit_tol, max_iters, rho, d_lambda, d_dz, nullptr, stream)
                        : gato_linsys_device(s, d_G_row, d_G_col, d_G_val, d_C_row, d_C_col, d_C_val, d_g, d_c, exit_tol, max_iters, rho,
                                             d_lambda, d_dz, stream);
        if (rc) return rc;
        s->cross = {1, s->as.gen};
        return GATO_OK;
    }
    CrossWs o;
    if ((rc = cross_prepare_csr_ws(s, who, d_G_row, d_G_col, d_G_val, nnz_G, d_C_row, d_C_col, d_C_val, nnz_C, d_g, rho, nullptr, nullptr,
                                   nullptr, &o, st)))
        return rc;
    return cross_solve_ws(s, o, d_c, exit_tol, max_iters, rho, d_lambda, d_dz, st);
}

extern "C" int gato_kkt_grad_csr_cross(gato_solver *s, const int *d_G_row, const int *d_G_col, int nnz_G, const int *d_C_row,
                                       const int *d_C_col, int nnz_C, const void *d_dz, const void *d_lam, const void *d_adz,
                                       const void *d_alam, void *d_Gbar_val, void *d_Cbar_val, void *stream)
{
    const char *who = "kkt_grad_csr_cross";
    if (!solver_usable(s, who, "gradients")) return GATO_EINVAL;
    if (!d_dz || !d_lam || !d_adz || !d_alam) { set_error("%s: d_dz, d_lam, d_adz and d_alam are required", who); return GATO_EINVAL; }
    if (!d_Gbar_val && !d_Cbar_val) { set_error("%s: both outputs are NULL", who); return GATO_EINVAL; }
    if ((d_Gbar_val && (!d_G_row || !d_G_col || nnz_G < 0)) || (d_Cbar_val && (!d_C_row || !d_C_col || nnz_C < 0))) {
        set_error("%s: an output needs its row pointers, column indices and nnz >= 0", who);
        return GATO_EINVAL;
    }
    return grad_csr_cross(kernel_dims(s), s->dtype, d_G_row, d_G_col, nnz_G, d_C_row, d_C_col, nnz_C, d_dz, d_lam, d_adz, d_alam,
                          d_Gbar_val, d_Cbar_val, (hipStream_t)stream);
}
