// Box-constrained QP (ADMM over the re-solve), its polish, the active-set iteration with its line search, the augmented-
// Lagrangian outer loop, bound gradients and tangent right-hand sides: the host side of gato_qp.hip / gato_polish.hip /
// gato_pdas.hip / gato_pdas_ls.hip / gato_alm.hip / gato_tangent.hip.  The active-set entries each fill a BoxProblem and share
// pdas_loop; the bound-gradient entries share bound_grad.
#include <cmath>
#include <initializer_list>

#include "gato_solver.h"

// Grow-only work area (qp_ws, pol_ws): waits for everything that may still use the old one before it is replaced.
static int grow_ws(char **ws, size_t *have, size_t bytes, hipStream_t st)
{
    if (bytes <= *have) return GATO_OK;
    char *w = nullptr;
    GATO_HIP_CHECK(hipStreamSynchronize(st));           // a call still queued on another stream may use the old area
    GATO_HIP_CHECK(hipDeviceSynchronize());
    GATO_HIP_CHECK(hipMalloc((void **)&w, bytes));
    if (*ws) (void)hipFree(*ws);
    *ws = w; *have = bytes;
    return GATO_OK;
}

// The first check of the solve, polish and active-set entries: a usable solver, then p and every pointer of `required`
// (d_C_blocks only for K > 1).  ptr_note ends the entry's message inside its parentheses.
static int check_pointers(gato_solver *s, const char *who, const gato_box_qp_params *p, const void *d_C_blocks,
                          std::initializer_list<const void *> required, const char *ptr_note = "")
{
    if (!solver_usable(s, who, "QP solves")) return GATO_EINVAL;
    bool ok = p && (d_C_blocks || s->d.K <= 1);
    for (const void *q : required) ok = ok && q;
    if (!ok) set_error("%s: every pointer is required (d_C_blocks may be NULL only for K = 1%s)", who, ptr_note);
    return ok ? GATO_OK : GATO_EINVAL;
}

// Their last check: these entries read a count on the host (`reads` says which) and cannot run on a stream being captured.
static int check_not_capturing(const char *who, const char *reads, hipStream_t st)
{
    if (!stream_is_capturing(st)) return GATO_OK;
    set_error("%s: the stream is being captured; %s on the host and cannot be captured", who, reads);
    return GATO_EINVAL;
}

// The solver's dimensions as the box-QP kernels take them: every knot, no shared right-hand sides.
static Dims kernel_dims(const gato_solver *s)
{
    Dims d = s->d;
    d.k_lo = d.k_hi = 0; d.rhs = 0;
    return d;
}

// The start of a call: the work area zeroed from w + from to w + end (maxima, counts, counters), then the caller's status (the
// polish: its codes) -1 = running (undecided).
static int start_call(char *w, size_t from, size_t end, int *d_status, size_t B, hipStream_t st)
{
    GATO_HIP_CHECK(hipMemsetAsync(w + from, 0, end - from, st));
    GATO_HIP_CHECK(hipMemsetAsync(d_status, 0xff, B * sizeof(int), st));
    return GATO_OK;
}

// The systems still live (ctr[0]) to *live, once everything queued on st has run: what the loops wait for between rounds.
static int read_live(const char *who, const int *ctr, int *live, hipStream_t st)
{
    hipError_t he = hipMemcpyAsync(live, ctr, sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he == hipSuccess) return GATO_OK;
    set_error("%s: reading the live count failed: %s", who, hipGetErrorString(he));
    return GATO_EHIP;
}

// What an entry that takes soft weights (and caps) adds to its pointer text: they may be NULL.
static const char *soft_note(bool takes_w, bool takes_cap)
{
    return takes_cap ? ", d_soft_w for no soft bound, d_soft_cap for no cap" : (takes_w ? ", d_soft_w for no soft bound" : "");
}

// The parameters a reduced solve reads (polish, active-set iteration): finite and in range.
static bool reduced_params_ok(const gato_box_qp_params &p)
{
    const bool fin = std::isfinite(p.rho) && std::isfinite(p.eps_abs) && std::isfinite(p.eps_rel) && std::isfinite(p.exit_tol);
    return fin && p.rho >= 0 && p.eps_abs >= 0 && p.eps_rel >= 0 && p.exit_tol >= 0 && p.max_iters >= 1;
}

// ---- box-constrained QP by ADMM over the re-solve (gato_qp.hip) ---------------------------------
extern "C" void gato_box_qp_default_params(gato_box_qp_params *p)
{
    if (!p) return;
    *p = gato_box_qp_params{};
    p->rho = 0; p->admm_rho = 0.1; p->sigma = 1e-6; p->alpha = 1.6; p->eps_abs = 1e-6; p->eps_rel = 1e-6;
    p->exit_tol = 1e-6; p->max_iters = 100; p->max_admm_iters = 4000; p->check_every = 25; p->warm = 0;
}

// One call: prepare, the whole solve on G' (the only assembly), then re-solve + update per iteration and a last launch
// that only tests.  Frozen systems are never written again, so the outputs do not depend on check_every.
// d_M_blocks (NULL: none): the cross blocks of gato_box_qp_solve_cross.  The cross prepare stage then
// transforms (G', M, C, g~0) into cross_ws, the whole solve and the re-solves run on that assembly in the variables (x, v), and
// qp_update_cross_kernel takes the place of qp_update_kernel: the iterates, the box and the residuals stay in (x, u).
static int admm_solve(gato_solver *s, const char *who, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks,
                      const void *d_g, const void *d_c, const void *d_lo, const void *d_hi, const gato_box_qp_params *p, void *d_x,
                      void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status, double *d_res, void *stream)
{
    if (check_pointers(s, who, p, d_C_blocks, {d_G_blocks, d_g, d_c, d_lo, d_hi, d_x, d_z, d_y, d_lambda, d_iters, d_status, d_res}))
        return GATO_EINVAL;
    const bool fin = std::isfinite(p->rho) && std::isfinite(p->admm_rho) && std::isfinite(p->sigma) && std::isfinite(p->alpha) &&
                     std::isfinite(p->eps_abs) && std::isfinite(p->eps_rel) && std::isfinite(p->exit_tol);
    if (!fin || p->rho < 0 || !(p->admm_rho > 0) || p->sigma < 0 || !(p->alpha > 0 && p->alpha < 2) || p->eps_abs < 0 ||
        p->eps_rel < 0 || p->exit_tol < 0 || p->max_iters < 1 || p->max_admm_iters < 1 || p->check_every < 1) {
        set_error("%s: parameters out of range (want finite values, rho >= 0, admm_rho > 0, sigma >= 0, 0 < alpha < 2, "
                  "eps_abs, eps_rel, exit_tol >= 0, max_iters, max_admm_iters, check_every >= 1)", who);
        return GATO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (check_not_capturing(who, "the loop reads the live count", st)) return GATO_EINVAL;
    const bool cross = d_M_blocks != nullptr;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    int rc = gato_solver_reserve_rhs(s, 1);
    if (rc) return rc;
    const Dims &d = s->d;
    const size_t e = s->esz, B = d.B, vN = align_up(B * d.N() * e), vK = align_up(B * d.sk() * e);
    const size_t o_Gp = 0, o_rho = o_Gp + align_up(B * d.g_dense() * e), o_x0 = o_rho + vN, o_x1 = o_x0 + vN, o_gt = o_x1 + vN;
    const size_t o_dz = o_gt + vN, o_lt = o_dz + vN, o_sl = o_lt + vK;
    const size_t o_tot = o_sl + align_up(B * 3 * GATO_QP_NSLOT * 8), o_ctr = o_tot + align_up(B * sizeof(int));
    // option qp_cross_unfused: a W of zeros (zeroed with the counters) and the right-hand side cross_rhs transforms into
    const bool unfused = cross && s->qp_cross_unfused;
    const size_t o_W0 = o_ctr + 256, o_gp = o_W0 + (unfused ? align_up(B * (size_t)(d.K - 1) * d.S * d.C * e) : 0);
    const size_t zero_end = unfused ? o_gp : o_ctr + 256, bytes = o_gp + (unfused ? vN : 0);
    if ((rc = grow_ws(&s->qp_ws, &s->qp_ws_bytes, bytes, st))) return rc;
    char *w = s->qp_ws;
    int *ctr = (int *)(w + o_ctr);
    s->qp_pcg_total = (int *)(w + o_tot);
    if ((rc = start_call(w, o_sl, zero_end, d_status, B, st))) return rc;              // slots, PCG totals, counters
    if (p->warm) GATO_HIP_CHECK(hipMemcpyAsync(w + o_lt, d_lambda, B * d.sk() * e, hipMemcpyDeviceToDevice, st));
    QpArgs a;
    memset(&a, 0, sizeof(a));
    a.G = d_G_blocks; a.Cd = d_C_blocks; a.g = d_g; a.c = d_c; a.lo = d_lo; a.hi = d_hi;
    a.Gp = w + o_Gp; a.rho = w + o_rho; a.x = d_x; a.z = d_z; a.y = d_y; a.lam = d_lambda; a.gt = w + o_gt;
    a.xt = w + o_dz; a.lt = w + o_lt; a.slots = (unsigned long long *)(w + o_sl);
    a.status = d_status; a.iters = d_iters; a.ctr = ctr; a.res = d_res; a.pcg_total = (int *)(w + o_tot);
    a.rho_reg = p->rho; a.admm_rho = p->admm_rho; a.sigma = p->sigma; a.alpha = p->alpha; a.eps_abs = p->eps_abs;
    a.eps_rel = p->eps_rel; a.warm = p->warm ? 1 : 0;
    a.xw = w + o_x0;
    if ((rc = s->ops->qp_prepare(d, a, st))) return rc;
    int h[2] = {0, 0};
    GATO_HIP_CHECK(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    if (h[1] > 0) {
        set_error("%s: %d bound(s) with lo > hi or NaN; d_status marks the systems (3 = BAD_BOUNDS)", who, h[1]);
        return GATO_EINVAL;
    }
    PcgOpts o = pcg_opts(*s);
    o.warm = p->warm ? 1 : 0;                          // the first x-step: cold, or from the caller's lambda
    AsmInput in{2, nullptr, nullptr, w + o_Gp, nullptr, nullptr, nullptr, d_C_blocks, false};
    const void *g0 = w + o_gt;
    QpCrossArgs ca{a, d_M_blocks, nullptr};
    if (cross) {                                       // (G', M, C, g~0) -> the transformed blocks, W and g~0' in cross_ws
        CrossWs cw;
        if ((rc = cross_prepare_ws(s, who, w + o_Gp, d_M_blocks, d_C_blocks, w + o_gt, p->rho, &cw, st))) return rc;
        char *xw = s->cross_ws;
        in.G_val = xw + cw.G; in.C_dense = xw + cw.C; g0 = xw + cw.g; ca.W = xw + cw.W;
    }
    // either update launch: the cross kernel reads and writes what qp_update_kernel does, and M and W
    const Dims kd = kernel_dims(s);
    auto update = [&](int it, int last) {
        if (!cross) return s->ops->qp_update(d, a, it, last, st);
        ca.q = a;
        return qp_update_cross(kd, s->dtype, ca, it, last, st);
    };
    rc = whole_solve(s, o, in, g0, d_c, p->exit_tol, p->max_iters, p->rho, w + o_lt, w + o_dz, st);
    if (cross) s->lc.valid = 0;                        // a recover would leave the x-step's solution in other variables than the loop reads
    if (rc) return rc;
    // unfused: the two maps of an iteration as cross_finish and cross_rhs launches, the update kernel's own with W = 0 the identity
    const void *W = ca.W;
    if (unfused) {
        ca.W = w + o_W0;
        if ((rc = cross_finish(kd, s->dtype, 1, W, w + o_dz, st))) return rc;
    }
    o.warm = 1;                                        // every later x-step: lambda warm from the previous one
    for (int it = 0;; ++it) {
        a.xr = w + (it % 2 ? o_x1 : o_x0);
        a.xw = w + (it % 2 ? o_x0 : o_x1);
        a.pcg_its = it == 0 ? s->iters : rhs_iters(s);
        if ((rc = update(it, 0))) return rc;
        if (it + 1 == p->max_admm_iters) {
            a.xr = a.xw;
            if ((rc = update(it + 1, 1))) return rc;        // the test of the last iterate only
            break;
        }
        if ((it + 1) % p->check_every == 0) {               // systems still live, after the test of iterate it
            if ((rc = read_live(who, ctr, h, st))) return rc;
            if (h[0] == 0) break;
        }
        if (unfused && (rc = cross_rhs(kd, s->dtype, 1, W, w + o_gt, w + o_gp, st))) return rc;
        rc = solve_rhs(s, o, 1, w + (unfused ? o_gp : o_gt), d_c, p->exit_tol, p->max_iters, w + o_lt, w + o_dz, rhs_iters(s), st);
        if (cross) s->lc.valid = 0;
        if (rc) return rc;
        if (unfused && (rc = cross_finish(kd, s->dtype, 1, W, w + o_dz, st))) return rc;
    }
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    return gato_pcg_status(s, nullptr);
}

extern "C" int gato_box_qp_solve(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g,
                                 const void *d_c, const void *d_lo, const void *d_hi, const gato_box_qp_params *p, void *d_x,
                                 void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status, double *d_res,
                                 void *stream)
{
    return admm_solve(s, "box_qp_solve", d_G_blocks, nullptr, d_C_blocks, d_g, d_c, d_lo, d_hi, p, d_x, d_z, d_y, d_lambda, d_iters,
                      d_status, d_res, stream);
}

// ---- the same with a state-control cross term in the stage cost (gato_qp_cross.hip) -------------------
extern "C" int gato_box_qp_solve_cross(gato_solver *s, const void *d_G_blocks, const void *d_M_blocks, const void *d_C_blocks,
                                       const void *d_g, const void *d_c, const void *d_lo, const void *d_hi,
                                       const gato_box_qp_params *p, void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters,
                                       int *d_status, double *d_res, void *stream)
{
    const char *who = "box_qp_solve_cross";
    if (!solver_usable(s, who, "QP solves")) return GATO_EINVAL;
    if (s->d.K > 1 && !d_M_blocks) {
        set_error("%s: d_M_blocks is required (it may be NULL only for K = 1, which has no cross term)", who);
        return GATO_EINVAL;
    }
    return admm_solve(s, who, d_G_blocks, s->d.K > 1 ? d_M_blocks : nullptr, d_C_blocks, d_g, d_c, d_lo, d_hi, p, d_x, d_z, d_y,
                      d_lambda, d_iters, d_status, d_res, stream);
}

// ---- polish of a box QP and its bound gradients (gato_polish.hip) --------------------------------
extern "C" int gato_box_qp_active_set(gato_solver *s, const void *d_z, const void *d_y, const void *d_lo, const void *d_hi,
                                      signed char *d_act, void *stream)
{
    if (!solver_usable(s, "box_qp_active_set", "QP solves")) return GATO_EINVAL;
    if (!d_z || !d_y || !d_lo || !d_hi || !d_act) { set_error("box_qp_active_set: every pointer is required"); return GATO_EINVAL; }
    return s->ops->qp_active(kernel_dims(s), d_z, d_y, d_lo, d_hi, d_act, (hipStream_t)stream);
}

// The work area of the polish and of the active-set iteration (pol_ws), as offsets: the reduced system's right-hand side, the
// reduced solve and the polished point, then what only the iteration has (act', a second set of maxima, the round counts, polish
// flags of its own) around the maxima and the counters, and what only its line search has (the iterate, the knots' partial sums).
// Everything from sl on is zeroed at the start of a call.
struct PolishWs {
    size_t gp, cp, xt, lt, xp, zp, yp;      // [B][N] each, cp and lt [B][S K]
    size_t a2;                              // iteration: act' [B][N] int8
    size_t xc, part;                        // line search: LineSearchArgs::xc [B][N], part [B][K][2] doubles
    size_t sl;                              // the maxima, [B][GATO_POLISH_NSLOT]; iteration: [B][2][GATO_POLISH_NSLOT]
    size_t rn, pol;                         // iteration: PdasArgs::round [B][2][2], PolishArgs::polish [B]
    size_t ctr;                             // polish: the BAD_ACTIVE count; iteration: PdasArgs::ctr and the count after it
    size_t bytes;
};
static PolishWs polish_ws(const Dims &d, size_t e, bool pdas, bool ls = false)
{
    const size_t B = d.B, vN = align_up(B * d.N() * e), vK = align_up(B * d.sk() * e);
    PolishWs o;
    o.gp = 0; o.cp = o.gp + vN; o.xt = o.cp + vK; o.lt = o.xt + vN; o.xp = o.lt + vK; o.zp = o.xp + vN; o.yp = o.zp + vN;
    o.a2 = o.yp + vN;
    o.xc = o.a2 + (pdas ? align_up(B * d.N()) : 0);
    o.part = o.xc + (ls ? vN : 0);
    o.sl = o.part + (ls ? align_up(B * (size_t)d.K * 2 * sizeof(double)) : 0);
    o.rn = o.sl + align_up(B * (pdas ? 2 : 1) * GATO_POLISH_NSLOT * 8);
    o.pol = o.rn + (pdas ? align_up(B * 4 * sizeof(int)) : 0);
    o.ctr = o.pol + (pdas ? align_up(B * sizeof(int)) : 0);
    o.bytes = o.ctr + 256;
    return o;
}

// The problem of an active-set call, as its extern "C" entry (or gato_box_qp_alm, from its work area) fills it for pdas_loop.
struct BoxPoint {
    void *x, *z, *y, *lam;                  // [B][N], lam [B][S K]
    int *iters, *status;                    // [B]
    double *res;                            // [B][2]
};
struct BoxProblem {
    const char *who;                        // names the entry in errors
    bool takes_w, takes_cap;                // the entry has d_soft_w / d_soft_cap arguments: its texts speak of them
    const void *G, *C, *g, *c, *lo, *hi;    // the caller's blocks (G without rho, C raw) and vectors
    const void *w, *cap;                    // soft weights (NULL: all hard, section 3.10), caps of their forces (NULL: none, 3.11)
    signed char *act;                       // in: the start act; the iteration writes the final one
    BoxPoint pt;
};
// The exact line search of section 3.12, asked of pdas_loop: d_alpha [B][max_pdas_iters] (may be NULL) receives the step lengths.
struct LineSearch { double *d_alpha; };

// The part of PolishArgs both entries fill alike: the solver's buffers, the work area at w and the parameters.
static PolishArgs polish_args(const gato_solver *s, char *w, const PolishWs &o, const gato_box_qp_params *p)
{
    PolishArgs a;
    memset(&a, 0, sizeof(a));
    a.Gd = s->G_dense; a.Ginv = s->Ginv; a.gp = w + o.gp; a.cp = w + o.cp; a.xt = w + o.xt; a.lt = w + o.lt;
    a.xp = w + o.xp; a.zp = w + o.zp; a.yp = w + o.yp; a.slots = (unsigned long long *)(w + o.sl);
    a.rho = p->rho; a.eps_abs = p->eps_abs; a.eps_rel = p->eps_rel;
    return a;
}

// add rho, the masked inversion and shifted right-hand side (polish_prepare), then the stage kernels of the whole solve with
// the given inverses: Schur, the preconditioner; the PCG and dz follow as in gato_linsys_device_blocks.
extern "C" int gato_box_qp_polish(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                                  const void *d_lo, const void *d_hi, const signed char *d_act, const gato_box_qp_params *p,
                                  void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_status, double *d_res, int *d_polish,
                                  void *stream)
{
    if (check_pointers(s, "box_qp_polish", p, d_C_blocks,
                       {d_G_blocks, d_g, d_c, d_lo, d_hi, d_act, d_x, d_z, d_y, d_lambda, d_status, d_res, d_polish}))
        return GATO_EINVAL;
    if (!reduced_params_ok(*p)) {
        set_error("box_qp_polish: parameters out of range (want finite values, rho, eps_abs, eps_rel, exit_tol >= 0, max_iters >= 1)");
        return GATO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (check_not_capturing("box_qp_polish", "the polish reads the active-set check", st)) return GATO_EINVAL;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    const PolishWs o = polish_ws(s->d, s->esz, false);
    int rc;
    if ((rc = grow_ws(&s->pol_ws, &s->pol_ws_bytes, o.bytes, st))) return rc;
    char *w = s->pol_ws;
    int *nbad = (int *)(w + o.ctr);
    if ((rc = start_call(w, o.sl, o.bytes, d_polish, s->d.B, st))) return rc;         // slots, the BAD_ACTIVE count; -1 until decided
    PolishArgs a = polish_args(s, w, o, p);
    a.G = d_G_blocks; a.Cd = d_C_blocks; a.g = d_g; a.c = d_c; a.lo = d_lo; a.hi = d_hi; a.act = d_act; a.bad = nbad;
    a.x = d_x; a.z = d_z; a.y = d_y; a.lam = d_lambda; a.status = d_status; a.polish = d_polish; a.res = d_res;
    // the assembly: add rho and the masked inversion here, then the stage path of the whole solve with the inverses given
    s->d.k_lo = s->d.k_hi = 0;
    s->as.valid = 0;
    s->lc.valid = 0;                        // G_dense and Ginv are rewritten: nothing earlier is left to recover
    if ((rc = s->ops->add_rho(s->d, d_G_blocks, p->rho, s->G_dense, st))) return rc;
    if ((rc = s->ops->polish_prepare(s->d, a, st))) return rc;
    int h = 0;
    GATO_HIP_CHECK(hipMemcpyAsync(&h, nbad, sizeof(int), hipMemcpyDeviceToHost, st));
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    if (h > 0) {
        set_error("box_qp_polish: %d system(s) with an act that is not -1, 0 or 1, names an infinite bound or a state of x_0; "
                  "d_polish marks them (3 = BAD_ACTIVE)", h);
        return GATO_EINVAL;
    }
    PcgOpts po = pcg_opts(*s);
    po.warm = 0;                            // always a cold start
    const AsmInput in{2, nullptr, nullptr, d_G_blocks, nullptr, nullptr, nullptr, d_C_blocks, true};
    if ((rc = whole_solve(s, po, in, w + o.gp, w + o.cp, p->exit_tol, p->max_iters, p->rho, w + o.lt, w + o.xt, st))) return rc;
    if ((rc = s->ops->polish_finish(s->d, a, st))) return rc;
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    return gato_pcg_status(s, nullptr);
}

// ---- primal-dual active-set iteration: the polish iterated (gato_pdas.hip, DESIGN.md sections 3.9, 3.10) ----------------
// Per solve: add rho, the masked inversion and shifted right-hand side, the stage path of the whole solve (all as in the
// polish), then the step and the decision and one read of the live count.  b.w: the weights of soft bounds, read by the check,
// the prepare and the step; b.cap: the caps of their forces (not read without weights).  The texts speak of weights and caps
// where the entry takes them (b.takes_w, b.takes_cap), given or not.
// ls (may be NULL): the exact line search of section 3.12 - the scope check after the check launch, and between the step and the
// decision of every solve the two launches that move the iterate xc and take act' and its changed count from it.
static int pdas_loop(gato_solver *s, const BoxProblem &b, const gato_box_qp_params *p, int max_pdas_iters, hipStream_t st,
                     const LineSearch *ls)
{
    const char *who = b.who;
    const BoxPoint &pt = b.pt;
    if (check_pointers(s, who, p, b.C, {b.G, b.g, b.c, b.lo, b.hi, b.act, pt.x, pt.z, pt.y, pt.lam, pt.iters, pt.status, pt.res},
                       soft_note(b.takes_w, b.takes_cap)))
        return GATO_EINVAL;
    if (!reduced_params_ok(*p) || max_pdas_iters < 1) {
        set_error("%s: parameters out of range (want finite values, rho, eps_abs, eps_rel, exit_tol >= 0, max_iters, "
                  "max_pdas_iters >= 1)", who);
        return GATO_EINVAL;
    }
    if (check_not_capturing(who, "the loop reads the live count", st)) return GATO_EINVAL;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    const size_t B = s->d.B;
    const PolishWs o = polish_ws(s->d, s->esz, true, ls != nullptr);
    int rc;
    if ((rc = grow_ws(&s->pol_ws, &s->pol_ws_bytes, o.bytes, st))) return rc;
    char *w = s->pol_ws;
    int *ctr = (int *)(w + o.ctr);
    if ((rc = start_call(w, o.sl, o.bytes, pt.status, B, st))) return rc;             // both sets of maxima and counts, the counters
    double *d_alpha = ls ? ls->d_alpha : nullptr;
    if (d_alpha) GATO_HIP_CHECK(hipMemsetAsync(d_alpha, 0, B * max_pdas_iters * sizeof(double), st));   // 0: no step taken
    PdasArgs a;
    memset(&a, 0, sizeof(a));
    PolishArgs &q = a.p;
    q = polish_args(s, w, o, p);
    q.G = b.G; q.Cd = b.C; q.g = b.g; q.c = b.c; q.lo = b.lo; q.hi = b.hi; q.act = b.act; q.w = b.w;
    q.cap = b.w ? b.cap : nullptr;
    q.x = pt.x; q.z = pt.z; q.y = pt.y; q.lam = pt.lam; q.status = pt.status; q.polish = (int *)(w + o.pol); q.res = pt.res;
    q.bad = ctr + 3;
    a.act = b.act; a.act2 = (signed char *)(w + o.a2); a.round = (int *)(w + o.rn); a.ctr = ctr; a.iters = pt.iters;
    s->d.k_lo = s->d.k_hi = 0;
    s->as.valid = 0;
    s->lc.valid = 0;                        // G_dense and Ginv are rewritten: nothing earlier is left to recover
    if ((rc = s->ops->pdas_check(s->d, a, st))) return rc;
    LineSearchArgs la;
    memset(&la, 0, sizeof(la));
    if (ls) {
        la.G = b.G; la.g = b.g; la.lo = b.lo; la.hi = b.hi; la.w = b.w; la.cap = q.cap;
        la.xc = la.xout = w + o.xc; la.xp = q.xp; la.part = (double *)(w + o.part); la.alpha_stride = max_pdas_iters;
        la.status = la.status_out = pt.status; la.slots = q.slots; la.act = b.act; la.act2 = a.act2; la.round = a.round;
        la.bad = ctr + 4;
        la.rho = p->rho; la.eps_abs = p->eps_abs; la.eps_rel = p->eps_rel;
        if ((rc = s->ops->ls_scope(s->d, la, st))) return rc;
    }
    PcgOpts po = pcg_opts(*s);
    po.warm = 0;                            // every reduced solve is a cold start
    const AsmInput in{2, nullptr, nullptr, b.G, nullptr, nullptr, nullptr, b.C, true};
    for (int it = 1; it <= max_pdas_iters; ++it) {
        if ((rc = s->ops->add_rho(s->d, b.G, p->rho, s->G_dense, st))) return rc;
        if ((rc = s->ops->polish_prepare(s->d, q, st))) return rc;
        int h[5] = {0, 0, 0, 0, 0};         // ctr[3] is the polish's own count, ctr[4] the line search's scope check
        if (it == 1) {                      // the caller's bounds and start act; later acts are the device's own: valid
            GATO_HIP_CHECK(hipMemcpyAsync(h, ctr, (ls ? 5 : 3) * sizeof(int), hipMemcpyDeviceToHost, st));
            GATO_HIP_CHECK(hipStreamSynchronize(st));
            if (h[1] > 0 || h[2] > 0 || h[4] > 0) {
                set_error("%s:%s%s%s; d_status marks the systems", who,
                          h[4] > 0 ? " a finite bound off x_0 has no weight: the line search takes soft bounds only, every variable "
                                     "with a finite bound needs w_i > 0 (BAD_BOUNDS)" : "",
                          h[1] <= 0 ? ""
                          : b.takes_cap ? " a bound is NaN, lo > hi, a weight is NaN, negative or infinite or a cap is NaN or negative "
                                          "(BAD_BOUNDS)"
                          : b.takes_w ? " a bound is NaN, lo > hi or a weight is NaN, negative or infinite (BAD_BOUNDS)"
                                      : " a bound is NaN or lo > hi (BAD_BOUNDS)",
                          h[2] <= 0 ? ""
                          : b.takes_cap ? " a start act is not -2 .. 2, names an infinite bound or a state of x_0, or is +-2 without a "
                                          "weight and a finite cap (BAD_ACTIVE)"
                                        : " a start act is not -1, 0 or 1, names an infinite bound or a state of x_0 (BAD_ACTIVE)");
                return GATO_EINVAL;
            }
        }
        if ((rc = whole_solve(s, po, in, w + o.gp, w + o.cp, p->exit_tol, p->max_iters, p->rho, w + o.lt, w + o.xt, st))) return rc;
        if ((rc = s->ops->pdas_step(s->d, a, it, st))) return rc;
        if (ls) {
            la.it = it;
            la.alpha = d_alpha ? d_alpha + (it - 1) : nullptr;
            if ((rc = s->ops->line_search(s->d, la, st))) return rc;
        }
        if ((rc = s->ops->pdas_decide(s->d, a, it, it == max_pdas_iters, st))) return rc;
        if (it == max_pdas_iters) break;    // every system still live froze in that decision
        if ((rc = read_live(who, ctr, h, st))) return rc;
        if (h[0] == 0) break;
    }
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    return gato_pcg_status(s, nullptr);
}

extern "C" int gato_box_qp_pdas(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                                const void *d_lo, const void *d_hi, signed char *d_act, const gato_box_qp_params *p,
                                int max_pdas_iters, void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status,
                                double *d_res, void *stream)
{
    const BoxProblem b{"box_qp_pdas", false, false, d_G_blocks, d_C_blocks, d_g, d_c, d_lo, d_hi, nullptr, nullptr, d_act,
                       {d_x, d_z, d_y, d_lambda, d_iters, d_status, d_res}};
    return pdas_loop(s, b, p, max_pdas_iters, (hipStream_t)stream, nullptr);
}

// ---- soft bounds in the active-set iteration ------------------------------------------------------
extern "C" int gato_box_qp_pdas_soft(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g,
                                     const void *d_c, const void *d_lo, const void *d_hi, const void *d_soft_w, signed char *d_act,
                                     const gato_box_qp_params *p, int max_pdas_iters, void *d_x, void *d_z, void *d_y,
                                     void *d_lambda, int *d_iters, int *d_status, double *d_res, void *stream)
{
    const BoxProblem b{"box_qp_pdas_soft", true, false, d_G_blocks, d_C_blocks, d_g, d_c, d_lo, d_hi, d_soft_w, nullptr, d_act,
                       {d_x, d_z, d_y, d_lambda, d_iters, d_status, d_res}};
    return pdas_loop(s, b, p, max_pdas_iters, (hipStream_t)stream, nullptr);
}

// The three bound-gradient entries: the check of the pointers the entry takes (takes_w: lo, hi, x and w_bar too, takes_cap:
// cap_bar too; a.w and a.cap may be NULL), then the launch.
static int bound_grad(gato_solver *s, const char *who, bool takes_w, bool takes_cap, BoundGradArgs a, void *stream)
{
    if (!solver_usable(s, who, "gradients")) return GATO_EINVAL;
    bool ok = a.G && (a.Cd || s->d.K <= 1) && a.act && a.xbar && a.adz && a.beta && a.lo_bar && a.hi_bar;
    if (takes_w) ok = ok && a.lo && a.hi && a.x && a.w_bar;
    if (takes_cap) ok = ok && a.cap_bar;
    if (!ok) {
        set_error("%s: every pointer is required (d_C_blocks may be NULL only for K = 1%s)", who, soft_note(takes_w, takes_cap));
        return GATO_EINVAL;
    }
    if (!a.w) a.cap = nullptr;              // no cap is read without weights
    return s->ops->qp_bound_grad(kernel_dims(s), a, (hipStream_t)stream);
}

extern "C" int gato_box_qp_soft_grad(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act,
                                     const void *d_soft_w, const void *d_lo, const void *d_hi, const void *d_x, const void *d_xbar,
                                     const void *d_a, const void *d_beta, void *d_lo_bar, void *d_hi_bar, void *d_w_bar,
                                     void *stream)
{
    return bound_grad(s, "box_qp_soft_grad", true, false,
                      {d_G_blocks, d_C_blocks, d_act, d_soft_w, d_lo, d_hi, d_x, d_xbar, d_a, d_beta, d_lo_bar, d_hi_bar, d_w_bar}, stream);
}

extern "C" int gato_box_qp_bound_grad(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act,
                                      const void *d_xbar, const void *d_a, const void *d_beta, void *d_lo_bar, void *d_hi_bar,
                                      void *stream)
{
    return bound_grad(s, "box_qp_bound_grad", false, false,
                      {d_G_blocks, d_C_blocks, d_act, nullptr, nullptr, nullptr, nullptr,      // no weights: no lo, hi, x
                       d_xbar, d_a, d_beta, d_lo_bar, d_hi_bar, nullptr}, stream);
}

// ---- capped (Huber) soft bounds in the active-set iteration -------------------------------------------
extern "C" int gato_box_qp_pdas_huber(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g,
                                      const void *d_c, const void *d_lo, const void *d_hi, const void *d_soft_w,
                                      const void *d_soft_cap, signed char *d_act, const gato_box_qp_params *p, int max_pdas_iters,
                                      void *d_x, void *d_z, void *d_y, void *d_lambda, int *d_iters, int *d_status, double *d_res,
                                      void *stream)
{
    const BoxProblem b{"box_qp_pdas_huber", true, true, d_G_blocks, d_C_blocks, d_g, d_c, d_lo, d_hi, d_soft_w, d_soft_cap, d_act,
                       {d_x, d_z, d_y, d_lambda, d_iters, d_status, d_res}};
    return pdas_loop(s, b, p, max_pdas_iters, (hipStream_t)stream, nullptr);
}

extern "C" int gato_box_qp_huber_grad(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const signed char *d_act,
                                      const void *d_soft_w, const void *d_soft_cap, const void *d_lo, const void *d_hi,
                                      const void *d_x, const void *d_xbar, const void *d_a, const void *d_beta, void *d_lo_bar,
                                      void *d_hi_bar, void *d_w_bar, void *d_cap_bar, void *stream)
{
    return bound_grad(s, "box_qp_huber_grad", true, true,
                      {d_G_blocks, d_C_blocks, d_act, d_soft_w, d_lo, d_hi, d_x, d_xbar, d_a, d_beta, d_lo_bar, d_hi_bar, d_w_bar,
                       d_soft_cap, d_cap_bar}, stream);
}

// ---- right-hand side of the tangent system (gato_tangent.hip) -------------------------------------------
extern "C" int gato_kkt_tangent_rhs(gato_solver *s, int R, const void *d_G_dot, const void *d_C_dot, const void *d_g_dot,
                                    const void *d_c_dot, const void *d_lo_dot, const void *d_hi_dot, const void *d_w_dot,
                                    const void *d_m_dot, const void *d_x, const void *d_lambda, const void *d_G_blocks,
                                    const void *d_C_blocks, const signed char *d_act, const void *d_soft_w, const void *d_soft_cap,
                                    const void *d_lo, const void *d_hi, void *d_tg, void *d_tc, void *stream)
{
    if (!solver_usable(s, "kkt_tangent_rhs", "tangents")) return GATO_EINVAL;
    if (R < 1) { set_error("kkt_tangent_rhs: R = %d: at least one direction", R); return GATO_EINVAL; }
    if (!d_x || !d_lambda || !d_tg || !d_tc) { set_error("kkt_tangent_rhs: d_x, d_lambda, d_tg and d_tc are required"); return GATO_EINVAL; }
    if (d_act && (!d_G_blocks || (!d_C_blocks && s->d.K > 1))) {
        set_error("kkt_tangent_rhs: an act needs d_G_blocks and d_C_blocks (d_C_blocks may be NULL only for K = 1)");
        return GATO_EINVAL;
    }
    if (d_act && d_soft_w && (!d_lo || !d_hi)) { set_error("kkt_tangent_rhs: soft weights need d_lo and d_hi"); return GATO_EINVAL; }
    // without an act nothing is active; without weights no cap and no tangent of a weight or a cap is read
    const bool soft = d_act && d_soft_w;
    const TangentArgs a{d_G_dot, d_C_dot, d_g_dot, d_c_dot, d_act ? d_lo_dot : nullptr, d_act ? d_hi_dot : nullptr,
                        soft ? d_w_dot : nullptr, soft ? d_m_dot : nullptr, d_x, d_lambda, d_G_blocks, d_C_blocks, d_act,
                        soft ? d_soft_w : nullptr, soft ? d_soft_cap : nullptr, d_lo, d_hi, d_tg, d_tc};
    return s->ops->kkt_tangent_rhs(kernel_dims(s), R, a, (hipStream_t)stream);
}

// ---- exact line search of the soft active-set iteration (gato_pdas_ls.hip) -----------------------------
extern "C" int gato_box_qp_pdas_ls(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                                   const void *d_lo, const void *d_hi, const void *d_soft_w, const void *d_soft_cap,
                                   signed char *d_act, const gato_box_qp_params *p, int max_pdas_iters, void *d_x, void *d_z,
                                   void *d_y, void *d_lambda, int *d_iters, int *d_status, double *d_res, double *d_alpha,
                                   void *stream)
{
    if (!d_soft_w) {
        set_error("box_qp_pdas_ls: d_soft_w is required (the line search takes soft bounds only; d_soft_cap and d_alpha may be NULL)");
        return GATO_EINVAL;
    }
    const BoxProblem b{"box_qp_pdas_ls", true, true, d_G_blocks, d_C_blocks, d_g, d_c, d_lo, d_hi, d_soft_w, d_soft_cap, d_act,
                       {d_x, d_z, d_y, d_lambda, d_iters, d_status, d_res}};
    const LineSearch ls{d_alpha};
    return pdas_loop(s, b, p, max_pdas_iters, (hipStream_t)stream, &ls);
}

extern "C" int gato_box_qp_line_search(gato_solver *s, const void *d_G_blocks, const void *d_g, const void *d_lo, const void *d_hi,
                                       const void *d_soft_w, const void *d_soft_cap, double rho, const void *d_xc, const void *d_xplus,
                                       double *d_alpha, double *d_slope, void *d_x, void *stream)
{
    if (!solver_usable(s, "box_qp_line_search", "QP solves")) return GATO_EINVAL;
    if (!d_G_blocks || !d_g || !d_lo || !d_hi || !d_soft_w || !d_xc || !d_xplus || !d_alpha || !d_slope) {
        set_error("box_qp_line_search: every pointer is required (d_soft_cap may be NULL for no cap, d_x for no stepped point)");
        return GATO_EINVAL;
    }
    if (!std::isfinite(rho) || rho < 0) { set_error("box_qp_line_search: rho must be finite and >= 0"); return GATO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    const PolishWs o = polish_ws(s->d, s->esz, true, true);
    int rc;
    if ((rc = grow_ws(&s->pol_ws, &s->pol_ws_bytes, o.bytes, st))) return rc;
    LineSearchArgs la;
    memset(&la, 0, sizeof(la));
    la.G = d_G_blocks; la.g = d_g; la.lo = d_lo; la.hi = d_hi; la.w = d_soft_w; la.cap = d_soft_cap;
    la.xc = d_xc; la.xp = d_xplus; la.xout = d_x; la.part = (double *)(s->pol_ws + o.part);
    la.alpha = d_alpha; la.alpha_stride = 1; la.slope = d_slope; la.rho = rho; la.it = 2;
    return s->ops->line_search(kernel_dims(s), la, st);
}

// ---- hard bounds by an augmented-Lagrangian outer loop (gato_alm.hip) ----------------------------------
// The work area of the outer loop, behind the line-search iteration's in pol_ws (which the inner runs use and zero as they
// always do): the inner run's inputs and point, the multiplier, then what a call zeroes - the maxima, the counts, the counters.
struct AlmWs {
    size_t lo2, hi2, w2, cap2, mu, xi, zi, yi;   // [B][N] each
    size_t li;                              // [B][S K]
    size_t act;                             // [B][N] int8
    size_t res_i, state;                    // [B][2], [B][2][2] doubles
    size_t sl;                              // [B][2][2] maxima; zeroed from here on
    size_t st_i, it_i, flag, tot;           // [B] ints
    size_t ctr;
    size_t st_o, it_o, res_o;               // gato_box_qp_alm_update: the status, solves [B] and residuals [B][2] it has no caller for
    size_t bytes;
};
static AlmWs alm_ws(const Dims &d, size_t e)
{
    const size_t B = d.B, vN = align_up(B * d.N() * e), vB = align_up(B * sizeof(int));
    AlmWs o;
    o.lo2 = polish_ws(d, e, true, true).bytes;
    o.hi2 = o.lo2 + vN; o.w2 = o.hi2 + vN; o.cap2 = o.w2 + vN; o.mu = o.cap2 + vN; o.xi = o.mu + vN; o.zi = o.xi + vN; o.yi = o.zi + vN;
    o.li = o.yi + vN;
    o.act = o.li + align_up(B * d.sk() * e);
    o.res_i = o.act + align_up(B * d.N());
    o.state = o.res_i + align_up(B * 2 * sizeof(double));
    o.sl = o.state + align_up(B * 4 * sizeof(double));
    o.st_i = o.sl + align_up(B * 4 * 8);
    o.it_i = o.st_i + vB; o.flag = o.it_i + vB; o.tot = o.flag + vB; o.ctr = o.tot + vB;
    o.st_o = o.ctr + 256; o.it_o = o.st_o + vB; o.res_o = o.it_o + vB;
    o.bytes = o.res_o + align_up(B * 2 * sizeof(double));
    return o;
}

// The part of AlmArgs both entries fill alike: the work area at w.
static AlmArgs alm_args(char *w, const AlmWs &o, bool caps)
{
    AlmArgs a;
    memset(&a, 0, sizeof(a));
    a.lo2 = w + o.lo2; a.hi2 = w + o.hi2; a.w2 = w + o.w2; a.cap2 = caps ? w + o.cap2 : nullptr; a.mu = w + o.mu;
    a.xi = w + o.xi; a.zi = w + o.zi; a.yi = w + o.yi; a.li = w + o.li;
    a.status_i = (const int *)(w + o.st_i); a.iters_i = (const int *)(w + o.it_i); a.res_i = (const double *)(w + o.res_i);
    a.state = (double *)(w + o.state); a.slots = (unsigned long long *)(w + o.sl);
    a.flag = (int *)(w + o.flag); a.tot = (int *)(w + o.tot); a.ctr = (int *)(w + o.ctr);
    return a;
}

static bool alm_params_ok(double alm_weight, double alm_growth, double alm_weight_max)
{
    return std::isfinite(alm_weight) && alm_weight > 0 && alm_growth > 1 && alm_weight_max >= alm_weight;
}

// Per outer step: the inner run - gato_box_qp_pdas_ls's loop on the work area's bounds, weights and act, launch for launch - then
// the update and the decision and one read of the live count.  Only the decision writes the caller's arrays.
extern "C" int gato_box_qp_alm(gato_solver *s, const void *d_G_blocks, const void *d_C_blocks, const void *d_g, const void *d_c,
                               const void *d_lo, const void *d_hi, const void *d_soft_w, const void *d_soft_cap, signed char *d_act,
                               const gato_box_qp_params *p, int max_pdas_iters, double alm_weight, double alm_growth,
                               double alm_weight_max, int max_alm_iters, const void *d_mu0, void *d_x, void *d_z, void *d_y,
                               void *d_lambda, int *d_iters, int *d_status, double *d_res, int *d_outer, double *d_weight,
                               void *stream)
{
    const char *who = "box_qp_alm";
    if (check_pointers(s, who, p, d_C_blocks, {d_G_blocks, d_g, d_c, d_lo, d_hi, d_act, d_x, d_z, d_y, d_lambda, d_iters, d_status, d_res},
                       ", d_soft_w for no soft bound, d_soft_cap for no cap, d_mu0 for a zero multiplier, d_outer and d_weight"))
        return GATO_EINVAL;
    if (!reduced_params_ok(*p) || max_pdas_iters < 1 || max_alm_iters < 1) {
        set_error("%s: parameters out of range (want finite values, rho, eps_abs, eps_rel, exit_tol >= 0, max_iters, "
                  "max_pdas_iters, max_alm_iters >= 1)", who);
        return GATO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (check_not_capturing(who, "the loop reads the live count", st)) return GATO_EINVAL;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    const size_t B = s->d.B;
    const bool caps = d_soft_w && d_soft_cap;
    const AlmWs o = alm_ws(s->d, s->esz);
    int rc;
    if ((rc = grow_ws(&s->pol_ws, &s->pol_ws_bytes, o.bytes, st))) return rc;     // the inner runs find their part large enough
    char *w = s->pol_ws;
    if ((rc = start_call(w, o.sl, o.bytes, d_status, B, st))) return rc;
    AlmArgs a = alm_args(w, o, caps);
    a.lo = d_lo; a.hi = d_hi; a.w = d_soft_w; a.cap = caps ? d_soft_cap : nullptr; a.mu0 = d_mu0;
    a.act0 = d_act; a.act = (signed char *)(w + o.act); a.act_out = d_act;
    a.x = d_x; a.z = d_z; a.y = d_y; a.lam = d_lambda; a.iters = d_iters; a.status = d_status; a.outer = d_outer;
    a.res = d_res; a.weight = d_weight;
    a.alm_weight = alm_weight; a.growth = alm_growth; a.weight_max = alm_weight_max; a.eps_abs = p->eps_abs; a.eps_rel = p->eps_rel;
    const Dims d = kernel_dims(s);
    if ((rc = s->ops->alm_check(d, a, st))) return rc;
    int h[2] = {0, 0};
    GATO_HIP_CHECK(hipMemcpyAsync(h, a.ctr, sizeof(h), hipMemcpyDeviceToHost, st));
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    if (h[1] > 0) {
        set_error("%s:%s a bound is NaN, lo > hi, a weight is NaN, negative or infinite or a cap is NaN or negative (BAD_BOUNDS); "
                  "d_status marks the systems", who,
                  alm_params_ok(alm_weight, alm_growth, alm_weight_max) ? "" : " want a finite alm_weight > 0, alm_growth > 1 and "
                  "alm_weight_max >= alm_weight, or");
        return GATO_EINVAL;
    }
    // the inner runs: the work area's bounds, weights and act, their point into it, the line search without a record of its steps
    const BoxProblem inner{who, true, true, d_G_blocks, d_C_blocks, d_g, d_c, a.lo2, a.hi2, a.w2, a.cap2, a.act,
                           {w + o.xi, w + o.zi, w + o.yi, w + o.li, (int *)(w + o.it_i), (int *)(w + o.st_i), (double *)(w + o.res_i)}};
    const LineSearch ls{nullptr};
    for (int it = 1; it <= max_alm_iters; ++it) {
        rc = pdas_loop(s, inner, p, max_pdas_iters, st, &ls);
        if (rc) {                           // step 1: a start act the inner run refuses, its marks to the caller; a later
            if (it == 1) {                  // error (HIP, a hand-off time-out) leaves d_status -1 on the systems still running
                GATO_HIP_CHECK(hipMemcpyAsync(d_status, w + o.st_i, B * sizeof(int), hipMemcpyDeviceToDevice, st));
                GATO_HIP_CHECK(hipStreamSynchronize(st));
            }
            return rc;
        }
        if ((rc = s->ops->alm_update(d, a, it, it == max_alm_iters, st))) return rc;
        if (it == max_alm_iters) break;     // every system still live froze in that decision
        if ((rc = read_live(who, a.ctr, h, st))) return rc;
        if (h[0] == 0) break;
    }
    GATO_HIP_CHECK(hipStreamSynchronize(st));
    return gato_pcg_status(s, nullptr);
}

// The update and the decision alone, two launches, on a given inner point of converged inner runs.
extern "C" int gato_box_qp_alm_update(gato_solver *s, const void *d_x, const void *d_y, const void *d_lambda, void *d_mu,
                                      const double *d_w, const double *d_v_prev, const void *d_lo, const void *d_hi, const void *d_soft_w,
                                      double eps_abs, double eps_rel, double alm_growth,
                                      double alm_weight_max, int last, double *d_v, double *d_xinf, int *d_dec, void *d_lo2,
                                      void *d_hi2, void *d_w2, void *d_z, void *stream)
{
    if (!solver_usable(s, "box_qp_alm_update", "QP solves")) return GATO_EINVAL;
    if (!d_x || !d_y || !d_lambda || !d_mu || !d_w || !d_v_prev || !d_lo || !d_hi || !d_v || !d_xinf || !d_dec || !d_lo2 || !d_hi2 ||
        !d_w2 || !d_z) {
        set_error("box_qp_alm_update: every pointer is required (d_soft_w may be NULL for no soft bound)");
        return GATO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    GATO_HIP_CHECK(hipSetDevice(s->device));
    const size_t B = s->d.B;
    const AlmWs o = alm_ws(s->d, s->esz);
    int rc;
    if ((rc = grow_ws(&s->pol_ws, &s->pol_ws_bytes, o.bytes, st))) return rc;
    char *w = s->pol_ws;
    // inner status CONVERGED, residuals and solves 0; the status it has no caller for: running
    if ((rc = start_call(w, o.res_i, o.bytes, (int *)(w + o.st_o), B, st))) return rc;
    AlmArgs a = alm_args(w, o, false);
    a.lo = d_lo; a.hi = d_hi; a.w = d_soft_w;                    // the caps are not read: a capped variable has a weight and is no ALM variable
    a.xi = d_x; a.zi = d_x; a.yi = d_y; a.li = d_lambda; a.mu = d_mu; a.lo2 = d_lo2; a.hi2 = d_hi2; a.w2 = d_w2;
    a.x = w + o.xi; a.y = w + o.yi; a.lam = w + o.li; a.z = d_z;
    a.status = (int *)(w + o.st_o); a.iters = (int *)(w + o.it_o); a.res = (double *)(w + o.res_o); a.dec = d_dec;
    a.growth = alm_growth; a.weight_max = alm_weight_max; a.eps_abs = eps_abs; a.eps_rel = eps_rel;
    // set 1 of the state is step 1's: {w, v_prev} interleaved from the caller's arrays
    GATO_HIP_CHECK(hipMemcpy2DAsync(a.state + 2, 4 * sizeof(double), d_w, sizeof(double), sizeof(double), B, hipMemcpyDeviceToDevice, st));
    GATO_HIP_CHECK(hipMemcpy2DAsync(a.state + 3, 4 * sizeof(double), d_v_prev, sizeof(double), sizeof(double), B, hipMemcpyDeviceToDevice, st));
    if ((rc = s->ops->alm_update(kernel_dims(s), a, 1, last, st))) return rc;
    // the maxima of set 1, step 1's
    GATO_HIP_CHECK(hipMemcpy2DAsync(d_v, sizeof(double), a.slots + 2, 4 * 8, 8, B, hipMemcpyDeviceToDevice, st));
    GATO_HIP_CHECK(hipMemcpy2DAsync(d_xinf, sizeof(double), a.slots + 3, 4 * 8, 8, B, hipMemcpyDeviceToDevice, st));
    return GATO_OK;
}
