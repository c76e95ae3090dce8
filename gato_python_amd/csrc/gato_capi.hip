// C ABI of libgato_hip.so (include/gato_hip.h): solver object, stage-level entry points on device
// pointers, the device-resident whole solve and the host-pointer drop-in for main_call
// (gpu_library.cu:85-234).
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include "gato_solver.h"

namespace gato {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace gato

using namespace gato;

bool solver_usable(const gato_solver *s, const char *entry, const char *unsupported)
{
    if (!s) set_error("%s: null solver", entry);
    else if (s->cl.on || s->cl.local) set_error("%s: the solver is a cluster rank; sharded %s are not supported", entry, unsupported);
    else return true;
    return false;
}

extern "C" const char *gato_last_error(void) { return g_err; }
extern "C" int gato_version(void) { return 100; }

extern "C" int gato_num_shapes(void)
{
    int n = 0;
#define X(S_, C_) ++n;
    GATO_SHAPES(X)
#undef X
    return n;
}

extern "C" int gato_shape(int i, int *S, int *C)
{
    int n = 0;
#define X(S_, C_)              \
    if (n++ == i) {            \
        *S = S_; *C = C_;      \
        return GATO_OK;        \
    }
    GATO_SHAPES(X)
#undef X
    return GATO_EINVAL;
}

extern "C" int gato_device_info(int device, int *num_cus, int *lds_bytes, char *name, int name_len)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device visible");
        return GATO_ENODEV;
    }
    hipDeviceProp_t p;
    GATO_HIP_CHECK(hipGetDeviceProperties(&p, device));
    if (num_cus) *num_cus = p.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)p.sharedMemPerBlock;
    if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    return GATO_OK;
}

extern "C" int gato_infer_shape(const int *C_row, int len_C_row, int len_g, int len_c, int *S, int *C, int *K)
{
    // S = number of leading rows of C holding exactly one entry (row-block 0 = identity,
    // gato_schur.cuh:725); then K = len_c / S and C from N = (S+C)K - C.
    if (!C_row || len_C_row != len_c + 1 || len_c <= 0 || len_g <= 0) {
        set_error("infer_shape: len(C_row)=%d must be len(c)+1=%d", len_C_row, len_c + 1);
        return GATO_EINVAL;
    }
    int s = 0;
    while (s < len_c && C_row[s + 1] - C_row[s] == 1) ++s;
    if (s == 0 || len_c % s != 0) {
        // all rows single-entry (K == 1) or no identity block: fall back to the compiled shapes
        for (int i = 0; i < gato_num_shapes(); ++i) {
            int ss, cc;
            gato_shape(i, &ss, &cc);
            if (len_c % ss == 0) {
                int k = len_c / ss;
                if ((long long)(ss + cc) * k - cc == len_g) { *S = ss; *C = cc; *K = k; return GATO_OK; }
            }
        }
        set_error("infer_shape: cannot infer S from C_row (leading identity rows = %d, len(c) = %d)", s, len_c);
        return GATO_EINVAL;
    }
    int k = len_c / s;
    if (k == 1) {
        if (len_g != s) { set_error("infer_shape: K=1 needs len(g) == S"); return GATO_EINVAL; }
        *S = s; *K = 1; *C = 0;
        for (int i = 0; i < gato_num_shapes(); ++i) { int ss, cc; gato_shape(i, &ss, &cc); if (ss == s) *C = cc; }
        return GATO_OK;
    }
    long long num = (long long)len_g - (long long)s * k;   // = C*(K-1)
    if (num < 0 || num % (k - 1) != 0) {
        set_error("infer_shape: len(g)=%d inconsistent with S=%d K=%d", len_g, s, k);
        return GATO_EINVAL;
    }
    *S = s; *K = k; *C = (int)(num / (k - 1));
    return GATO_OK;
}

extern "C" int gato_solver_create(int S, int C, int K, int dtype, int device, gato_solver **out)
{
    return gato_solver_create_batched(S, C, K, 1, dtype, device, out);
}

extern "C" int gato_solver_create_batched(int S, int C, int K, int B, int dtype, int device, gato_solver **out)
{
    if (B < 1 || B > 65535) {           // the batched launches take one grid row (blockIdx.y) per system
        set_error("solver_create: batch must be in 1 .. 65535 (got %d); split larger batches over several calls", B);
        return GATO_EINVAL;
    }
    if (!out || K < 1 || (dtype != GATO_F32 && dtype != GATO_F64)) {
        set_error("solver_create: bad arguments (K=%d dtype=%d)", K, dtype);
        return GATO_EINVAL;
    }
    const Ops *ops = find_ops(S, C, dtype);
    if (!ops) {
        set_error("solver_create: (STATE_SIZE=%d, CONTROL_SIZE=%d) is not a compiled shape", S, C);
        return GATO_ESHAPE;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device >= count) {
        set_error("solver_create: no HIP device %d (visible devices: %d)", device, count);
        return GATO_ENODEV;
    }
    GATO_HIP_CHECK(hipSetDevice(device));
    gato_solver *s = new gato_solver();
    memset(s, 0, sizeof(*s));
    s->d = Dims{S, C, K};
    s->d.B = B;
    s->dtype = dtype;
    s->device = device;
    s->esz = dtype == GATO_F32 ? 4 : 8;
    s->ops = ops;
    hipDeviceProp_t p;
    GATO_HIP_CHECK(hipGetDeviceProperties(&p, device));
    s->num_cus = p.multiProcessorCount;
    ops->pcg_plan(&s->plan);
    s->pcg_mode = GATO_PCG_AUTO;
    s->xcd_pack = -1;
    s->xcd_sel = -1;
    s->wave_pub = 1;
    s->dpp_rows = -1;
    s->pcg_semi = -1;
    s->timeout_ms = 2000;
    s->cluster_flat = 1;

    const Dims &d = s->d;
    const size_t e = s->esz;
    const int max_groups = 4096;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes ? bytes : 8); return o; };
    // status block first, granules right behind it: one memset re-initialises both before a launch
    const size_t o_status = take(64);
    const int slot_g = pcg_slot_granules(S, (int)e) > pcg_slot_granules_cg1(S, (int)e) ? pcg_slot_granules(S, (int)e)
                                                                                        : pcg_slot_granules_cg1(S, (int)e);
    const size_t o_slots = take((size_t)2 * 256 * slot_g * 8);
    s->slots_bytes = (size_t)2 * 256 * slot_g * 8;
    const size_t nb = (size_t)B;
    const size_t o_G = take(d.g_dense() * e * nb), o_C = take(d.c_dense() * e * nb), o_Gi = take(d.g_dense() * e * nb);
    const size_t o_S = take(d.bd() * e * nb), o_P = take(d.bd() * e * nb), o_gam = take(d.sk() * e * nb);
    const size_t o_lam = take(d.sk() * e * nb), o_dz = take(d.N() * e * nb);
    const size_t o_its = take(sizeof(int) * nb);
    const size_t o_vec = take(6 * d.sk() * e);
    const size_t o_part = take((size_t)4 * max_groups * e), o_scal = take(64 * 8), o_done = take(64);
    const size_t o_gh = take((size_t)8 * S * e);
    const size_t o_hist = take(sizeof(double) * (GATO_ETA_HIST_MAX + 1));
    const size_t o_xtab = take(sizeof(void *) * GATO_MAX_RANKS);
    // images for the one-workgroup two-rows-per-lane kernels (one system whose rows fit one of them)
    const long long rows = (long long)K * S;
    const bool img = B == 1 && ((s->plan.pair_threads > 0 && rows <= 2ll * s->plan.pair_threads) || (s->plan.mixed_rows > 0 && rows <= s->plan.mixed_rows));
    int img_ld = 0;
    if (img) {
        img_ld = (int)((rows + 63) / 64 * 64) + 128;                    // every lane of the launch reads inside its column
        if (img_ld < s->plan.mixed_rows) img_ld = s->plan.mixed_rows;
    }
    const size_t o_iS = take(img ? (size_t)3 * S * img_ld * e : 0), o_iP = take(img ? (size_t)3 * S * img_ld * e : 0);
    s->arena_bytes = off;
    GATO_HIP_CHECK(hipMalloc((void **)&s->arena, off));
    GATO_HIP_CHECK(hipMemset(s->arena, 0, off));
    char *a = s->arena;
    s->slots = (unsigned long long *)(a + o_slots);
    s->status = (int *)(a + o_status);
    s->iters = B > 1 ? (int *)(a + o_its) : (int *)(a + o_status + 8);
    s->final_eta = (double *)(a + o_status + 16);
    s->tune_status = (int *)(a + o_status + 32); s->tune_iters = (int *)(a + o_status + 40); s->tune_eta = (double *)(a + o_status + 48);
    s->dz_flag = (int *)(a + o_status + 56);
    s->G_dense = a + o_G; s->C_dense = a + o_C; s->Ginv = a + o_Gi;
    s->Sbd = a + o_S; s->Pbd = a + o_P; s->gamma = a + o_gam; s->lambda = a + o_lam; s->dz = a + o_dz;
    s->sw.vecs = a + o_vec;
    s->sw.partials = a + o_part; s->sw.scalars = a + o_scal; s->sw.done = (int *)(a + o_done);
    s->sw.max_groups = max_groups;
    s->ghosts = a + o_gh;
    s->eta_hist = (double *)(a + o_hist);
    s->cl_tab = (unsigned long long **)(a + o_xtab);
    if (img) { s->imgS = a + o_iS; s->imgP = a + o_iP; s->img_ld = img_ld; }
    // placement of the one-XCD launches of the default geometry: measured here, where the caller waits anyway
    // (allocation, memset), never inside an enqueue-only entry.  GATO_NO_TUNE=1 skips it (XCD 0).
    const char *nt = getenv("GATO_NO_TUNE");
    if (!(nt && atoi(nt))) {
        const int rc = gato_solver_tune(s, nullptr);
        if (rc) { gato_solver_destroy(s); return rc; }
    }
    *out = s;
    return GATO_OK;
}

extern "C" int gato_solver_destroy(gato_solver *s)
{
    if (!s) return GATO_OK;
    (void)hipSetDevice(s->device);
    gato_cluster_destroy(s);
    if (s->ev_pcg0) (void)hipEventDestroy(s->ev_pcg0);
    if (s->ev_pcg1) (void)hipEventDestroy(s->ev_pcg1);
    if (s->ev_cal0) (void)hipEventDestroy(s->ev_cal0);
    if (s->ev_cal1) (void)hipEventDestroy(s->ev_cal1);
    for (int i = 0; i < 4; ++i)
        if (s->ev_stage[i]) (void)hipEventDestroy(s->ev_stage[i]);
    if (s->arena) (void)hipFree(s->arena);
    if (s->rhs_ws) (void)hipFree(s->rhs_ws);
    if (s->qp_ws) (void)hipFree(s->qp_ws);
    if (s->pol_ws) (void)hipFree(s->pol_ws);
    if (s->cross_ws) (void)hipFree(s->cross_ws);
    if (s->cross_rhs_ws) (void)hipFree(s->cross_rhs_ws);
    if (s->in_arena) (void)hipFree(s->in_arena);
    for (int i = 0; i < 2; ++i)
        if (s->host_ev[i]) (void)hipEventDestroy(s->host_ev[i]);
    if (s->pin) (void)hipHostFree(s->pin);
    delete s;
    return GATO_OK;
}

extern "C" void *gato_solver_buffer(gato_solver *s, int which)
{
    switch (which) {
        case 0: return s->G_dense;
        case 1: return s->C_dense;
        case 2: return s->Ginv;
        case 3: return s->Sbd;
        case 4: return s->Pbd;
        case 5: return s->gamma;
        case 6: return s->lambda;
        case 7: return s->dz;
        case 8: return s->iters;
        case 9: return (unsigned long long *)s->sw.scalars + 8;   // diagnostic stamps (option stamp_pcg)
        case 10: return s->eta_hist;                              // double[max_iters + 1] (option record_eta)
        case 11: return s->rhs_ws;                                // gamma of the re-solves [B][rhs_R][S K] (nullptr: none reserved)
        case 12: return s->qp_pcg_total;                          // PCG iterations per system of the latest box QP solve [B] (int)
        case 13: case 14: case 15: case 16: {                      // the cross-term work area: G', C', W, g' (nullptr: no cross solve yet)
            if (!s->cross_ws) return nullptr;
            const size_t e = s->esz, nb = (size_t)s->d.B;
            size_t off = 0;
            if (which > 13) off += align_up(s->d.g_dense() * e * nb);
            if (which > 14) off += align_up(s->d.c_dense() * e * nb);
            if (which > 15) off += align_up((size_t)(s->d.K - 1) * s->d.S * s->d.C * e * nb);
            return s->cross_ws + off;
        }
        default: return nullptr;
    }
}

extern "C" int gato_solver_set_option(gato_solver *s, const char *name, int value)
{
    if (!strcmp(name, "pcg_mode")) s->pcg_mode = value;
    else if (!strcmp(name, "pcg_threads")) s->pcg_threads = value;
    else if (!strcmp(name, "pcg_groups")) s->pcg_groups = value;
    else if (!strcmp(name, "asm_mode")) s->asm_mode = value;
    else if (!strcmp(name, "pcg_semi")) s->pcg_semi = value;
    else if (!strcmp(name, "pcg_epoch")) s->pcg_epoch = (unsigned)value;      // test hook: place the counter near its wrap
    else if (!strcmp(name, "cluster_epoch")) s->cl.xepoch = (unsigned)value;  // test hook: the cluster's counter near its end (every rank alike)
    else if (!strcmp(name, "stamp_asm")) s->stamp_asm = value;
    else if (!strcmp(name, "stamp_pcg")) s->stamp_pcg = value;
    else if (!strcmp(name, "ablate")) s->ablate = value;
    else if (!strcmp(name, "no_single_lds")) s->no_single_lds = value;
    else if (!strcmp(name, "no_pair")) s->no_pair = value;
    else if (!strcmp(name, "wave_pub")) s->wave_pub = value;
    else if (!strcmp(name, "dpp_rows")) s->dpp_rows = value;
    else if (!strcmp(name, "pcg_variant")) s->pcg_variant = value;
    else if (!strcmp(name, "record_eta")) s->record_eta = value;
    else if (!strcmp(name, "xcd_pack")) s->xcd_pack = value;
    else if (!strcmp(name, "xcd_sel")) s->xcd_sel = value < 0 ? -1 : (value & 7);
    else if (!strcmp(name, "true_warm_start")) s->true_warm_start = value;
    else if (!strcmp(name, "timeout_ms")) s->timeout_ms = value > 0 ? value : 2000;
    else if (!strcmp(name, "max_workgroups")) s->max_workgroups = value;
    else if (!strcmp(name, "no_fuse_dz")) s->no_fuse_dz = value;
    else if (!strcmp(name, "no_image")) s->no_image = value;
    else if (!strcmp(name, "qp_cross_unfused")) s->qp_cross_unfused = value;
    else if (!strcmp(name, "cross_tangent_form")) s->cross_tangent_form = value;
    else if (!strcmp(name, "cross_csr_threads")) s->cross_csr_threads = value;
    else if (!strcmp(name, "coop_launch")) s->coop_launch = value;
    else if (!strcmp(name, "cluster_flat")) s->cluster_flat = value;
    else if (!strcmp(name, "knot_lo") || !strcmp(name, "knot_hi")) {          // stage-level entries: knots [knot_lo, knot_hi)
        if (value < 0 || value > s->d.K) { set_error("%s = %d is outside [0, %d]", name, value, s->d.K); return GATO_EINVAL; }
        (name[5] == 'l' ? s->d.k_lo : s->d.k_hi) = value;
    }
    else if (!strcmp(name, "precon_mode")) {
        if (value < GATO_PRECON_STAIR || value > GATO_PRECON_POINT_JACOBI) { set_error("precon_mode must be 0, 1 or 2"); return GATO_EINVAL; }
        s->precon_mode = value;
    }
    else if (!strcmp(name, "time_stages")) {
        s->time_stages = value;
        if (value && !s->ev_stage[0])
            for (int i = 0; i < 4; ++i) GATO_HIP_CHECK(hipEventCreate(&s->ev_stage[i]));
    }
    else if (!strcmp(name, "batch_nnz_G")) s->d.nnzG = value;
    else if (!strcmp(name, "batch_nnz_C")) s->d.nnzC = value;
    else if (!strcmp(name, "time_pcg")) {
        s->time_pcg = value;
        if (value && !s->ev_pcg0) {
            GATO_HIP_CHECK(hipEventCreate(&s->ev_pcg0));
            GATO_HIP_CHECK(hipEventCreate(&s->ev_pcg1));
        }
    }
    else { set_error("unknown option %s", name); return GATO_EINVAL; }
    return GATO_OK;
}

extern "C" int gato_pcg_last_ms(gato_solver *s, float *ms)
{
    if (!s->time_pcg || !s->ev_pcg0) { set_error("pcg_last_ms: option time_pcg is off"); return GATO_EINVAL; }
    GATO_HIP_CHECK(hipEventSynchronize(s->ev_pcg1));
    GATO_HIP_CHECK(hipEventElapsedTime(ms, s->ev_pcg0, s->ev_pcg1));
    return GATO_OK;
}

// Stage times of the most recent whole solve as data (the reference prints "Forming Schur took" and the solve time,
// gato_schur.cuh:907-913,972-982; gpu_library.cu:186-198): ms[0] = CSR scatter + Schur + preconditioner, ms[1] = PCG,
// ms[2] = dz.  Needs option time_stages = 1; synchronises on the last event.
extern "C" int gato_last_stage_ms(gato_solver *s, float *ms)
{
    if (!s->time_stages || !s->ev_stage[0]) { set_error("last_stage_ms: option time_stages is off"); return GATO_EINVAL; }
    GATO_HIP_CHECK(hipEventSynchronize(s->ev_stage[3]));
    for (int i = 0; i < 3; ++i) GATO_HIP_CHECK(hipEventElapsedTime(ms + i, s->ev_stage[i], s->ev_stage[i + 1]));
    return GATO_OK;
}

extern "C" int gato_solver_get_option(gato_solver *s, const char *name, int *value)
{
    if (!strcmp(name, "pcg_mode")) *value = s->pcg_mode;
    else if (!strcmp(name, "pcg_threads")) *value = s->pcg_threads;
    else if (!strcmp(name, "pcg_groups")) *value = s->pcg_groups;
    else if (!strcmp(name, "last_groups")) *value = s->last_groups;
    else if (!strcmp(name, "last_threads")) *value = s->last_threads;
    else if (!strcmp(name, "last_mode")) *value = s->last_mode;
    else if (!strcmp(name, "last_pair")) *value = s->last_pair;
    else if (!strcmp(name, "last_dpp")) *value = s->last_dpp;
    else if (!strcmp(name, "last_xcd_sel")) *value = s->last_xcd_sel;
    else if (!strcmp(name, "last_variant")) *value = s->last_variant;
    else if (!strcmp(name, "asm_mode")) *value = s->asm_mode;
    else if (!strcmp(name, "last_asm_fused")) *value = s->last_asm_fused;
    else if (!strcmp(name, "last_image")) *value = s->last_image;
    else if (!strcmp(name, "last_semi")) *value = s->last_semi;
    else if (!strcmp(name, "last_fallback")) *value = s->last_fallback;
    else if (!strcmp(name, "last_dz_fused")) *value = s->dz_fused;
    else if (!strcmp(name, "last_cluster_flat")) *value = s->cl.on ? s->cl.last_flat : 0;
    else if (!strcmp(name, "timeout_ms")) *value = s->timeout_ms;
    else if (!strcmp(name, "precon_mode")) *value = s->precon_mode;
    else if (!strcmp(name, "cluster_mem_kind")) *value = s->cl.on ? s->cl.mem_kind : -1;
    else if (!strcmp(name, "num_cus")) *value = s->num_cus;
    else if (!strcmp(name, "batch")) *value = s->d.B;
    else if (!strcmp(name, "rhs_reserved")) *value = s->rhs_R;
    else if (!strcmp(name, "assembly_valid")) *value = s->as.valid;
    else if (!strcmp(name, "assembly_gen")) *value = (int)s->as.gen;     // wraps: compare for equality only
    else if (!strcmp(name, "true_warm_start")) *value = s->true_warm_start;
    else if (!strcmp(name, "max_semi_knots"))
        *value = s->plan.semi_threads > 0 ? (s->plan.semi_threads / s->d.S + s->plan.semi_rows * s->plan.semi_threads / s->d.S) * (s->num_cus < 256 ? s->num_cus : 256) : 0;
    else if (!strcmp(name, "max_resident_knots")) *value = s->plan.max_knots_per_wg * (s->num_cus < 256 ? s->num_cus : 256);
    else { set_error("unknown option %s", name); return GATO_EINVAL; }
    return GATO_OK;
}

// ---- stage-level entry points -------------------------------------------------------------------
// A stage entry that writes into the solver's own workspace may overwrite the blocks of the latest assembly: the re-solve
// (gato_solve_rhs) then has nothing it can trust any more.
static bool owned(const gato_solver *s, const void *p)
{
    const char *q = (const char *)p;
    return q && ((q >= s->arena && q < s->arena + s->arena_bytes) || (s->rhs_ws && q >= s->rhs_ws && q < s->rhs_ws + s->rhs_ws_bytes));
}
static void note_stage_outputs(gato_solver *s, const void *a, const void *b, const void *c = nullptr, const void *d = nullptr)
{
    if (owned(s, a) || owned(s, b) || owned(s, c) || owned(s, d)) s->as.valid = 0;
}

extern "C" int gato_convert(gato_solver *s, const int *d_G_row, const int *d_G_col, const void *d_G_val,
                            const int *d_C_row, const int *d_C_col, const void *d_C_val, double rho,
                            void *d_G_dense, void *d_C_dense, void *stream)
{
    note_stage_outputs(s, d_G_dense, d_C_dense);
    if (s->d.B > 1 && (s->d.nnzG <= 0 || s->d.nnzC <= 0)) {
        set_error("convert: a batched solver needs the per-system nnz (gato_linsys_device_batched, or options "
                  "batch_nnz_G / batch_nnz_C)");
        return GATO_EINVAL;
    }
    return s->ops->convert(s->d, d_G_row, d_G_col, d_G_val, d_C_row, d_C_col, d_C_val, rho, d_G_dense, d_C_dense,
                           nullptr, (hipStream_t)stream);
}

extern "C" int gato_form_schur(gato_solver *s, const void *d_G_dense, const void *d_C_dense, const void *d_g,
                               const void *d_c, void *d_S, void *d_Pinv, void *d_gamma, void *d_Ginv_dense,
                               void *stream)
{
    note_stage_outputs(s, d_S, d_Pinv, d_gamma, d_Ginv_dense);
    return s->ops->form_schur(s->d, d_G_dense, d_C_dense, d_g, d_c, d_S, d_Pinv, d_gamma, d_Ginv_dense, false,
                              (hipStream_t)stream);
}

extern "C" int gato_form_ss(gato_solver *s, const void *d_S, void *d_Pinv, void *stream)
{
    note_stage_outputs(s, d_Pinv, nullptr);
    return s->ops->form_ss(s->d, d_S, d_Pinv, (hipStream_t)stream);
}

extern "C" int gato_compute_dz(gato_solver *s, const void *d_Ginv_dense, const void *d_C_dense, const void *d_g,
                               const void *d_lambda, void *d_dz, void *stream)
{
    return s->ops->compute_dz(s->d, d_Ginv_dense, d_C_dense, d_g, d_lambda, d_dz, (hipStream_t)stream);
}

