// Host-pointer drop-in for main_call (gpu_library.cu:85-234) and its cached solver.
#include <cstdlib>

#include "gato_solver.h"

static std::mutex g_cache_mu;
static gato_solver *g_cached_solver = nullptr;

extern "C" int gato_release_cache(void)
{
    std::lock_guard<std::mutex> lock(g_cache_mu);
    if (g_cached_solver) gato_solver_destroy(g_cached_solver);
    g_cached_solver = nullptr;
    return GATO_OK;
}

// ---- host-pointer drop-in for main_call (gpu_library.cu:85-234) -----------------------------------
template <typename T>
static int linsys_solve_host(int dtype, const int *G_row, int len_G_row, const int *G_col, const T *G_val, int nnz_G,
                             const int *C_row, int len_C_row, const int *C_col, const T *C_val, int nnz_C,
                             const T *g, int len_g, const T *c, int len_c, const T *lambda_in, int S, int C, int K,
                             int testiters, T exit_tol, int max_iters, int warm_start, T rho, T *lambda_out,
                             T *dz_out, int *iters_out, float *ms_out)
{
    (void)lambda_in; (void)warm_start;   // D5: the reference resets lambda to 0 (gato_pcg.cuh:303)
    const long long N = (long long)(S + C) * K - C;
    if (len_G_row != N + 1 || len_C_row != (long long)S * K + 1 || len_g != N || len_c != S * K ||
        nnz_G < 0 || nnz_C < 0 || testiters < 1) {
        set_error("linsys_solve: lengths do not match S=%d C=%d K=%d: len(G_row)=%d (want %lld), len(C_row)=%d "
                  "(want %d), len(g)=%d (want %lld), len(c)=%d (want %d)",
                  S, C, K, len_G_row, N + 1, len_C_row, S * K + 1, len_g, N, len_c, S * K);
        return GATO_EINVAL;
    }
    // The scatter kernel trusts the CSR arrays (as the reference does, gato_schur.cuh:674-743); an out-of-range index
    // would be an out-of-bounds device write, so the host copy is validated here (O(nnz), the arrays are in cache).
    {
        auto bad = [&](const char *name, const int *row, int nrows, const int *col, int nnz, long long ncols) -> bool {
            if (row[0] != 0) { set_error("linsys_solve: %s_row[0] must be 0", name); return true; }
            for (int i = 0; i < nrows; ++i)
                if (row[i + 1] < row[i] || row[i + 1] > nnz) {
                    set_error("linsys_solve: %s_row is not a monotone indptr at row %d", name, i);
                    return true;
                }
            for (int i = 0; i < nnz; ++i)
                if (col[i] < 0 || col[i] >= ncols) {
                    set_error("linsys_solve: %s_col[%d] = %d is outside [0, %lld)", name, i, col[i], ncols);
                    return true;
                }
            return false;
        };
        if (bad("G", G_row, len_G_row - 1, G_col, nnz_G, N) || bad("C", C_row, len_C_row - 1, C_col, nnz_C, N)) return GATO_EINVAL;
    }
    if (G_row[len_G_row - 1] != nnz_G || C_row[len_C_row - 1] != nnz_C) {
        set_error("linsys_solve: indptr[-1] does not match nnz (G %d vs %d, C %d vs %d)", G_row[len_G_row - 1], nnz_G,
                  C_row[len_C_row - 1], nnz_C);
        return GATO_EINVAL;
    }
    // The reference allocates and frees 22 device buffers per call (gpu_library.cu:36-45,140-147; gato_pcg.cuh:486-492).
    // Here the solver of the most recent (S, C, K, dtype) and its input staging area are kept for the next call.
    std::lock_guard<std::mutex> lock(g_cache_mu);
    gato_solver *&cached = g_cached_solver;
    gato_solver *s = cached;
    int rc;
    if (!s || s->d.S != S || s->d.C != C || s->d.K != K || s->dtype != dtype || s->d.B != 1) {
        if (s) gato_solver_destroy(s);
        cached = s = nullptr;
        if ((rc = gato_solver_create(S, C, K, dtype, 0, &s))) return rc;
        cached = s;
    } else {
        (void)hipSetDevice(s->device);
    }
    const char *env = getenv("GATO_PCG_MODE");
    s->pcg_mode = env ? atoi(env) : GATO_PCG_AUTO;
    const char *envp = getenv("GATO_PRECON");        // 0 stair (the reference's default build), 1 block-Jacobi, 2 point-Jacobi
    s->precon_mode = envp ? atoi(envp) : GATO_PRECON_STAIR;
    if (s->precon_mode < GATO_PRECON_STAIR || s->precon_mode > GATO_PRECON_POINT_JACOBI) s->precon_mode = GATO_PRECON_STAIR;

    size_t off = 0;
    auto take = [&](size_t b) { size_t o = off; off += align_up(b ? b : 8); return o; };
    const size_t oGr = take(sizeof(int) * len_G_row), oGc = take(sizeof(int) * nnz_G), oGv = take(sizeof(T) * nnz_G);
    const size_t oCr = take(sizeof(int) * len_C_row), oCc = take(sizeof(int) * nnz_C), oCv = take(sizeof(T) * nnz_C);
    const size_t og = take(sizeof(T) * len_g), oc = take(sizeof(T) * len_c);
    hipError_t e = hipSuccess;
    if (s->in_bytes < off) {
        if (s->in_arena) (void)hipFree(s->in_arena);
        s->in_arena = nullptr; s->in_bytes = 0;
        e = hipMalloc((void **)&s->in_arena, off);
        if (e != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", off, hipGetErrorString(e)); return GATO_EHIP; }
        s->in_bytes = off;
    }
    char *a = s->in_arena;
    hipStream_t st = nullptr;
    if (!s->host_ev[0]) {
        (void)hipEventCreate(&s->host_ev[0]);
        (void)hipEventCreate(&s->host_ev[1]);
    }
    const hipEvent_t ev0 = s->host_ev[0], ev1 = s->host_ev[1];
    auto fail = [&](int code) { return code; };
    // one H2D transfer: the eight input arrays are packed into a pinned staging buffer laid out like the device
    // arena (the reference issues eight blocking cudaMemcpy from pageable memory, gpu_library.cu:150-157)
    // lambda and dz are neighbours in the solver's arena: ONE D2H copy brings both (and the padding between them)
    const size_t dz_off = (size_t)((const char *)s->dz - (const char *)s->lambda), out_span = dz_off + sizeof(T) * (size_t)N;
    if (s->pin_bytes < off + 64 + out_span) {
        if (s->pin) (void)hipHostFree(s->pin);
        s->pin = nullptr; s->pin_bytes = 0;
        const size_t want = off + 64 + out_span + 256;
        if ((e = hipHostMalloc((void **)&s->pin, want, hipHostMallocDefault)) != hipSuccess) {
            set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            return fail(GATO_EHIP);
        }
        s->pin_bytes = want;
    }
    memcpy(s->pin + oGr, G_row, sizeof(int) * len_G_row); memcpy(s->pin + oGc, G_col, sizeof(int) * nnz_G);
    memcpy(s->pin + oGv, G_val, sizeof(T) * nnz_G);       memcpy(s->pin + oCr, C_row, sizeof(int) * len_C_row);
    memcpy(s->pin + oCc, C_col, sizeof(int) * nnz_C);     memcpy(s->pin + oCv, C_val, sizeof(T) * nnz_C);
    memcpy(s->pin + og, g, sizeof(T) * len_g);            memcpy(s->pin + oc, c, sizeof(T) * len_c);
    if ((e = hipMemcpyAsync(a, s->pin, off, hipMemcpyHostToDevice, st)) != hipSuccess) {
        set_error("H2D copy failed: %s", hipGetErrorString(e));
        return fail(GATO_EHIP);
    }
    char *pout = s->pin + off;                               // pinned landing area: iters | lambda | dz
    int iters = 0;
    for (int i = 0; i < testiters; ++i) {                       // gpu_library.cu:169-192
        (void)hipEventRecord(ev0, st);
        rc = gato_linsys_device(s, (const int *)(a + oGr), (const int *)(a + oGc), a + oGv, (const int *)(a + oCr),
                                (const int *)(a + oCc), a + oCv, a + og, a + oc, (double)exit_tol, max_iters,
                                (double)rho, nullptr, nullptr, st);
        if (rc) return fail(rc);
        if ((e = hipMemcpyAsync(pout + 64, s->lambda, out_span, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipMemcpyAsync(pout, s->iters, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) {
            set_error("D2H copy failed: %s", hipGetErrorString(e));
            return fail(GATO_EHIP);
        }
        (void)hipEventRecord(ev1, st);
        if ((e = hipEventSynchronize(ev1)) != hipSuccess) {
            set_error("solve failed: %s", hipGetErrorString(e));
            return fail(GATO_EHIP);
        }
        iters = *(const int *)pout;
        if (iters < 0) {
            // in-band time-out mark of a persistent launch (its workgroups were not co-resident): slower correct answer
            // through the streaming kernels instead of an error, then fetch the results again
            int recovered = 0;
            if ((rc = gato_solver_recover(s, &recovered, st))) return fail(rc);
            if ((e = hipMemcpy(pout + 64, s->lambda, out_span, hipMemcpyDeviceToHost)) != hipSuccess ||
                (e = hipMemcpy(pout, s->iters, sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) {
                set_error("D2H copy failed: %s", hipGetErrorString(e));
                return fail(GATO_EHIP);
            }
            (void)hipEventRecord(ev1, st);
            (void)hipEventSynchronize(ev1);
            iters = *(const int *)pout;
        }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        if (ms_out) ms_out[i] = ms;
        if (i == 0 && iters_out) *iters_out = iters;            // the reference prints the first run's count (:189-191)
    }
    memcpy(lambda_out, pout + 64, sizeof(T) * (size_t)S * K);
    memcpy(dz_out, pout + 64 + dz_off, sizeof(T) * (size_t)N);
    return fail(GATO_OK);
}

extern "C" int gato_linsys_solve_f32(const int *G_row, int len_G_row, const int *G_col, const float *G_val, int nnz_G,
                                     const int *C_row, int len_C_row, const int *C_col, const float *C_val, int nnz_C,
                                     const float *g, int len_g, const float *c, int len_c, const float *lambda_in,
                                     int S, int C, int K, int testiters, float exit_tol, int max_iters, int warm_start,
                                     float rho, float *lambda_out, float *dz_out, int *iters_out, float *ms_out)
{
    return linsys_solve_host<float>(GATO_F32, G_row, len_G_row, G_col, G_val, nnz_G, C_row, len_C_row, C_col, C_val,
                                    nnz_C, g, len_g, c, len_c, lambda_in, S, C, K, testiters, exit_tol, max_iters,
                                    warm_start, rho, lambda_out, dz_out, iters_out, ms_out);
}

extern "C" int gato_linsys_solve_f64(const int *G_row, int len_G_row, const int *G_col, const double *G_val, int nnz_G,
                                     const int *C_row, int len_C_row, const int *C_col, const double *C_val, int nnz_C,
                                     const double *g, int len_g, const double *c, int len_c, const double *lambda_in,
                                     int S, int C, int K, int testiters, double exit_tol, int max_iters, int warm_start,
                                     double rho, double *lambda_out, double *dz_out, int *iters_out, float *ms_out)
{
    return linsys_solve_host<double>(GATO_F64, G_row, len_G_row, G_col, G_val, nnz_G, C_row, len_C_row, C_col, C_val,
                                     nnz_C, g, len_g, c, len_c, lambda_in, S, C, K, testiters, exit_tol, max_iters,
                                     warm_start, rho, lambda_out, dz_out, iters_out, ms_out);
}

// List-level re-solve: the system of the most recent gato_linsys_solve_* (the cached solver) for a new g / c.
template <typename T>
static int linsys_resolve_host(int dtype, const T *g, int len_g, const T *c, int len_c, T exit_tol, int max_iters,
                               T *lambda_out, T *dz_out, int *iters_out)
{
    const char *name = dtype == GATO_F32 ? "f32" : "f64";
    if (!g || !c || !lambda_out || !dz_out) { set_error("linsys_resolve_%s: null argument", name); return GATO_EINVAL; }
    std::lock_guard<std::mutex> lock(g_cache_mu);
    gato_solver *s = g_cached_solver;
    if (!s) {
        set_error("linsys_resolve_%s: no system to re-solve: call gato_linsys_solve_%s first (none since the library was loaded "
                  "or since gato_release_cache)", name, name);
        return GATO_EINVAL;
    }
    if (s->dtype != dtype) {
        set_error("linsys_resolve_%s: the most recent linsys_solve ran in %s", name, s->dtype == GATO_F32 ? "f32" : "f64");
        return GATO_EINVAL;
    }
    const int S = s->d.S, K = s->d.K;
    const long long N = (long long)s->d.N();
    if (len_g != N || len_c != S * K) {
        set_error("linsys_resolve_%s: lengths do not match the last solve (S=%d C=%d K=%d): len(g)=%d (want %lld), len(c)=%d "
                  "(want %d)", name, S, s->d.C, K, len_g, N, len_c, S * K);
        return GATO_EINVAL;
    }
    if (!s->as.valid) { set_error("linsys_resolve_%s: the last solve did not complete", name); return GATO_EINVAL; }
    (void)hipSetDevice(s->device);
    // the staging areas of the solve (its inputs included g and c) are large enough for g | c here
    const size_t oc = align_up(sizeof(T) * (size_t)N), off = oc + align_up(sizeof(T) * (size_t)S * K);
    const size_t dz_off = (size_t)((const char *)s->dz - (const char *)s->lambda), out_span = dz_off + sizeof(T) * (size_t)N;
    if (!s->in_arena || s->in_bytes < off || !s->pin || s->pin_bytes < off + 64 + out_span) {
        set_error("linsys_resolve_%s: the cached solver has no staging area", name);
        return GATO_EINVAL;
    }
    hipStream_t st = nullptr;
    hipError_t e;
    memcpy(s->pin, g, sizeof(T) * (size_t)N);
    memcpy(s->pin + oc, c, sizeof(T) * (size_t)S * K);
    char *a = s->in_arena, *pout = s->pin + off;
    if ((e = hipMemcpyAsync(a, s->pin, off, hipMemcpyHostToDevice, st)) != hipSuccess) {
        set_error("H2D copy failed: %s", hipGetErrorString(e));
        return GATO_EHIP;
    }
    int rc = gato_solve_rhs(s, 1, a, a + oc, (double)exit_tol, max_iters, s->lambda, s->dz, s->iters, st);
    if (rc) return rc;
    if ((e = hipMemcpyAsync(pout + 64, s->lambda, out_span, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(pout, s->iters, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess) {
        set_error("re-solve failed: %s", hipGetErrorString(e));
        return GATO_EHIP;
    }
    int iters = *(const int *)pout;
    if (iters < 0) {                     // in-band time-out mark of a persistent launch: re-run through the streaming kernels
        int recovered = 0;
        if ((rc = gato_solver_recover(s, &recovered, st))) return rc;
        if ((e = hipMemcpy(pout + 64, s->lambda, out_span, hipMemcpyDeviceToHost)) != hipSuccess ||
            (e = hipMemcpy(pout, s->iters, sizeof(int), hipMemcpyDeviceToHost)) != hipSuccess) {
            set_error("D2H copy failed: %s", hipGetErrorString(e));
            return GATO_EHIP;
        }
        iters = *(const int *)pout;
    }
    if (iters_out) *iters_out = iters;
    memcpy(lambda_out, pout + 64, sizeof(T) * (size_t)S * K);
    memcpy(dz_out, pout + 64 + dz_off, sizeof(T) * (size_t)N);
    return GATO_OK;
}

extern "C" int gato_linsys_resolve_f32(const float *g, int len_g, const float *c, int len_c, float exit_tol, int max_iters,
                                       float *lambda_out, float *dz_out, int *iters_out)
{
    return linsys_resolve_host<float>(GATO_F32, g, len_g, c, len_c, exit_tol, max_iters, lambda_out, dz_out, iters_out);
}

extern "C" int gato_linsys_resolve_f64(const double *g, int len_g, const double *c, int len_c, double exit_tol, int max_iters,
                                       double *lambda_out, double *dz_out, int *iters_out)
{
    return linsys_resolve_host<double>(GATO_F64, g, len_g, c, len_c, exit_tol, max_iters, lambda_out, dz_out, iters_out);
}

