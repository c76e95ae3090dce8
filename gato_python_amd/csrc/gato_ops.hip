// Type-erased op table of libgato_hip.so: one Ops entry per compiled (STATE_SIZE, CONTROL_SIZE, dtype).
#include <vector>

#include "gato_common.h"

namespace gato {

// ---- type-erased op table -------------------------------------------------------------------
template <typename T, int S, int C>
static Ops make_ops(int dtype)
{
    Ops o;
    o.S = S; o.C = C; o.dtype = dtype;
    o.convert = [](const Dims &d, const int *gr, const int *gc, const void *gv, const int *cr, const int *cc,
                   const void *cv, double rho, void *Gd, void *Cd, void *Gi, hipStream_t st) {
        return launch_convert<T, S, C>(d, gr, gc, (const T *)gv, cr, cc, (const T *)cv, (T)rho, (T *)Gd, (T *)Cd, (T *)Gi, st);
    };
    o.add_rho = [](const Dims &d, const void *Gin, double rho, void *Gd, hipStream_t st) {
        return launch_add_rho<T, S, C>(d, (const T *)Gin, (T)rho, (T *)Gd, st);
    };
    o.form_schur = [](const Dims &d, const void *Gd, const void *Cd, const void *g, const void *c, void *Sb,
                      void *Pb, void *gam, void *Gi, bool have_inv, hipStream_t st) {
        return launch_form_schur<T, S, C>(d, (const T *)Gd, (const T *)Cd, (const T *)g, (const T *)c, (T *)Sb,
                                          (T *)Pb, (T *)gam, (T *)Gi, have_inv, st);
    };
    o.assemble = [](const Dims &d, const AsmArgs &a, hipStream_t st) { return launch_assemble<T, S, C>(d, a, st); };
    o.form_ss = [](const Dims &d, const void *Sb, void *Pb, hipStream_t st) {
        return launch_form_ss<T, S, C>(d, (const T *)Sb, (T *)Pb, st);
    };
    o.point_jacobi = [](const Dims &d, const void *Sb, void *Pb, hipStream_t st) {
        return launch_point_jacobi<T, S, C>(d, (const T *)Sb, (T *)Pb, st);
    };
    o.compute_dz = [](const Dims &d, const void *Gi, const void *Cd, const void *g, const void *lam, void *dz,
                      hipStream_t st) {
        return launch_compute_dz<T, S, C>(d, (const T *)Gi, (const T *)Cd, (const T *)g, (const T *)lam, (T *)dz, st);
    };
    o.rhs_gamma = [](const Dims &d, int R, const void *Gi, const void *Cd, const void *Sb, const void *g, const void *c,
                     void *gam, hipStream_t st) {
        return launch_rhs_gamma<T, S, C>(d, R, (const T *)Gi, (const T *)Cd, (const T *)Sb, (const T *)g, (const T *)c,
                                         (T *)gam, st);
    };
    o.grad_blocks = [](const Dims &d, const void *dz, const void *lam, const void *a, const void *beta, void *Gb, void *Cb,
                       hipStream_t st) {
        return launch_grad_blocks<T, S, C>(d, (const T *)dz, (const T *)lam, (const T *)a, (const T *)beta, (T *)Gb, (T *)Cb, st);
    };
    o.grad_csr = [](const Dims &d, const int *gr, const int *gc, int nG, const int *cr, const int *cc, int nC, const void *dz,
                    const void *lam, const void *a, const void *beta, void *Gb, void *Cb, hipStream_t st) {
        return launch_grad_csr<T, S, C>(d, gr, gc, nG, cr, cc, nC, (const T *)dz, (const T *)lam, (const T *)a,
                                        (const T *)beta, (T *)Gb, (T *)Cb, st);
    };
    o.qp_prepare = [](const Dims &d, const QpArgs &a, hipStream_t st) { return launch_qp_prepare<T, S, C>(d, a, st); };
    o.qp_update = [](const Dims &d, const QpArgs &a, int it, int last, hipStream_t st) {
        return launch_qp_update<T, S, C>(d, a, it, last, st);
    };
    o.qp_active = [](const Dims &d, const void *z, const void *y, const void *lo, const void *hi, signed char *act, hipStream_t st) {
        return launch_qp_active<T, S, C>(d, z, y, lo, hi, act, st);
    };
    o.polish_prepare = [](const Dims &d, const PolishArgs &a, hipStream_t st) { return launch_polish_prepare<T, S, C>(d, a, st); };
    o.polish_finish = [](const Dims &d, const PolishArgs &a, hipStream_t st) { return launch_polish_finish<T, S, C>(d, a, st); };
    o.qp_bound_grad = [](const Dims &d, const BoundGradArgs &a, hipStream_t st) { return launch_qp_bound_grad<T, S, C>(d, a, st); };
    o.kkt_tangent_rhs = [](const Dims &d, int R, const TangentArgs &a, hipStream_t st) { return launch_kkt_tangent_rhs<T, S, C>(d, R, a, st); };
    o.pdas_check = [](const Dims &d, const PdasArgs &a, hipStream_t st) { return launch_pdas_check<T, S, C>(d, a, st); };
    o.pdas_step = [](const Dims &d, const PdasArgs &a, int it, hipStream_t st) { return launch_pdas_step<T, S, C>(d, a, it, st); };
    o.pdas_decide = [](const Dims &d, const PdasArgs &a, int it, int last, hipStream_t st) {
        return launch_pdas_decide<T, S, C>(d, a, it, last, st);
    };
    o.ls_scope = [](const Dims &d, const LineSearchArgs &a, hipStream_t st) { return launch_ls_scope<T, S, C>(d, a, st); };
    o.line_search = [](const Dims &d, const LineSearchArgs &a, hipStream_t st) { return launch_line_search<T, S, C>(d, a, st); };
    o.alm_check = [](const Dims &d, const AlmArgs &a, hipStream_t st) { return launch_alm_check<T, S, C>(d, a, st); };
    o.alm_update = [](const Dims &d, const AlmArgs &a, int it, int last, hipStream_t st) {
        return launch_alm_update<T, S, C>(d, a, it, last, st);
    };
    o.pcg_plan = [](PcgPlan *p) { return pcg_resident_plan<T, S>(p); };
    o.pcg_resident = [](const PcgLaunch &a, hipStream_t st) { return launch_pcg_resident<T, S>(a, st); };   // incl. the DPP-row layout
    o.pcg_dma_max_knots = []() { return pcg_dma_max_knots<T, S>(); };
    o.pcg_dma = [](const PcgLaunch &a, hipStream_t st) { return launch_pcg_dma<T, S>(a, st); };
    o.pcg_cg1_max_threads = []() { return pcg_cg1_max_threads<T, S>(); };
    o.pcg_cg1 = [](const PcgLaunch &a, hipStream_t st) { return launch_pcg_cg1<T, S>(a, st); };
    o.stream_grid = [](int K, int mg) { return stream_grid<T, S>(K, mg); };
    o.stream_step = [](int ph, const StreamStep &a, int grid, hipStream_t st) { return launch_stream_step<T, S>(ph, a, grid, st); };
    o.stream_pack = [](const void *sl, int n, const void *y, int K, void *send, hipStream_t st) {
        return launch_stream_pack<T, S>(sl, n, y, K, send, st);
    };
    o.stream_finish = [](const void *part, int n, int stride, double tol, int last_it, int *done, int *iters,
                         double *fe, double *hist, hipStream_t st) {
        return launch_stream_finish<T, S>(part, n, stride, tol, last_it, done, iters, fe, hist, st);
    };
    o.pcg_streaming = [](const Dims &d, const void *Sb, const void *Pb, const void *gam, void *lam, double tol,
                         int max_iters, int *iters, const PcgStreamWork &w, hipStream_t st) {
        return launch_pcg_streaming<T, S>(d, (const T *)Sb, (const T *)Pb, (const T *)gam, (T *)lam, (T)tol,
                                          max_iters, iters, w, st);
    };
    return o;
}

static const std::vector<Ops> &all_ops()
{
    static const std::vector<Ops> v = [] {
        std::vector<Ops> t;
#define X(S_, C_)                                     \
    t.push_back(make_ops<float, S_, C_>(GATO_F32));   \
    t.push_back(make_ops<double, S_, C_>(GATO_F64));
        GATO_SHAPES(X)
#undef X
        return t;
    }();
    return v;
}

const Ops *find_ops(int S, int C, int dtype)
{
    for (const Ops &o : all_ops())
        if (o.S == S && o.C == C && o.dtype == dtype) return &o;
    return nullptr;
}

}  // namespace gato
