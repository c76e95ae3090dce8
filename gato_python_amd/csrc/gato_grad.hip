// Gradients of a KKT solve with respect to its blocks (gato_kkt_grad_blocks / gato_kkt_grad_csr): the backward pass of
// M x = b, M = [[G + rho I, C^T], [C, 0]], x = [dz; lambda], b = [g; c].  With the adjoint [a; beta] = M^-1 [dz_bar; lam_bar]
// (a re-solve of the same assembly, M is symmetric) the matrix gradients are, per knot k:
//   Q_bar_k = -1/2 (a_x,k dz_x,k^T + dz_x,k a_x,k^T),  R_bar_k likewise with the u-parts   (symmetric perturbations)
//   A_bar_k = -(beta_k+1 dz_x,k^T + lambda_k+1 a_x,k^T),  B_bar_k = -(beta_k+1 dz_u,k^T + lambda_k+1 a_u,k^T)
// Both kernels evaluate an output entry through the same two device functions, so a CSR entry's gradient is bit for bit
// the block gradient at the slot the forward scatter wrote it into.  Nothing here reads the assembly: four vectors in.
#include "gato_cross_device.h"
#include "gato_grad_elem.h"

namespace gato {
namespace {

constexpr int NT = 256;

// Entry w of knot k's [Q_k | R_k] block (G_dense layout, column-major).  Contraction off: p + q is one rounding of two
// rounded products, so the result does not depend on how the call site is compiled, and Q_bar is exactly symmetric.
template <typename T, int S, int C>
__device__ __forceinline__ T grad_G_elem(const T *__restrict__ dz, const T *__restrict__ a, int k, int w)
{
#pragma clang fp contract(off)
    constexpr int n = S + C, SS = S * S;
    int base, i, j;
    if (w < SS) { i = w % S; j = w / S; base = k * n; }
    else { w -= SS; i = w % C; j = w / C; base = k * n + S; }
    const T p = a[base + i] * dz[base + j];
    const T q = dz[base + i] * a[base + j];
    return (T)-0.5 * (p + q);
}

// Entry w of knot k's [A_k | B_k] block (C_dense layout, column-major, S rows): row (k+1) S + w % S of C, column
// k n + w / S of the KKT unknowns (x_k then u_k).
template <typename T, int S, int C>
__device__ __forceinline__ T grad_C_elem(const T *__restrict__ dz, const T *__restrict__ lam, const T *__restrict__ a,
                                         const T *__restrict__ beta, int k, int w)
{
#pragma clang fp contract(off)
    constexpr int n = S + C;
    const int row = (k + 1) * S + w % S, col = k * n + w / S;
    const T p = beta[row] * dz[col];
    const T q = lam[row] * a[col];
    return -(p + q);
}

// One launch for both outputs: a flat index over [B][g_dense] then [B][c_dense], E consecutive elements per lane and one
// 16-byte store where the destination allows (the per-system strides may be odd, so the batch is one flat array).
template <typename T, int S, int C>
__global__ __launch_bounds__(NT) void grad_blocks_kernel(const T *__restrict__ dz, const T *__restrict__ lam,
                                                         const T *__restrict__ a, const T *__restrict__ beta,
                                                         T *__restrict__ Gbar, T *__restrict__ Cbar, size_t nG, size_t nC,
                                                         size_t vG, size_t vC, BatchStride bs)
{
    constexpr int E = 16 / sizeof(T);
    constexpr int KG = S * S + C * C, KC = S * S + S * C;
    typedef T V __attribute__((ext_vector_type(E)));
    const size_t v = (size_t)blockIdx.x * NT + threadIdx.x;
    if (v >= vG + vC) return;
    const bool isG = v < vG;
    const size_t e0 = (isG ? v : v - vG) * E, total = isG ? nG : nC, per = isG ? bs.g : bs.c;
    T *out = isG ? Gbar : Cbar;
    size_t sys = e0 / per, r = e0 - sys * per;
    T val[E];
#pragma unroll
    for (int u = 0; u < E; ++u) {
        val[u] = (T)0;
        if (e0 + u >= total) continue;
        if (r >= per) { r -= per; ++sys; }                                // per >= 4 >= E: at most one wrap per vector
        const int knot = (int)(r / (isG ? KG : KC)), w = (int)(r - (size_t)knot * (isG ? KG : KC));
        val[u] = isG ? grad_G_elem<T, S, C>(dz + sys * bs.n, a + sys * bs.n, knot, w)
                     : grad_C_elem<T, S, C>(dz + sys * bs.n, lam + sys * bs.sk, a + sys * bs.n, beta + sys * bs.sk, knot, w);
        ++r;
    }
    if (e0 + E <= total && ((uintptr_t)(out + e0) & 15) == 0) {
        V o;
#pragma unroll
        for (int u = 0; u < E; ++u) o[u] = val[u];
        *(V *)(out + e0) = o;
    } else {
        for (int u = 0; u < E && e0 + u < total; ++u) out[e0 + u] = val[u];
    }
}

// largest i in [0, nrows) with ptr[i] <= e, -1 if e lies before ptr[0] or from ptr[nrows] on
__device__ __forceinline__ int row_of(const int *__restrict__ ptr, int nrows, int e)
{
    if (nrows <= 0 || e < ptr[0] || e >= ptr[nrows]) return -1;
    int lo = 0, hi = nrows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

constexpr int SYS_PER = 8;   // systems per thread of the CSR kernel: the slot of an entry is found once for all of them

// The chain rule through the forward scatter (gather_kernel / assemble_kernel, gato_assembly.hip): entry e of a CSR row
// carries the gradient of the dense slot it was written into, or 0 when the scatter dropped it (rows of C's block row 0,
// C columns beyond the block row, G entries between the Q and R parts) or a later entry of the same row wrote that slot
// again (the last entry in storage order wins).  Thread = entry (G entries first, then C), grid.y = groups of systems.
// CROSS (gato_kkt_grad_csr_cross): the scatter is cross_prepare_csr_kernel's, where a G entry of a state
// row with a control column in a knot k < K - 1 is M_k's and carries M_bar at its slot (grad_M_elem, the expression of
// grad_cross_kernel); its mirror, such an entry in the last knot and an overwritten one get 0.  Everything else as without.
template <typename T, int S, int C, bool CROSS>
__global__ __launch_bounds__(NT) void grad_csr_kernel(const int *__restrict__ G_row, const int *__restrict__ G_col, int nnzG,
                                                      const int *__restrict__ C_row, const int *__restrict__ C_col, int nnzC,
                                                      const T *__restrict__ dz, const T *__restrict__ lam,
                                                      const T *__restrict__ a, const T *__restrict__ beta,
                                                      T *__restrict__ Gbar, T *__restrict__ Cbar, int K, int B, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S;
    bool isM = false;
    const int nG = Gbar ? nnzG : 0, nC = Cbar ? nnzC : 0;
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= nG + nC) return;
    const bool isG = t < nG;
    const int e = isG ? t : t - nG;
    int knot = -1, w = 0;
    if (isG) {
        const int N = n * K - C;
        const int row = row_of(G_row, N, e), col = G_col[e];
        if (row >= 0 && col >= 0) {
            const int isr = row % n, isc = col % n;
            isM = CROSS && isr < S && isc >= S && row / n < K - 1;
            if ((isr < S) == (isc < S) || isM) {
                knot = row / n;
                w = isM ? (isc - S) * S + isr : isc < S ? isc * S + isr : SS + (isc - S) * C + (isr - S);
                for (int e2 = e + 1; e2 < G_row[row + 1] && e2 < nnzG; ++e2) {
                    const int c2 = G_col[e2];
                    if (c2 >= 0 && c2 % n == isc) { knot = -1; break; }
                }
            }
        }
    } else {
        const int row = row_of(C_row, S * K, e), col = C_col[e];
        const int br = row / S - 1;
        if (row >= S && col >= 0 && col / n <= br) {
            knot = br;
            w = (col % n) * S + row % S;
            for (int e2 = e + 1; e2 < C_row[row + 1] && e2 < nnzC; ++e2) {
                const int c2 = C_col[e2];
                if (c2 >= 0 && c2 % n == col % n && c2 / n <= br) { knot = -1; break; }
            }
        }
    }
    const int s1 = min(B, (int)(blockIdx.y + 1) * SYS_PER);
    for (int sys = blockIdx.y * SYS_PER; sys < s1; ++sys) {
        const T *dzs = dz + (size_t)sys * bs.n, *as = a + (size_t)sys * bs.n;
        T v = (T)0;
        if (knot >= 0)
            v = isM ? grad_M_elem<T, S, C>(dzs, as, (size_t)knot, w)
                : isG ? grad_G_elem<T, S, C>(dzs, as, knot, w)
                      : grad_C_elem<T, S, C>(dzs, lam + (size_t)sys * bs.sk, as, beta + (size_t)sys * bs.sk, knot, w);
        if (isG) Gbar[(size_t)sys * nnzG + e] = v;
        else Cbar[(size_t)sys * nnzC + e] = v;
    }
}

}  // namespace

template <typename T, int S, int C>
int launch_grad_blocks(const Dims &d, const T *dz, const T *lam, const T *a, const T *beta, T *Gbar, T *Cbar, hipStream_t st)
{
    constexpr int E = 16 / sizeof(T);
    const BatchStride bs = batch_stride(d);
    const size_t nG = Gbar ? (size_t)d.B * bs.g : 0, nC = Cbar ? (size_t)d.B * bs.c : 0;
    const size_t vG = (nG + E - 1) / E, vC = (nC + E - 1) / E, blocks = (vG + vC + NT - 1) / NT;
    if (blocks == 0) return GATO_OK;
    if (blocks > 0x7fffffff) { set_error("kkt_grad_blocks: %zu elements are beyond one launch", nG + nC); return GATO_EINVAL; }
    hipLaunchKernelGGL((grad_blocks_kernel<T, S, C>), dim3((unsigned)blocks), dim3(NT), 0, st, dz, lam, a, beta, Gbar, Cbar,
                       nG, nC, vG, vC, bs);
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

template <typename T, int S, int C, bool CROSS>
int launch_grad_csr(const Dims &d, const int *G_row, const int *G_col, int nnzG, const int *C_row, const int *C_col, int nnzC,
                    const T *dz, const T *lam, const T *a, const T *beta, T *Gbar, T *Cbar, hipStream_t st)
{
    const long long ent = (long long)(Gbar ? nnzG : 0) + (Cbar ? nnzC : 0);
    if (ent == 0) return GATO_OK;
    const long long bx = (ent + NT - 1) / NT, by = (d.B + SYS_PER - 1) / SYS_PER;
    if (bx > 0x7fffffff || by > 65535) {
        set_error("%s: %lld entries x %d systems are beyond one launch", CROSS ? "kkt_grad_csr_cross" : "kkt_grad_csr", ent, d.B);
        return GATO_EINVAL;
    }
    hipLaunchKernelGGL((grad_csr_kernel<T, S, C, CROSS>), dim3((unsigned)bx, (unsigned)by), dim3(NT), 0, st, G_row, G_col, nnzG,
                       C_row, C_col, nnzC, dz, lam, a, beta, Gbar, Cbar, d.K, d.B, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

#define X(S_, C_)                                                                                                       \
    template int launch_grad_blocks<float, S_, C_>(const Dims &, const float *, const float *, const float *,          \
                                                   const float *, float *, float *, hipStream_t);                      \
    template int launch_grad_blocks<double, S_, C_>(const Dims &, const double *, const double *, const double *,      \
                                                    const double *, double *, double *, hipStream_t);                  \
    template int launch_grad_csr<float, S_, C_>(const Dims &, const int *, const int *, int, const int *, const int *, \
                                                int, const float *, const float *, const float *, const float *,       \
                                                float *, float *, hipStream_t);                                        \
    template int launch_grad_csr<double, S_, C_>(const Dims &, const int *, const int *, int, const int *,             \
                                                 const int *, int, const double *, const double *, const double *,     \
                                                 const double *, double *, double *, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato

int grad_csr_cross(const Dims &d, int dtype, const int *G_row, const int *G_col, int nnzG, const int *C_row, const int *C_col, int nnzC,
                   const void *dz, const void *lam, const void *a, const void *beta, void *Gbar, void *Cbar, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_)                                                                                           \
    launch_grad_csr<T, S_, C_, true>(d, G_row, G_col, nnzG, C_row, C_col, nnzC, (const T *)dz, (const T *)lam, (const T *)a,   \
                                     (const T *)beta, (T *)Gbar, (T *)Cbar, st)
    GATO_CROSS_DISPATCH("kkt_grad_csr_cross");
#undef GATO_CROSS_LAUNCH
}
