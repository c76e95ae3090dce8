// CSR entry to the cross solve: the gather of gather_kernel (gato_assembly.hip) and the change of
// variables of cross_prepare_kernel (gato_cross.hip) in one launch, so that a G whose state rows hold control columns costs
// no more launches than the block form.
// SCATTER RULE.  Addressing is gather_kernel's: knot = row / n, in-knot column = col % n (the knot of the column is not looked
// at), a slot written twice keeps the LAST entry in storage order, explicit zeros are values.  New: a G entry with isr < S,
// isc >= S in a knot k < K - 1 lands in M_k[isr + (isc - S) S] (S x C column-major, the layout of gato_linsys_device_blocks_cross).
// The mirror entries (isr >= S, isc < S) are not read: the solver takes G as symmetric, and where the two triangles disagree
// the state-row one counts.  State rows of the last knot have no M: a control column there is dropped, as everywhere before.
// rho is NOT added while gathering: the work area's G' is "without rho", as gato_cross_prepare takes its blocks, and the whole
// solve adds rho to every diagonal entry - the plain CSR path adds it to the diagonal entries the CSR stores, so the two differ
// exactly on a diagonal entry that is not stored.
// One workgroup per knot, grid.x strides over the knots, grid.y = system (shared index arrays, own values).  The transform calls
// cross_transform_knot (gato_cross_device.h) on the LDS blocks, as cross_prepare_kernel does: one writer and one chain of fused
// multiply-adds over the ascending inner index per output element, so the work area equals, bit for bit, gato_cross_prepare on
// the scattered blocks, whatever the workgroup size.
#include "gato_cross_device.h"

namespace gato {
namespace {

constexpr int WAVE = 64;

// largest i in [0, nrows) with ptr[i] <= e  (ptr[0] <= e < ptr[nrows]); row_of_entry of gato_assembly.hip
__device__ __forceinline__ int csr_row_of(const int *ptr, int nrows, int e)
{
    int lo = 0, hi = nrows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T, int S, int C, int NT>
__global__ __launch_bounds__(NT) void cross_prepare_csr_kernel(CrossCsrArgs a, int K, BatchStride bs)
{
    constexpr int n = S + C, SS = S * S, CC = C * C, SC = S * C, ABS = SS + SC;
    static_assert(NT % WAVE == 0, "whole waves");
    // Q_k | R_k | A^_k | B^_k | M_k: the first two are knot k of G_dense, the next two of C_dense
    constexpr int OR = SS, OA = SS + CC, OB = OA + SS, OM = OA + ABS, NSLOT = OM + SC;
    __shared__ T blk[NSLOT], sW[SC], sRi[CC], sg[n];
    __shared__ int sPtrG[n + 1], sPtrC[S + 1];
    // collisions: gather_kernel's rule and fast path (a bit per slot, owners only in a workgroup that saw a bit set twice)
    __shared__ unsigned smask[(NSLOT + 31) / 32];
    __shared__ int sown[NSLOT];
    __shared__ int s_coll;
    T *sQ = blk, *sR = blk + OR, *sA = blk + OA, *sB = blk + OB, *sM = blk + OM;
    const int tid = threadIdx.x;
    const size_t sys = blockIdx.y, ms = (size_t)(K - 1) * SC;
    const int *__restrict__ G_row = a.G_row, *__restrict__ G_col = a.G_col, *__restrict__ C_row = a.C_row, *__restrict__ C_col = a.C_col;
    const T *__restrict__ G_val = (const T *)a.G_val + sys * bs.nnzG, *__restrict__ C_val = (const T *)a.C_val + sys * bs.nnzC;
    const T *__restrict__ g = (const T *)a.g + sys * bs.n;
    T *Gp = (T *)a.Gp + sys * bs.g, *Cp = (T *)a.Cp + sys * bs.c, *W = (T *)a.W + sys * ms, *gp = (T *)a.gp + sys * bs.n;
    T *Go = a.G_out ? (T *)a.G_out + sys * bs.g : nullptr, *Co = a.C_out ? (T *)a.C_out + sys * bs.c : nullptr;
    T *Mo = a.M_out ? (T *)a.M_out + sys * ms : nullptr;
    const T rho = (T)a.rho;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const bool last = k == K - 1;
        const int r0 = k * n, nrG = last ? S : n;
        const int c0 = (k + 1) * S, nrC = last ? 0 : S;
        const size_t gb = (size_t)k * (SS + CC), v0 = (size_t)k * n;
        __syncthreads();                                                     // the previous knot's readers are done
        for (int i = tid; i <= nrG; i += NT) sPtrG[i] = G_row[r0 + i];
        if (nrC) for (int i = tid; i <= nrC; i += NT) sPtrC[i] = C_row[c0 + i];
        for (int i = tid; i < NSLOT; i += NT) blk[i] = (T)0;
        for (int i = tid; i < (NSLOT + 31) / 32; i += NT) smask[i] = 0u;
        for (int i = tid; i < nrG; i += NT) sg[i] = g[v0 + i];
        if (tid == 0) s_coll = 0;
        __syncthreads();
        const int eG0 = sPtrG[0], nG = sPtrG[nrG] - eG0;
        const int eC0 = nrC ? sPtrC[0] : 0, nC = nrC ? sPtrC[nrC] - eC0 : 0;
        // destination slot in blk of entry t given its column, -1 if the entry is dropped (the rule above)
        auto slot_of = [&](int t, int colv) -> int {
            if (t < nG) {
                const int isr = csr_row_of(sPtrG, nrG, eG0 + t);
                const int isc = colv % n;
                if (isc < S) return isr < S ? isc * S + isr : -1;             // Q; the mirror of M is not read
                if (isr >= S) return OR + (isc - S) * C + (isr - S);          // R
                return last ? -1 : OM + (isc - S) * S + isr;                  // M; the last knot has none
            }
            const int i = csr_row_of(sPtrC, nrC, eC0 + (t - nG));
            return colv / n <= k ? OA + (colv % n) * S + i : -1;
        };
        constexpr int U = 4;
        for (int t0 = tid; t0 < nG + nC; t0 += NT * U) {
            int col[U];
            T val[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * NT;
                if (t < nG) { col[u] = G_col[eG0 + t]; val[u] = G_val[eG0 + t]; }
                else if (t < nG + nC) { col[u] = C_col[eC0 + (t - nG)]; val[u] = C_val[eC0 + (t - nG)]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * NT;
                if (t < nG + nC) {
                    const int sl = slot_of(t, col[u]);
                    if (sl >= 0) {
                        blk[sl] = val[u];
                        const unsigned bit = 1u << (sl & 31);
                        if (atomicOr(&smask[sl >> 5], bit) & bit) s_coll = 1;
                    }
                }
            }
        }
        __syncthreads();
        if (s_coll) {                                                        // workgroup-uniform; never taken for duplicate-free rows
            for (int i = tid; i < NSLOT; i += NT) sown[i] = -1;
            __syncthreads();
            for (int pass = 0; pass < 2; ++pass) {
                for (int t = tid; t < nG + nC; t += NT) {
                    const int colv = t < nG ? G_col[eG0 + t] : C_col[eC0 + (t - nG)];
                    const int sl = slot_of(t, colv);
                    if (sl < 0) continue;
                    // (within a row storage order = index order; entries of different rows never share a slot)
                    if (pass == 0) atomicMax(&sown[sl], t);
                    else if (sown[sl] == t) blk[sl] = t < nG ? G_val[eG0 + t] : C_val[eC0 + (t - nG)];
                }
                __syncthreads();
            }
        }
        // the scattered blocks, for callers that go on with them (each NULL or written whole)
        if (Go) for (int i = tid; i < SS + (last ? 0 : CC); i += NT) Go[gb + i] = blk[i];
        if (last) {                                                          // no M: Q and g_x as they are
            for (int e = tid; e < SS; e += NT) Gp[gb + e] = sQ[e];
            if (tid < S) gp[v0 + tid] = sg[tid];
            continue;
        }
        const size_t cb = (size_t)k * ABS, mb = (size_t)k * SC;
        if (Co) for (int i = tid; i < ABS; i += NT) Co[cb + i] = sA[i];
        if (Mo) for (int i = tid; i < SC; i += NT) Mo[mb + i] = sM[i];
        cross_transform_knot<T, S, C, NT>(sQ, sR, sA, sB, sM, sg, sW, sRi, rho, tid, Gp, gb, Cp, cb, W, mb, gp, v0);
    }
}

template <typename T, int S, int C>
int launch_prepare_csr(const Dims &d, const CrossCsrArgs &a, int threads, hipStream_t st)
{
    if (d.B < 1 || d.B > 65535) { set_error("cross_prepare_csr: B = %d", d.B); return GATO_EINVAL; }
    const dim3 grid(knot_grid(d.K), d.B);
    if (threads == WAVE) hipLaunchKernelGGL((cross_prepare_csr_kernel<T, S, C, WAVE>), grid, dim3(WAVE), 0, st, a, d.K, batch_stride(d));
    else hipLaunchKernelGGL((cross_prepare_csr_kernel<T, S, C, 256>), grid, dim3(256), 0, st, a, d.K, batch_stride(d));
    GATO_HIP_CHECK(hipGetLastError());
    return GATO_OK;
}

}  // namespace
}  // namespace gato

int cross_prepare_csr(const Dims &d, int dtype, const CrossCsrArgs &a, int threads, hipStream_t st)
{
#define GATO_CROSS_LAUNCH(T, S_, C_) launch_prepare_csr<T, S_, C_>(d, a, threads, st)
    GATO_CROSS_DISPATCH("cross term");
#undef GATO_CROSS_LAUNCH
}
