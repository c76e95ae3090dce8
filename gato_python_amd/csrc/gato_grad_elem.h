// One entry of M_bar, shared by grad_cross_kernel (gato_cross.hip) and grad_csr_kernel<..., CROSS = true>
// (gato_grad.hip) so that a CSR cross entry's gradient is bit for bit the block gradient of its slot.  Internal header.
#pragma once
#include "gato_common.h"

namespace gato {
namespace {

// Entry w of M_bar_k = -(a_x,k dz_u,k^T + dz_x,k a_u,k^T) in M's layout (S x C column-major), dz and a of one system.
// Contraction off, as grad_G_elem: p + q is one rounding of two rounded products.
template <typename T, int S, int C>
__device__ __forceinline__ T grad_M_elem(const T *__restrict__ dz, const T *__restrict__ a, size_t k, int w)
{
#pragma clang fp contract(off)
    constexpr int n = S + C;
    const int i = w % S, j = w / S;
    const T *dzs = dz + k * n, *as = a + k * n;
    const T p = as[i] * dzs[S + j];
    const T q = dzs[i] * as[S + j];
    return -(p + q);
}

}  // namespace
}  // namespace gato
