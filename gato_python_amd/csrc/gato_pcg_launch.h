// Host helpers shared by the launchers of the persistent PCG kernels (gato_pcg_resident*.hip, gato_pcg_cg1.hip, gato_pcg_dma.hip).
#pragma once
#include "gato_common.h"

namespace gato {

typedef void (*PcgKernel)(PcgLaunch);

// The knot range of a launch.  A cluster launch (mr: one rank of a multi-GPU solve) works on the shard [k_begin, k_end) of the
// K knots and the shard is checked; any other launch works on all of them and its shard fields are set accordingly.
// unserved: the launch asks for something `who` does not serve in a cluster.  *Kl: the knots this launch works on.
inline int pcg_shard(PcgLaunch &a, bool mr, bool unserved, const char *who, int *Kl)
{
    if (!mr) { a.k_begin = 0; a.k_end = a.K; a.rank = 0; a.nranks = 1; }
    *Kl = a.k_end - a.k_begin;
    if (mr && (unserved || a.nranks < 1 || a.nranks > GATO_MAX_RANKS || a.rank < 0 || a.rank >= a.nranks || a.k_begin < 0 || *Kl < 1 ||
               a.k_end > a.K || (a.rank == 0) != (a.k_begin == 0) || (a.rank == a.nranks - 1) != (a.k_end == a.K))) {
        set_error("%s(cluster): bad shard rank=%d/%d knots [%d,%d) of %d", who, a.rank, a.nranks, a.k_begin, a.k_end, a.K);
        return GATO_EINVAL;
    }
    return GATO_OK;
}

// groups workgroups of knots_per_wg knots each cover the Kl knots of the launch and none of them is empty
inline bool pcg_groups_cover(const PcgLaunch &a, int Kl)
{
    return (long long)a.groups * a.knots_per_wg >= Kl && (long long)(a.groups - 1) * a.knots_per_wg < Kl;
}

// One persistent launch between the caller's timing events.  No re-initialisation of the hand-off area in front of it: granules
// carry epochs from the solver's ever-growing counter and the status word is matched against this launch's id.
// coop: option coop_launch (A12: cudaLaunchCooperativeKernel + check_sms, gato_pcg.cuh:502-526, gato_utils.cuh:829-854) - the
// multi-workgroup kernels through hipLaunchCooperativeKernel, so that the RUNTIME keeps the launch from starting before all
// its workgroups can be resident (kernels of other streams and processes included), instead of this library's own gate over
// its own launches.  Measured cost and verdict: DESIGN.md 3.1b.
inline int pcg_launch(PcgKernel kernel, dim3 grid, dim3 block, const PcgLaunch &a, hipStream_t st, bool coop = false)
{
    if (a.ev_start) GATO_HIP_CHECK(hipEventRecord(a.ev_start, st));
    if (coop) {
        PcgLaunch arg = a;
        void *args[] = {(void *)&arg};
        (void)hipLaunchCooperativeKernel(reinterpret_cast<const void *>(kernel), grid, block, args, 0, st);
    } else hipLaunchKernelGGL(kernel, grid, block, 0, st, a);
    GATO_HIP_CHECK(hipGetLastError());
    if (a.ev_stop) GATO_HIP_CHECK(hipEventRecord(a.ev_stop, st));
    return GATO_OK;
}

}  // namespace gato
