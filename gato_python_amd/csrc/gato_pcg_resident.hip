// Resident PCG, host side: what the planner may ask for (pcg_resident_plan) and the dispatch of a launch to the variants of
// pcg_resident_kernel (gato_pcg_resident_kernel.h: every row resident, semi-resident, no resident rows), to the DPP-row
// instantiations (gato_pcg_resident_dpp.hip) and to the one-workgroup two-rows-per-lane kernels (gato_pcg_resident_single.hip).
#include "gato_pcg_resident_launch.h"

namespace gato {

template <typename T, int S>
int pcg_resident_plan(PcgPlan *plan)
{
    plan->max_threads = MaxThreads<T, S>::v;
    plan->max_knots_per_wg = MaxThreads<T, S>::v / S;
    plan->single_max_threads = SingleCu<T, S>::threads;
    plan->pair_threads = (sizeof(T) == 4 && S % 2 == 0) ? PairThreads<S>::v : 0;
    plan->mixed_rows = sizeof(T) == 8 ? mixed_rows<S>() : 0;
    plan->mixed_threads = sizeof(T) == 8 ? 64 * MixedCfg<S>::wt : 0;
    plan->semi_threads = SemiThreads<T, S>::v;
    plan->semi_rows = SemiRows<T, S>::v;
    plan->nores_threads = NoresThreads<T, S>::v;
    plan->nores_rows = NoresRows<T, S>::v;
    plan->dpp_lanes = DppRows<S>::ok ? DppRows<S>::lanes : 0;
    return GATO_OK;
}

template <typename T, int S>
int launch_pcg_resident(const PcgLaunch &a0, hipStream_t st)
{
    // cluster launch (one rank of a multi-GPU solve): the MR instantiations, geometry over the rank's knot range
    const bool mr = a0.xslots != nullptr;
    PcgLaunch a = a0;
    int Kl;                                             // knots this launch works on
    if (pcg_shard(a, mr, a.pair || a.batch > 1 || a.xcd_pack || a.stamps, "pcg_resident", &Kl) != GATO_OK) return GATO_EINVAL;
    if (a.dpp_rows) {
        if (a.pair || a.semi) {
            set_error("pcg_resident: the DPP-row layout serves the plain and the cluster launches only");
            return GATO_EINVAL;
        }
        return launch_pcg_resident_dpp<T, S>(a, st);
    }
    // the one-workgroup kernels with two rows per lane (pair = 1: fp32; 2: fp64 mixed rows): a translation unit of their own
    if (a.pair) return launch_pcg_single<T, S>(a, mr, st);
    if constexpr (SemiThreads<T, S>::v > 0) {
        if (a.semi == 1) {
            constexpr int XT = SemiThreads<T, S>::v, XR = SemiRows<T, S>::v;
            const long long extra_rows = ((long long)a.knots_per_wg - a.threads / S) * S;
            if (a.batch > 1 || a.threads != XT || a.groups < (mr ? 1 : 2) || a.groups > 256 || a.threads / S < 2 ||
                extra_rows > (long long)XR * a.threads || !pcg_groups_cover(a, Kl)) {
                set_error("pcg_resident(semi): bad launch geometry (K=%d groups=%d knots/wg=%d threads=%d)", a.K, a.groups,
                          a.knots_per_wg, a.threads);
                return GATO_EINVAL;
            }
            return pcg_launch(mr ? pcg_resident_kernel<T, S, XT, 0, 0, XR, false, true> : pcg_resident_kernel<T, S, XT, 0, 0, XR>,
                              dim3(a.groups), dim3(a.threads), a, st, a.coop);
        }
    }
    if constexpr (NoresThreads<T, S>::v > 0) {
        if (a.semi == 2) {
            constexpr int NT = NoresThreads<T, S>::v, NX = NoresRows<T, S>::v;
            if (a.batch > 1 || a.threads != NT || a.groups < (mr ? 1 : 2) || a.groups > 256 ||
                (long long)a.knots_per_wg * S > (long long)NX * NT || !pcg_groups_cover(a, Kl)) {
                set_error("pcg_resident(no resident rows): bad launch geometry (K=%d groups=%d knots/wg=%d threads=%d)", a.K,
                          a.groups, a.knots_per_wg, a.threads);
                return GATO_EINVAL;
            }
            return pcg_launch(mr ? pcg_resident_kernel<T, S, NT, 0, 0, NX, true, true> : pcg_resident_kernel<T, S, NT, 0, 0, NX, true>,
                              dim3(a.groups), dim3(a.threads), a, st, a.coop);
        }
    }
    return launch_plain<T, S, false>(a, mr, Kl, st);
}

#define X(S_, C_)                                                      \
    template int pcg_resident_plan<float, S_>(PcgPlan *);              \
    template int pcg_resident_plan<double, S_>(PcgPlan *);             \
    template int launch_pcg_resident<float, S_>(const PcgLaunch &, hipStream_t); \
    template int launch_pcg_resident<double, S_>(const PcgLaunch &, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
