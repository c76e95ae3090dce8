// launch_plain: the launcher of the every-row-resident instantiations of pcg_resident_kernel, shared by the two translation
// units that compile them (gato_pcg_resident.hip: lane = row; gato_pcg_resident_dpp.hip: the DPP-row layout).
#pragma once
#include "gato_pcg_geometry.h"
#include "gato_pcg_launch.h"
#include "gato_pcg_resident_kernel.h"

namespace gato {

// The plain and the cluster launches (every row register resident): geometry check and the hand-off form.  DR: the DPP-row
// layout.
template <typename T, int S, bool DR>
int launch_plain(const PcgLaunch &a, bool mr, int Kl, hipStream_t st)
{
    constexpr int LPK = DR ? DppRows<S>::lanes : S;
    constexpr int MAXT0 = MaxThreads<T, S>::v;
    constexpr int SINGLE_T = SingleCu<T, S>::threads;
    const bool single_lds = !DR && !mr && SINGLE_T > MAXT0 && a.groups == 1 && a.threads > MAXT0 && a.threads <= SINGLE_T;
    const int MAXT = single_lds ? SINGLE_T : MAXT0;
    if (a.batch > 1 && a.groups != 1) {
        set_error("pcg_resident: a batch needs one workgroup per system");
        return GATO_EINVAL;
    }
    if ((DR && a.stamps) || a.threads > MAXT || a.threads % 64 != 0 || a.threads < 2 * S || a.knots_per_wg * LPK > a.threads ||
        a.groups < 1 || a.groups > 256 || !pcg_groups_cover(a, Kl)) {
        set_error("pcg_resident: bad launch geometry (K=%d groups=%d knots/wg=%d threads=%d max=%d)", a.K,
                  a.groups, a.knots_per_wg, a.threads, MAXT);
        return GATO_EINVAL;
    }
    const int nblocks = a.batch > 1 ? a.batch
                      : (a.xcd_pack > 0 ? 8 * ((a.groups + a.xcd_pack - 1) / a.xcd_pack) : a.groups);
    const dim3 grid(nblocks), block(a.threads);
    if constexpr (SINGLE_T > 0 && !DR) {
        if (single_lds) {
            constexpr int NL = SingleCu<T, S>::nl;
            return pcg_launch(a.stamps ? pcg_resident_kernel<T, S, SINGLE_T, NL, 1>
                              : a.diag == 2 ? pcg_resident_kernel<T, S, SINGLE_T, NL, 2> : pcg_resident_kernel<T, S, SINGLE_T, NL>,
                              grid, block, a, st);
        }
    }
    // Hand-off form of the plain and the cluster launches (option wave_pub, default 1): ghost blocks in registers always;
    // per-wave published partials where a sweep - W << ceil(log2(waves)) granules - is at most 4 loads per lane (up to 32
    // workgroups of 8 waves).  wave_pub = 0: the gathered form with the ghost blocks staged in LDS (also what the cycle-stamp
    // build, DIAG = 1, runs).
    const int nw_ = a.threads / 64, wsh_ = nw_ <= 1 ? 0 : 32 - __builtin_clz((unsigned)(nw_ - 1));
    const bool rg = a.batch <= 1 && a.wave_pub != 0 && !a.stamps && (a.groups > 1 || mr);
    const bool wp = rg && a.groups > 1 && nw_ * (int)(sizeof(T) / 4) <= 16 && (a.groups << wsh_) <= 256 && a.wave_pub != 3;
    // launch bound of the instantiation: shapes whose bound is above 512 threads (fp32, S <= 16: 768 threads = 168 registers per
    // lane) also exist with a bound of 512 (256 registers) for the launches that fit it - most multi-workgroup launches are 512
    // threads, and the hand-off's loop-invariant offsets do not fit 168 registers beside the matrix rows (spills)
    auto pick = [&](auto mt, auto wpm) -> PcgKernel {
        constexpr int MT = decltype(mt)::value, WPM = decltype(wpm)::value;
        if (mr) return pcg_resident_kernel<T, S, MT, 0, 0, 0, false, true, WPM, DR>;
        if (a.diag == 2) return pcg_resident_kernel<T, S, MT, 0, 2, 0, false, false, WPM, DR>;
        return pcg_resident_kernel<T, S, MT, 0, 0, 0, false, false, WPM, DR>;
    };
    auto form = [&](auto mt) -> PcgKernel {
        if constexpr (!DR) {
            if (a.stamps && !mr) return pcg_resident_kernel<T, S, MAXT0, 0, 1>;
        }
        if (wp) return pick(mt, std::integral_constant<int, 4>{});
        if (rg) return pick(mt, std::integral_constant<int, -1>{});
        return pick(mt, std::integral_constant<int, 0>{});
    };
    constexpr bool HAS512 = MAXT0 > 512 && S >= 12;
    PcgKernel kernel = form(std::integral_constant<int, MAXT0>{});
    if constexpr (HAS512) {
        if (a.threads <= 512 && a.batch <= 1) kernel = form(std::integral_constant<int, 512>{});
    }
    return pcg_launch(kernel, grid, block, a, st, a.coop);
}

}  // namespace gato
