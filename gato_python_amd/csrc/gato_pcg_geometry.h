// Compile-time launch geometry of the persistent PCG kernels per (type, STATE_SIZE): what pcg_resident_plan reports to the
// planner (gato_plan.hip) and what the launchers of gato_pcg_resident*.hip instantiate and check against.
#pragma once
#include "gato_pcg_device.h"

namespace gato {

// shape of the mixed kernel per STATE_SIZE (0 = none): waves with two rows per lane, waves in all (the others own 16-lane DPP rows,
// one knot each), k2 = knots the two-row lanes can take (LDS), npr = their Pinv columns in registers
template <int S> struct MixedCfg { static constexpr int w2 = 0, wt = 0, k2 = 0, npr = 0; };
template <> struct MixedCfg<14> { [[maybe_unused]] static constexpr int w2 = 4, wt = 8, k2 = 34, npr = 1; };   // 34 + 4 x 4 = 50 knots
template <int S> constexpr int mixed_rows()
{
    if (MixedCfg<S>::wt <= 0) return 0;
    return (MixedCfg<S>::k2 + 4 * (MixedCfg<S>::wt - MixedCfg<S>::w2)) * S;
}

template <int S> struct PairThreads { static constexpr int v = 4 * S - 2 > 64 ? 0 : (12 * S + 3 * S + 48) <= 256 ? 512 : ((12 * S + 3 * S + 48) <= 512 ? 256 : 0); };   // (private windows: one halo row per lane)
template <> struct PairThreads<14> { static constexpr int v = 512; };     // measured: 248 VGPRs, no spill at the 256 cap

// Generic rule for shapes added at build time: VGPRs per lane ~ matrix rows (6S words, x2 for fp64) + the
// operand window the compiler keeps in flight (3S words) + ~40; the specialisations below are the measured ones.
template <typename T, int S> struct MaxThreads {
    static constexpr int regs = (6 * S + 3 * S) * (int)(sizeof(T) / 4) + 40;
    static constexpr int v = regs <= 128 ? 1024 : regs <= 168 ? 768 : regs <= 256 ? 512 : 256;
    static_assert(regs <= 512, "STATE_SIZE too large for the register-resident PCG");
};
// VGPR budget: 3S*2 matrix registers per lane (x2 for fp64).  launch bound -> registers per lane:
// 1024 threads -> 128, 768 -> 168, 512 -> 256, 256 -> 512 (MI355X register file: 512 per lane per SIMD).
// Chosen so that the matrix rows plus the 3S-wide operand window stay in registers without spilling.
template <> struct MaxThreads<float, 2> { static constexpr int v = 1024; };
template <> struct MaxThreads<double, 2> { static constexpr int v = 1024; };
template <> struct MaxThreads<float, 14> { static constexpr int v = 768; };
template <> struct MaxThreads<double, 14> { static constexpr int v = 512; };
template <> struct MaxThreads<float, 32> { static constexpr int v = 512; };
template <> struct MaxThreads<double, 32> { static constexpr int v = 256; };

// Semi-resident variant (XR extra rows per lane): workgroup size with room for the extra rows' registers.
// Semi-resident variant: workgroup size by register need (resident rows 6S words + one streamed row 3S + ~80; two waves
// per SIMD when that fits 256 registers, else one), and extra rows per lane (their four state vectors take 64 KB of LDS).
template <typename T, int S> struct SemiThreads {
    static constexpr int need = 9 * S * (int)(sizeof(T) / 4) + 80;
    static constexpr int t = need <= 256 ? 512 : (need <= 512 ? 256 : 0);
    static constexpr int v = (t > 0 && MaxThreads<T, S>::v >= t && t >= 2 * S) ? t : 0;
};
template <typename T, int S> struct SemiRows {       // by LDS: two operand windows over all local knots + lambda and product of the extra rows
    static constexpr int t = SemiThreads<T, S>::v;
    static constexpr int maxk = (t + S - 1) / S, sp = pad_to(S, VecOf<T>::W), w = (int)sizeof(T);
    static constexpr int per_row = 2 * maxk * sp * w + 2 * t * w;
    static constexpr int fit = t > 0 ? (148 * 1024 - 2 * (maxk + 2) * sp * w) / per_row : 0;
    static constexpr int v = fit > 32 ? 32 : fit;
};

// No-resident-rows variant (NR): workgroup size by the registers one streamed row needs, rows per lane by LDS.
template <typename T, int S> struct NoresThreads {
    static constexpr int need = 4 * S * (int)(sizeof(T) / 4) + 70;
    static constexpr int v = 2 * S > 64 ? 0 : (need <= 120 ? 1024 : need <= 160 ? 768 : need <= 250 ? 512 : 256);
};
template <typename T, int S> struct NoresRows {
    static constexpr int t = NoresThreads<T, S>::v;
    static constexpr int maxk = t > 0 ? (t + S - 1) / S : 1, sp = pad_to(S, VecOf<T>::W), w = (int)sizeof(T);
    static constexpr int per_row = 2 * maxk * sp * w + 2 * t * w;
    static constexpr int fit = t > 0 ? (148 * 1024 - 4 * sp * w) / per_row : 0;
    static constexpr int v = fit > 32 ? 32 : fit;
};

// Single-workgroup variants with part of the Pinv rows in LDS: (threads, NL).
template <typename T, int S> struct SingleCu { static constexpr int threads = 0, nl = 0; };
template <> struct SingleCu<double, 14> { static constexpr int threads = 704, nl = 24; };   // IIWA 14/7/50 fp64

}  // namespace gato
