// Launch planning of the persistent PCG kernels: pure functions of the solver's options and the question asked.
#include "gato_solver.h"

// Geometry of a plain launch in the DPP-row layout (L lanes per knot); 0 if K does not fit max_wg such workgroups.
static int plan_dpp_rows(const gato_solver *s, int K, int L, int max_wg, int *groups, int *threads, int *kpw)
{
    const int maxT = s->plan.max_threads;
    int t = s->pcg_threads, g = s->pcg_groups;
    if (t > 0) {
        t = (t + 63) / 64 * 64;
        if (t > maxT) t = maxT;
        if (t < 64) t = 64;
    }
    if (g > 0 && t == 0) {
        const int k_per = (K + g - 1) / g;
        t = (k_per * L + 63) / 64 * 64;
        if (t > maxT) return 0;
    }
    if (t == 0) {
        if (K * L <= maxT) t = (K * L + 63) / 64 * 64;
        else {
            t = maxT < 512 ? maxT : 512;
            while (t < maxT && (K + (t / L) - 1) / (t / L) > max_wg) t += 64;
            if ((K + (t / L) - 1) / (t / L) > 32 && (K + (maxT / L) - 1) / (maxT / L) <= 32) {      // one XCD if larger workgroups get there
                while (t < maxT && (K + (t / L) - 1) / (t / L) > 32) t += 64;
            }
        }
    }
    const int k_per_max = t / L;
    if (k_per_max < 1) return 0;
    int W = (K + k_per_max - 1) / k_per_max;
    if (g > 0 && g >= W) W = g;
    if (W > max_wg) return 0;
    const int k_per = (K + W - 1) / W;
    W = (K + k_per - 1) / k_per;
    *groups = W; *threads = t; *kpw = k_per;
    return 1;
}

// Geometry of the resident launch.  One workgroup per CU at most (all workgroups must be
// co-resident: they hand partial dots and halo blocks to each other inside the launch).
bool plan_resident(const gato_solver &solver, const PcgOpts &o, int K, int batch, bool plain_only, PcgGeometry *geo)
{
    const gato_solver *s = &solver;
    *geo = PcgGeometry{};
    int *groups = &geo->groups, *threads = &geo->threads, *kpw = &geo->kpw;
    const bool no_pair = s->no_pair || plain_only, no_single_lds = s->no_single_lds || plain_only;
    const int S = s->d.S;
    int max_wg = s->num_cus < 256 ? s->num_cus : 256;
    if (s->max_workgroups > 0 && s->max_workgroups < max_wg) max_wg = s->max_workgroups;   // CUs this solver may count on
    int t = s->pcg_threads;
    int g = s->pcg_groups;
    const int maxT = s->plan.max_threads;
    // DPP-row layout of the plain / cluster launches (option dpp_rows: -1 auto, 0 never, 1 wherever such a launch fits): auto
    // leaves the one-workgroup special kernels (two rows per lane) and one-workgroup-per-system batches alone
    if (s->plan.dpp_lanes > 0 && s->dpp_rows != 0 && o.stamp != 1) {
        const int L = s->plan.dpp_lanes;
        const bool one_wg_kernel = t == 0 && g <= 1 &&
            ((!no_pair && s->plan.pair_threads > 0 && K * (S / 2) <= s->plan.pair_threads) ||
             (!no_pair && !no_single_lds && s->plan.mixed_rows > 0 && K * S <= s->plan.mixed_rows && K * L > maxT && !s->cl.on && K == s->d.K) ||
             (K * S > maxT && K * S <= s->plan.single_max_threads && !no_single_lds));
        const bool batch_split = batch > 1 && K * L > maxT && K * S <= maxT;          // a batch needs one workgroup per system
        // measured (tools/dpp_ab.py, same box, with the lean hand-off): fp64 14/7/512 2.76 -> 2.56 us per iteration, 14/7/1024
        // 2.94 -> 2.75, 32/16/1024 6.35 -> 5.10, one workgroup 14/7/20 1.71 -> 1.35 (14/7/4096 and 12/6/300 equal); fp32 keeps
        // the LDS windows with packed FMAs: 14/7/512 2.17 against 2.21, 32/16/256 2.53 against 2.78 (the DPP-row kernel spills
        // there), 32/16/1024 3.73 against 3.70, 12/6/300 1.86 against 2.13 (idle lanes cost workgroups)
        // (cluster launches still run the older hand-off, where the LDS-window kernel at S = 32 is the slower one: one-GPU
        //  rehearsal of 32/16/1024 f32 over 2 ranks 4.62 us per iteration with DPP rows, 4.9 without)
        const bool pays = s->esz == 8 || (S > 16 && s->cl.on);
        if ((s->dpp_rows > 0 || (pays && !one_wg_kernel && !batch_split)) && plan_dpp_rows(s, K, L, max_wg, groups, threads, kpw)) {
            geo->dpp = 1;
            return 1;
        }
    }
    if (t > 0) {
        t = (t + 63) / 64 * 64;
        if (t > maxT) t = maxT;
        if (t < 64) t = 64;
    }
    if (g > 0 && t == 0) {
        int k_per = (K + g - 1) / g;
        t = (k_per * S + 63) / 64 * 64;
        if (t < 64) t = 64;
        if (t > maxT) return 0;
    }
    if (t == 0 && g <= 1 && !no_pair && s->plan.pair_threads > 0 && K * (S / 2) <= s->plan.pair_threads) {
        // fp32: one workgroup, two rows per lane (packed FMAs, half the waves)
        *groups = 1; *threads = (K * (S / 2) + 63) / 64 * 64; *kpw = K;
        geo->pair = 1;
        return 1;
    }
    // (from the size at which the one-row-per-lane launch no longer fits ONE workgroup: K S > maxT, or - where the DPP-row layout
    //  would be taken, 16 lanes per knot - K 16 > maxT: 14/7/33..36 fp64 ran as two workgroups at 2.22 us per iteration)
    const int one_row_lanes = (s->plan.dpp_lanes > 0 && s->dpp_rows != 0 && s->esz == 8) ? s->plan.dpp_lanes : S;
    if (t == 0 && g <= 1 && !no_pair && !no_single_lds && s->plan.mixed_rows > 0 && K * S <= s->plan.mixed_rows && K * one_row_lanes > maxT &&
        o.stamp != 1 && !s->cl.on && K == s->d.K) {
        // fp64 beyond the register-resident single workgroup: one workgroup, two rows per lane in part of the waves
        *groups = 1; *threads = s->plan.mixed_threads; *kpw = K;
        geo->pair = 2;
        return 1;
    }
    if (t == 0) {
        // auto: one workgroup while the problem fits one CU's registers (no inter-CU traffic at all);
        // otherwise 512-thread workgroups (measured best on MI355X: 2 waves per SIMD hide the LDS latency
        // of the operand window, and W stays small enough that one wave sweeps all partial granules),
        // growing only if that would need more workgroups than CUs.
        if (K * S <= maxT) t = (K * S + 63) / 64 * 64;
        else if (K * S <= s->plan.single_max_threads && g <= 1 && !no_single_lds) {
            *groups = 1; *threads = (K * S + 63) / 64 * 64; *kpw = K;      // one CU, Pinv rows partly in LDS
            return 1;
        }
        else {
            t = maxT < 512 ? maxT : 512;
            while (t < maxT && (long long)((K + (t / S) - 1) / (t / S)) > max_wg) t += 64;
            // up to 32 workgroups fit one XCD (cheaper hand-offs): take larger workgroups if that gets there
            if ((K + (t / S) - 1) / (t / S) > 32 && (K + (maxT / S) - 1) / (maxT / S) <= 32) {
                while (t < maxT && (K + (t / S) - 1) / (t / S) > 32) t += 64;
            }
        }
        if (t < 64) t = 64;
    }
    int k_per_max = t / S;
    if (k_per_max < 1) return 0;
    int W = (K + k_per_max - 1) / k_per_max;
    if (g > 0 && g >= W) W = g;
    if (W > max_wg) {
        // beyond the register file: one workgroup per CU, the knots a workgroup has no lanes for become extra rows whose
        // matrix entries are re-read from memory every product (option pcg_semi: -1 auto, 0 never)
        // option pcg_semi: -1 auto, 0 never (streaming kernels), 1 semi-resident, 2 no resident rows
        if (s->pcg_semi == 0 || s->pcg_threads > 0 || s->pcg_groups > 0) return 0;
        const int kp = (K + max_wg - 1) / max_wg;
        const int Wx = (K + kp - 1) / kp;
        if (Wx < 2) return 0;
        const int xt = s->plan.semi_threads, nt = s->plan.nores_threads;
        const bool semi_ok = xt > 0 && (long long)(kp - xt / S) * S <= (long long)s->plan.semi_rows * xt;
        const bool nores_ok = nt > 0 && (long long)kp * S <= (long long)s->plan.nores_rows * nt;
        // the LDS-DMA ring (option pcg_semi = 3; auto: once the bytes of S and Pinv that ONE launch streams per product are well past
        // the 256 MB Infinity Cache, i.e. the re-read block rows come from HBM; below that the semi-resident launch is served by the
        // caches and wins).  Measured cross-overs against the semi-resident launch (tools/ring_crossover.py, profiles/r05_ring_crossover.log):
        // 14/7 f32 K ~ 90 000 (420 MB), 32/16 f32 K ~ 28 000 (690 MB: its semi-resident launch already reads at 6 TB/s), 14/7 f64
        // between K = 49 152 (462 MB: semi 79.6 / ring 82.9 us per iteration) and K = 65 536 (617 MB: 107.7 / 104.6; driver sweep of
        // round 4: 107.9 / 97.3) - the fp64 ring serves up to 256 knots per workgroup, so auto takes it from 550 MB up to K = 65 536.
        // (K = the knots of THIS launch: a rank's shard in a cluster - what matters is what one GPU streams per product.  A cluster
        //  judges by the LARGEST shard, ceil(K_system / ranks), on every rank: shards differ by a knot and neighbouring ranks must
        //  not land on different sides of the threshold.)
        const bool dma_ok = !o.warm && s->ops->pcg_dma_max_knots() > 0 && kp <= s->ops->pcg_dma_max_knots();
        const double K_rule = s->cl.on && s->cl.nranks > 0 ? (double)((s->d.K + s->cl.nranks - 1) / s->cl.nranks) : (double)K;
        const double ring_from = S > 16 ? 700e6 : (s->esz == 8 ? 550e6 : 450e6);
        const bool beyond_cache = 2.0 * 3.0 * S * S * K_rule * (double)s->esz > ring_from;
        int which = 0;
        if (s->pcg_semi == 1) which = semi_ok ? 1 : 0;
        else if (s->pcg_semi == 2) which = nores_ok ? 2 : 0;
        else if (s->pcg_semi == 3) which = dma_ok ? 3 : 0;
        else which = (dma_ok && beyond_cache) ? 3 : semi_ok ? 1 : (nores_ok ? 2 : 0);
        if (!which) return 0;
        *groups = Wx; *threads = which == 1 ? xt : which == 2 ? nt : 512; *kpw = kp;
        geo->semi = which;
        return 1;
    }
    int k_per = (K + W - 1) / W;                     // balanced
    W = (K + k_per - 1) / k_per;
    *groups = W; *threads = t; *kpw = k_per;
    return 1;
}

// Geometry of the single-reduction variant: a workgroup's lanes cover its own knots plus one ghost-lane knot per side.
bool plan_cg1(const gato_solver &solver, int K, PcgGeometry *geo)
{
    const gato_solver *s = &solver;
    *geo = PcgGeometry{};
    int *groups = &geo->groups, *threads = &geo->threads, *kpw = &geo->kpw;
    const int S = s->d.S;
    int max_wg = s->num_cus < 256 ? s->num_cus : 256;
    if (s->max_workgroups > 0 && s->max_workgroups < max_wg) max_wg = s->max_workgroups;   // CUs this solver may count on
    const int maxT = s->ops->pcg_cg1_max_threads();
    int t = s->pcg_threads > 0 ? (s->pcg_threads + 63) / 64 * 64 : 0;
    if (t > maxT) t = maxT;
    if (t == 0) {
        if ((K + 2) * S <= maxT) t = ((K + 2) * S + 63) / 64 * 64;
        else {
            t = maxT < 512 ? maxT : 512;
            while (t < maxT && (K + (t / S - 2) - 1) / (t / S - 2) > max_wg) t += 64;
        }
    }
    if (t < 4 * S) t = (4 * S + 63) / 64 * 64;
    if (t > maxT) return 0;
    const int per = t / S - 2;
    if (per < 2) return 0;
    int W = (K + per - 1) / per;
    if (s->pcg_groups > W) W = s->pcg_groups;
    if (W > max_wg) return 0;
    int k_per = (K + W - 1) / W;
    W = (K + k_per - 1) / k_per;
    // every workgroup needs two knots of its own (its two edge blocks on either side go to the neighbours).  When the even split
    // leaves the last workgroup ONE knot, the launcher takes the balanced split instead (sizes k_per and k_per - 1: launch_pcg_cg1)
    if (W > 1 && (k_per < 2 || (K - (W - 1) * k_per < 2 && k_per < 3))) return 0;
    *groups = W; *threads = t; *kpw = k_per;
    geo->cg1 = true;
    return 1;
}

// Do n systems (or right-hand sides) run as ONE launch of one-workgroup solves, a workgroup each?  (Planned as a batch of n is.)
bool plan_one_wg_each(const gato_solver &s, const PcgOpts &o, int n)
{
    PcgGeometry g;
    return n > 1 && o.mode != GATO_PCG_STREAMING && plan_resident(s, o, s.d.K, n, false, &g) && g.groups == 1;
}

// Geometry a cluster launch of `rank` would use (false: the rank's knots do not fit a persistent launch).
bool cluster_plan(const gato_solver &s, const PcgOpts &o, int rank, PcgGeometry *geo)
{
    // geometry over that rank's knots; the one-workgroup special kernels have no cross-GPU level
    int k0 = 0, k1 = 0;
    gato_cluster_knot_range(s.d.K, rank, s.cl.nranks, &k0, &k1);
    return plan_resident(s, o, k1 - k0, s.d.B, true, geo);
}

// Flat exchange: the whole cluster has at most 256 workgroups and every rank runs the plain resident variant.  Every rank derives
// every rank's geometry from the same rule (same device type, same options on all ranks); base = workgroups of the ranks before this one.
bool cluster_plan_flat(const gato_solver &s, const PcgOpts &o, int *flat_total, int *flat_base)
{
    int total = 0, base = 0;
    for (int r = 0; r < s.cl.nranks; ++r) {
        PcgGeometry g;
        if (!cluster_plan(s, o, r, &g) || g.semi) return false;
        if (r < s.cl.rank) base += g.groups;
        total += g.groups;
    }
    *flat_total = total; *flat_base = base;
    return total <= 256;
}

// Single-reduction recurrence in a cluster (option pcg_variant = 1): EVERY rank must be able to run it - its knots fit one launch
// of pcg_cg1_kernel<..., MR> and every workgroup of the cluster owns at least two knots (the exchange carries the first / last two
// blocks of w) - or every rank takes the default recurrence: each rank derives every rank's geometry from the same rule (same
// device type and options on all ranks, as for the flat exchange).  1 = variant 1 runs; geometry of THIS rank, and the flat
// exchange's numbering (total <= 256 workgroups) if it applies.
bool cluster_plan_cg1(const gato_solver &solver, const PcgOpts &o, PcgGeometry *geo, int *flat_total, int *flat_base)
{
    const gato_solver *s = &solver;
    if (s->pcg_variant != 1 || o.warm || o.mode == GATO_PCG_STREAMING) return false;
    int total = 0, base = 0;
    for (int r = 0; r < s->cl.nranks; ++r) {
        int k0 = 0, k1 = 0;
        PcgGeometry g;
        gato_cluster_knot_range(s->d.K, r, s->cl.nranks, &k0, &k1);
        const int Kr = k1 - k0;
        if (!plan_cg1(solver, Kr, &g)) return false;
        if (s->cl.nranks > 1 && (g.kpw < 2 || Kr - (g.groups - 1) * g.kpw < 2)) return false;
        if (r < s->cl.rank) base += g.groups;
        if (r == s->cl.rank) *geo = g;
        total += g.groups;
    }
    *flat_total = total; *flat_base = base;
    return true;
}

