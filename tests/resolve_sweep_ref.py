"""The named cases of the re-solve sweep (tests/test_gpu_resolve_sweep.py) and their inputs, shared with the CPU checks of
tests/test_sweep_refs_cpu.py.

A case is B systems of different seeds and R right-hand sides per system, every (b, r) with its own (g, c).  Its seed is the
first of ten at which the reference can carry the comparison check_solve makes (the oracle's exact iteration count in fp64):
for every (b, r) the C oracle and the numpy oracle stop at the same iteration and agree to 1e-9 in lambda and dz - for the
single-reduction cases the numpy restatement of that recurrence as well.  An fp32 case must also be one fp32 can carry: the fp32
C oracle, the fp32 numpy oracle and the fp64 oracle on the fp32-rounded inputs stop at the same iteration.  (Where the fp32
recurrence runs on past the fp64 one it iterates on rounding noise - 4/2/9 is 36 unknowns - and the iterate it is stopped at
depends on the summation order: tools/past_convergence.py, f32_parity.check_f32.  At seed 0 of 4/2/9 two right-hand sides take 18
iterations in fp32 and 16 in fp64; the GPU, whole solve and re-solve alike, stops them at 17.)  carries() is that rule; the
seeds below are its results, and test_sweep_refs_cpu.py holds every recorded seed to it."""
import numpy as np

from gato_python_amd import synth
from oracle import c_oracle as co
from oracle import gato_oracle as o
from test_gpu_resolve import new_rhs, tol_mi      # (helpers only: that module's tests need a GPU, these do not)

F64, F32 = np.float64, np.float32
AGREE = 1e-9             # the two oracles, in lambda and dz
DISTINCT = 1e-3          # the solutions of two systems of a case on the same (g, c) differ by more than this (relative)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def with_rhs(s, other):
    """The matrices of s with the (g, c) of `other`."""
    return synth.KKTSystem(s.S, s.C, s.K, s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, other.g, other.c, s.rho)


class Case:
    def __init__(self, name, S, C, K, dt, B, R, seed, opts=None, route=None, tol=None, mi=None):
        self.name, self.S, self.C, self.K, self.dt, self.B, self.R, self.seed = name, S, C, K, dt, B, R, seed
        self.opts, self.route = dict(opts or {}), dict(route or {})
        self.tol, self.mi = tol_mi(dt) if tol is None else (tol, mi)

    def inputs(self, seed=None):
        """-> (systems [B], right-hand sides [B][R] as systems with the matrices of b)."""
        seed = self.seed if seed is None else seed
        systems = [synth.make_system(self.S, self.C, self.K, seed=100 * seed + b) for b in range(self.B)]
        return systems, [[new_rhs(systems[b], 10000 * seed + 10 * b + r) for r in range(self.R)] for b in range(self.B)]

    @property
    def cg1(self):
        return self.opts.get("pcg_variant") == 1


def carries(case, seed):
    """The rule of the module docstring at one seed -> (ok, [(b, r, iterations C, iterations numpy, rel lambda, rel dz)])."""
    S, C, K = case.S, case.C, case.K
    tol, mi = (case.tol, case.mi) if np.dtype(case.dt) == np.float64 else tol_mi(F64)
    ok, rows = True, []
    for b, per in enumerate(case.inputs(seed)[1]):
        for r, s2 in enumerate(per):
            lam_c, dz_c, it_c = co.linsys_solve(*s2.csr_args(), S, C, K, tol, mi, s2.rho, dtype=F64)
            n = o.linsys_solve(*s2.csr_args(), S, C, K, tol, mi, s2.rho, dtype=F64, return_all=True)
            row = (b, r, it_c, n["iters"], rel(n["lam"], lam_c), rel(n["dz"], dz_c))
            good = it_c == n["iters"] and it_c < mi and row[4] <= AGREE and row[5] <= AGREE
            if case.cg1:
                lam_1, it_1 = o.pcg_single_reduction(n["S"], n["Pinv"], n["gamma"], S, K, tol, mi)
                row += (it_1, rel(lam_1, lam_c))
                good = good and it_1 == it_c and row[7] <= AGREE
            if np.dtype(case.dt) == np.float32:
                # fp32 cases also in fp32: both CPU orders and the fp64 recurrence on the fp32-rounded inputs stop at the same iteration
                t32, m32 = case.tol, case.mi
                s64, rho32 = s2.astype(F32).astype(F64), float(F32(s2.rho))
                its = (co.linsys_solve(*s2.csr_args(), S, C, K, t32, m32, s2.rho, dtype=F32)[2],
                       o.linsys_solve(*s2.csr_args(), S, C, K, t32, m32, s2.rho, dtype=F32)[2],
                       co.linsys_solve(*s64.csr_args(), S, C, K, t32, m32, rho32, dtype=F64)[2])
                row += its
                good = good and len(set(its)) == 1 and its[0] < m32
            rows.append(row)
            ok = ok and good
    return ok, rows


def distinct(case):
    """min over (b, r) of the relative distance between the C oracle's solution of system b and that of system (b + 1) % B
    on the same (g, c): what a kernel reading the wrong system's matrices would be off by."""
    S, C, K = case.S, case.C, case.K
    systems, rs = case.inputs()
    tol, mi = tol_mi(F64)
    worst = np.inf
    for b in range(case.B):
        for s2 in rs[b]:
            lam, dz, _ = co.linsys_solve(*s2.csr_args(), S, C, K, tol, mi, s2.rho, dtype=F64)
            other = with_rhs(systems[(b + 1) % case.B], s2)
            lam_x, dz_x, _ = co.linsys_solve(*other.csr_args(), S, C, K, tol, mi, other.rho, dtype=F64)
            worst = min(worst, rel(lam_x, lam), rel(dz_x, dz))
    return worst


ONE_WG = dict(last_mode=1, last_groups=1)
PLAIN = dict(ONE_WG, last_pair=0, last_dpp=0, last_variant=0)

# ---- A. every one-workgroup PCG route, B >= 2 and R >= 2 (routes: gato_plan.hip over gato_pcg_geometry.h) --------------------------
ROUTES = [
    # fp32, K S / 2 <= 512 lanes: two rows per lane
    Case("pair-f32-14-7-9", 14, 7, 9, F32, 2, 3, 0, route=dict(ONE_WG, last_pair=1)),
    Case("pair-f32-4-2-9", 4, 2, 9, F32, 3, 2, 1, route=dict(ONE_WG, last_pair=1)),
    # fp64 14/7, 16 K > 512 lanes and 14 K <= 700 rows: mixed rows
    Case("mixed-f64-14-7-40", 14, 7, 40, F64, 2, 3, 0, route=dict(ONE_WG, last_pair=2)),
    # fp64, S in (12, 14, 32) and K lanes-per-knot <= max threads: DPP rows
    Case("dpp-f64-14-7-20", 14, 7, 20, F64, 3, 2, 0, route=dict(ONE_WG, last_dpp=1, last_pair=0)),
    Case("dpp-f64-12-6-9", 12, 6, 9, F64, 2, 2, 0, route=dict(ONE_WG, last_dpp=1, last_pair=0)),
    Case("dpp-f64-32-16-5", 32, 16, 5, F64, 2, 3, 0, route=dict(ONE_WG, last_dpp=1, last_pair=0)),
    # fp64 without a DPP-row form (S = 2, 4, 6)
    Case("plain-f64-2-1-9", 2, 1, 9, F64, 3, 3, 0, route=PLAIN),
    Case("plain-f64-6-3-9", 6, 3, 9, F64, 2, 2, 0, route=PLAIN),
    # fp32 with the two-row kernel switched off, and at S = 32 where it does not exist
    Case("plain-f32-14-7-9-no_pair", 14, 7, 9, F32, 2, 2, 0, opts=dict(no_pair=1), route=PLAIN),
    Case("plain-f32-32-16-7", 32, 16, 7, F32, 2, 2, 0, route=PLAIN),
    # fp64 14/7, 512 < 14 K <= 704 with the mixed-rows kernel switched off: one CU, Pinv rows partly in LDS
    Case("single-cu-f64-14-7-45", 14, 7, 45, F64, 2, 2, 0, opts=dict(no_pair=1), route=dict(ONE_WG, last_pair=0, last_dpp=0)),
    # the single-reduction kernel (pcg_variant = 1): one workgroup holds K + 2 knots of lanes - fp64 14/7 has 256, so K <= 16
    Case("cg1-f64-14-7-16", 14, 7, 16, F64, 2, 3, 0, opts=dict(pcg_variant=1), route=dict(ONE_WG, last_variant=1)),
    Case("cg1-f32-14-7-9", 14, 7, 9, F32, 3, 2, 0, opts=dict(pcg_variant=1), route=dict(ONE_WG, last_variant=1)),
]
# dz as a launch of its own (no_fuse_dz = 1) beside dz in the PCG launch's epilogue: the three epilogues
DZ_LAUNCH = ["pair-f32-14-7-9", "dpp-f64-14-7-20", "mixed-f64-14-7-40"]

# ---- B. launch by launch: several workgroups per system, or the streaming kernels ------------------------------------------------
LAUNCHES = [
    Case("multi-wg-f32-14-7-512", 14, 7, 512, F32, 2, 2, 0, route=dict(last_mode=1)),
    Case("multi-wg-f64-14-7-512", 14, 7, 512, F64, 2, 2, 0, route=dict(last_mode=1)),
    Case("streaming-f64-14-7-50", 14, 7, 50, F64, 2, 2, 0, opts=dict(pcg_mode=2), route=dict(last_mode=2)),
]

# ---- D. true warm start, lambda0 read in place as [B][R] ---------------------------------------------------------------------------
WARM = [
    Case("warm-f64-14-7-20", 14, 7, 20, F64, 2, 2, 0, opts=dict(true_warm_start=1)),
    Case("warm-f32-14-7-9", 14, 7, 9, F32, 2, 2, 0, opts=dict(true_warm_start=1)),
]

ALL = ROUTES + LAUNCHES + WARM
BY_NAME = {c.name: c for c in ALL}


def warm_guess(lam, i):
    """lambda0 of right-hand side i of a case: near its solution, another one per (b, r)."""
    return lam * (0.9 - 0.04 * i) + 0.01 * (i + 1)
