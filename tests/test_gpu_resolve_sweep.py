"""The re-solve (gato_solve_rhs: rhs_gamma_kernel, the `rhs` argument of every PCG kernel and of dz_kernel) at every route,
shape and batch its first tests left out.  Every case is named and deterministic (tests/resolve_sweep_ref.py; the CPU side -
the two oracles agree on every case, two systems of a case are far apart - is tests/test_sweep_refs_cpu.py).

a. B >= 2 systems x R >= 2 right-hand sides through every one-workgroup PCG kernel: the shared-matrix index msys = sys / rhs is
   written out in each of them, and a wrong one shows only when B > 1, R > 1 and the matrices differ.  The route that ran is
   asserted from the solver's own report, so a case that lands on another kernel fails.
b. The launch-by-launch branch (several workgroups per system, streaming kernels) with B > 1: its pointers Sbd + b bd.
c. rhs_gamma_kernel alone against the oracle's gamma: every shape, K = 1, 2, 3, 9, S R on both sides of its 64 lanes, two
   systems, and the second grid pass (K > 8192).
d. True warm start with a lambda0 per (b, r).
Bars: those of tests/test_gpu_resolve.py - check_solve (fp64: the oracle's iteration count and 1e-8; fp32: check_f32), gamma
1e-12 relative in fp64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_polish_ref as P                      # noqa: E402
import resolve_sweep_ref as R                      # noqa: E402
from f32_parity import check_f32                   # noqa: E402
from gato_python_amd import _lib, synth            # noqa: E402
from oracle import gato_oracle as o                # noqa: E402
from test_gpu_parity import check_solve, host, rel   # noqa: E402
from test_gpu_resolve import new_rhs, rhs_dev, solver, tol_mi   # noqa: E402

CAP = 8192                                         # launch_rhs_gamma: workgroups in x; knots >= CAP run in a second pass


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def names(cases):
    return [c.name for c in cases]


def whole_solve(sol, systems, tol, mi):
    """linsys_batched of the B systems: the assembly every re-solve below reads."""
    B, sk = len(systems), systems[0].S * systems[0].K
    lam, dz, iters = sol.new(B * sk).zero_(), sol.new(B * sol.N), sol.new(B, torch.int32)     # (lambda = 0: a warm solver reads it)
    sol.linsys_batched(*sol.upload_batch(systems), tol, mi, systems[0].rho, lam, dz, iters)
    torch.cuda.synchronize()
    sol.check_status()


def run_case(case, iters=None, **more):
    """-> (flat right-hand sides [B R], lambda [B R, S K], dz [B R, N], iterations [B R], the solver's last_* report)."""
    systems, rs = case.inputs()
    flat = [s2 for per in rs for s2 in per]
    sol = solver(case.S, case.C, case.K, case.dt, batch=case.B, **dict(case.opts, **more))
    whole_solve(sol, systems, case.tol, case.mi)
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, flat), case.tol, case.mi, iters=iters)
    torch.cuda.synchronize()
    sol.check_status()
    report = {k: sol.get_option(k) for k in ("last_mode", "last_groups", "last_threads", "last_pair", "last_dpp", "last_variant",
                                             "last_dz_fused")}
    sol.close()
    n = case.B * case.R
    return flat, host(lam).reshape(n, -1), host(dz).reshape(n, -1), host(it), report


def check_case(case, flat, lam, dz, it, what=""):
    for i, s2 in enumerate(flat):
        check_solve(f"{case.name}{what} system {i // case.R} rhs {i % case.R}", s2, case.S, case.C, case.K, case.dt, case.tol,
                    case.mi, lam[i], dz[i], int(it[i]))


def check_route(case, report):
    print(case.name, report)
    for k, v in case.route.items():
        assert report[k] == v, (case.name, k, report)


# ---- a. every one-workgroup route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ROUTES, ids=names(R.ROUTES))
def test_batch_times_rhs_through_every_one_workgroup_route(case):
    flat, lam, dz, it, report = run_case(case)
    check_route(case, report)
    if case.name.startswith("single-cu"):
        assert report["last_threads"] > 512, report            # beyond the register-resident workgroup: Pinv rows partly in LDS
    assert report["last_dz_fused"] == (0 if case.cg1 else 1)  # one workgroup per right-hand side: dz rides in its epilogue
    check_case(case, flat, lam, dz, it)


@pytest.mark.parametrize("name", R.DZ_LAUNCH, ids=R.DZ_LAUNCH)
def test_batch_times_rhs_with_dz_as_its_own_launch(name):
    """no_fuse_dz = 1: dz_kernel over all B R right-hand sides (its own msys) instead of the PCG launch's epilogue.  Both held
    to check_solve; the same bits where the whole-solve tests promise them (the fp32 two-row kernel:
    test_dz_in_the_fp32_two_row_epilogue_of_a_batch_is_bit_identical_to_the_dz_launch)."""
    case = R.BY_NAME[name]
    flat, lam0, dz0, it0, rep0 = run_case(case)
    _, lam1, dz1, it1, rep1 = run_case(case, no_fuse_dz=1)
    check_route(case, rep0)
    check_route(case, rep1)
    assert rep0["last_dz_fused"] == 1 and rep1["last_dz_fused"] == 0
    check_case(case, flat, lam1, dz1, it1, " dz launch")
    check_case(case, flat, lam0, dz0, it0, " dz epilogue")
    assert np.array_equal(lam0, lam1) and np.array_equal(it0, it1)      # the PCG itself is the same launch
    same = np.array_equal(dz0, dz1)
    print(name, "dz of the epilogue and of the launch: same bits", same)
    if name.startswith("pair-f32"):
        assert same


# ---- b. launch by launch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LAUNCHES, ids=names(R.LAUNCHES))
def test_batch_times_rhs_launch_by_launch(case):
    n = case.B * case.R
    own = torch.full((n,), -7, dtype=torch.int32, device="cuda:0") if case.name == "multi-wg-f32-14-7-512" else None
    flat, lam, dz, it, report = run_case(case, iters=own)
    check_route(case, report)
    assert report["last_dz_fused"] == 0
    if case.name.startswith("multi-wg"):
        assert report["last_groups"] > 1, report
    if own is not None:                                           # the caller's tensor took all four counts
        assert it.tolist() == host(own).tolist() and (host(own) >= 0).all()
    check_case(case, flat, lam, dz, it)


# ---- c. rhs_gamma_kernel -------------------------------------------------------------------------------------------------------------
def r_past_the_wave(S):
    return 64 // S + 1                                            # S R > 64: the lane loop of the kernel takes a second trip


GAMMA_CASES = [(S, C, K, Rn, np.float64) for S, C in P.SWEEP_SHAPES for K in (1, 2, 3, 9) for Rn in (1, r_past_the_wave(S))] + \
              [(S, C, 9, Rn, np.float32) for S, C in P.SWEEP_SHAPES for Rn in (1, r_past_the_wave(S))]


def gamma_case(S, C, K, Rn, dt, B, seed=3, mi=None):
    """-> (right-hand sides [B R], gamma of the re-solve [B R, S K])."""
    make = lambda sd: synth.make_system(S, C, K, seed=sd) if K > 1 else synth.blocks_to_csr(*synth.make_blocks(S, C, 1, sd, False))
    systems = [make(seed + b) for b in range(B)]
    flat = [new_rhs(systems[b], 70 + 40 * b + r) for b in range(B) for r in range(Rn)]
    tol, mi_ = tol_mi(dt)
    sol = solver(S, C, K, dt, batch=B)
    whole_solve(sol, systems, tol, mi or mi_)
    sol.solve_rhs(*rhs_dev(sol, flat), tol, mi or mi_)
    torch.cuda.synchronize()
    sol.check_status()
    gam = sol.read_rhs_gamma(Rn).reshape(B * Rn, S * K)
    sol.close()
    return flat, gam


def oracle_gamma(s2, dt, rounded=False):
    """gamma of the numpy oracle's whole solve (one PCG iteration: gamma is formed in front of it)."""
    if rounded:
        s2, rho = s2.astype(np.float32).astype(np.float64), float(np.float32(s2.rho))
    else:
        rho = s2.rho
    return o.linsys_solve(*s2.csr_args(), s2.S, s2.C, s2.K, 1e-10, 1, rho, dtype=dt, return_all=True)["gamma"]


@pytest.mark.parametrize("S,C,K,Rn,dt", GAMMA_CASES, ids=["%d-%d-%d-R%d-%s" % (S, C, K, Rn, np.dtype(dt).name) for S, C, K, Rn, dt in GAMMA_CASES])
def test_gamma_of_the_resolve_every_shape(S, C, K, Rn, dt):
    """fp64: 1e-12 relative per (b, r).  fp32 (K = 9): the fp32 oracle's gamma beside the fp64 oracle's gamma of the fp32-rounded
    inputs (check_f32)."""
    B = 2
    assert (S * Rn > 64) == (Rn > 1)
    flat, gam = gamma_case(S, C, K, Rn, dt, B)
    for i, s2 in enumerate(flat):
        want = oracle_gamma(s2, dt)
        assert np.any(want != 0)
        if dt == np.float64:
            assert rel(gam[i], want) < 1e-12, (i // Rn, i % Rn, rel(gam[i], want))
        else:
            check_f32(f"re-solve gamma {S}/{C}/{K} system {i // Rn} rhs {i % Rn}", gam[i], want, oracle_gamma(s2, np.float64, rounded=True))


def test_gamma_of_the_resolve_second_grid_pass():
    """2/1/8197, R = 2: the whole vector, and the knots >= 8192 of the second pass alone."""
    S, C, K = P.SWEEP_LONG
    flat, gam = gamma_case(S, C, K, 2, np.float64, 1, mi=20)
    for i, s2 in enumerate(flat):
        want = oracle_gamma(s2, np.float64)
        tail = slice(CAP * S, None)
        assert len(want[tail]) == (K - CAP) * S and np.all(want[tail] != 0)
        assert rel(gam[i], want) < 1e-12 and rel(gam[i][tail], want[tail]) < 1e-12, (i, rel(gam[i], want), rel(gam[i][tail], want[tail]))


# ---- d. true warm start, a lambda0 per (b, r) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.WARM, ids=names(R.WARM))
def test_true_warm_start_per_system_and_rhs(case):
    """As test_gpu_resolve.py::test_true_warm_start per (b, r): the numpy oracle's PCG from the same lambda0 on the oracle's
    matrices - fp64 the same iteration count and 1e-8 (dz from that lambda as well); fp32 within two iterations and check_f32
    against the fp64 warm PCG of the fp32-rounded inputs run to 1e-14."""
    S, C, K, dt = case.S, case.C, case.K, case.dt
    f64 = dt == np.float64
    systems, rs = case.inputs()
    flat = [s2 for per in rs for s2 in per]
    refs, guesses = [], []
    for i, s2 in enumerate(flat):
        ref = o.linsys_solve(*s2.csr_args(), S, C, K, case.tol, case.mi, s2.rho, dtype=dt, return_all=True)
        refs.append(ref)
        guesses.append(R.warm_guess(ref["lam"].astype(np.float64), i).astype(dt))
    sol = solver(S, C, K, dt, batch=case.B, **case.opts)
    whole_solve(sol, systems, case.tol, case.mi)
    lam = sol.to_device(np.concatenate(guesses))
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, flat), case.tol, case.mi, lam=lam)
    torch.cuda.synchronize()
    sol.check_status()
    assert sol.get_option("last_groups") == 1 and sol.get_option("last_mode") == 1
    lam, dz, it = host(lam).reshape(len(flat), -1), host(dz).reshape(len(flat), -1), host(it)
    sol.close()
    for i, (s2, ref, lam0) in enumerate(zip(flat, refs, guesses)):
        lam_o, it_o = o.pcg(ref["S"], ref["Pinv"], ref["gamma"], S, K, case.tol, case.mi, lam0=lam0)
        dz_o = o.compute_dz(ref["Ginv"], ref["C_dense"], np.asarray(s2.g, dt), lam_o, S, C, K)
        cold = ref["iters"]
        print(case.name, i, "iterations", int(it[i]), "oracle warm", it_o, "oracle cold", cold)
        assert it_o < cold                                         # the guess is worth something: a kernel that ignored it shows
        if f64:
            assert int(it[i]) == it_o, (i, int(it[i]), it_o)
            assert rel(lam[i], lam_o) < 1e-8 and rel(dz[i], dz_o) < 1e-8, (i, rel(lam[i], lam_o), rel(dz[i], dz_o))
        else:
            assert abs(int(it[i]) - it_o) <= 2, (i, int(it[i]), it_o)
            s64 = s2.astype(np.float32).astype(np.float64)
            t = o.linsys_solve(*s64.csr_args(), S, C, K, 1e-14, 600, float(np.float32(s2.rho)), dtype=np.float64, return_all=True)
            lam_t, _ = o.pcg(t["S"], t["Pinv"], t["gamma"], S, K, 1e-14, 600, lam0=lam0.astype(np.float64))
            dz_t = o.compute_dz(t["Ginv"], t["C_dense"], s64.g, lam_t, S, C, K)
            check_f32(f"{case.name} lambda {i}", lam[i], lam_o, lam_t)
            check_f32(f"{case.name} dz {i}", dz[i], dz_o, dz_t)
