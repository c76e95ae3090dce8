"""The references, inputs, cases and bars of tests/pcg_ref.py on the CPU alone: the PCG bar holds between the two CPU orders on
every case, seed and n (the measurement its factor comes from), so do the gamma and dz bars; BlockReference equals the dense
asm_ref.Reference; the C oracle's converged fp64 solve is within a tenth of BASELINE's bar; eight mutations of a numpy
restatement - stand-ins for a subtly wrong kernel - break the bar on the hard inputs, three of them only there; two systems of
a re-solve case are far apart; and every runner of tests/test_gpu_pcg_ref.py end to end with the C oracle standing in."""
import numpy as np
import pytest

import asm_ref as ar                               # tests/asm_ref.py
import pcg_ref as pr                               # tests/pcg_ref.py
from gato_python_amd import synth
from oracle import c_oracle as co
from oracle import gato_oracle as o

LD = np.longdouble
names = lambda cases: [c.name for c in cases]


def test_the_cases_are_the_issues():
    assert len(pr.CASES) == 20 and len({c.name for c in pr.CASES}) == 20
    assert {(c.S, c.C, c.K, c.dt) for c in pr.CASES if c.route.get("last_pair") == 2} == {(14, 7, 37, pr.F64), (14, 7, 50, pr.F64)}
    assert all(c.route for c in pr.CASES)
    assert all(c.B == pr.BATCH and len({ar.system_of(c.S, c.C, c.K, c.dt, b).G_val.tobytes() for b in range(c.B)}) == c.B
               for c in pr.DZ_CASES if c.B > 1)


def test_dense_bd_and_pcg_ld_on_a_small_system():
    """dense_bd against the oracle's block-row product (garbage in the two unused boundary blocks), pcg_ld against the solution."""
    S, K = 3, 4
    rng = np.random.default_rng(5)
    L, M, R = (rng.standard_normal((K, S, S)) for _ in range(3))
    M = M @ M.transpose(0, 2, 1) + 4 * np.eye(S)
    R[:-1] = L[1:].transpose(0, 2, 1)
    buf = o.pack_bd(L, M, R)
    x = rng.standard_normal((K, S))
    D = pr.dense_bd(buf, S, K)
    assert np.abs(D @ x.reshape(-1).astype(LD) - o.bt_matvec(L, M, R, x).reshape(-1)).max() < 1e-14
    Pd = np.zeros_like(D)
    for k in range(K):
        Pd[k * S:(k + 1) * S, k * S:(k + 1) * S] = ar.inv_ld(M[k])
    b = rng.standard_normal(S * K)
    its = pr.pcg_ld(D, Pd, b, S * K)
    assert len(its) == S * K and pr.rel(its[-1], ar.solve_ld(D, b)) < 1e-15 and pr.rel(its[0], ar.solve_ld(D, b)) > 1e-3


# ---- the bars between the CPU orders: the measurement the factors come from ------------------------------------------------------
@pytest.mark.parametrize("seed", pr.SEEDS)
@pytest.mark.parametrize("case", pr.CASES, ids=names(pr.CASES))
def test_each_cpu_order_is_within_the_bar_of_the_other(case, seed):
    eps = ar.eps_of(case.dt)
    ea, eb = pr.cpu_pcg_errors(case.name, seed)
    for n in pr.NS:
        a, b = ea[f"lambda after {n}"], eb[f"lambda after {n}"]
        print(f"{case.name} seed {seed} n = {n}: {'single-reduction' if case.cg1 else 'numpy'} order {a / eps:.1f} eps, C order {b / eps:.1f} eps")
        assert 0 < a <= ar.bar([b], case.dt, pr.PCG_FACTOR[n]) and 0 < b <= ar.bar([a], case.dt, pr.PCG_FACTOR[n]), (n, a / eps, b / eps)


SOLVES = pr.DZ_CASES + pr.RESOLVE_CASES


@pytest.mark.parametrize("case", SOLVES, ids=names(SOLVES))
def test_each_cpu_order_of_gamma_and_dz_is_within_the_bar_of_the_other(case):
    """gamma of a new right-hand side and dz of a random lambda, every system of every whole-call case."""
    S, C, K, dt = case.S, case.C, case.K, case.dt
    eps = ar.eps_of(dt)
    for b in range(case.B):
        ref, chains = pr.block_reference_of(S, C, K, dt, b), pr.chains_of(S, C, K, dt, b)
        g, c = pr.new_rhs(S, C, K, dt, 0, b, 0)
        lam = ar.random_lambda(S, K, dt, b)
        eg = [pr.lam_error(x, ref.gamma(g, c), S, C, K) for x in pr.cpu_orders_gamma(chains, S, C, K, dt, g, c)]
        ez = [pr.dz_error(x, ref.dz(lam, g), S, C, K) for x in pr.cpu_orders_dz(chains, S, C, K, dt, g, lam)]
        print(f"{case.name} system {b}: gamma {eg[0] / eps:.1f}, {eg[1] / eps:.1f} eps; dz {ez[0] / eps:.1f}, {ez[1] / eps:.1f} eps")
        for e in (eg, ez):
            assert e[0] <= ar.bar([e[1]], dt, pr.FACTOR) and e[1] <= ar.bar([e[0]], dt, pr.FACTOR), (b, [x / eps for x in e])


# ---- BlockReference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ar.DTYPES)
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("S,C", ar.SHAPES)
def test_block_reference_equals_the_dense_reference(S, C, K, dt):
    """gamma and dz (per knot) to 64 longdouble ulps: both sum the same products, S + C + 1 of them at most, in another order.
    lam_kkt and dz_kkt: both references solve S lambda = gamma by solve_ld, with S and gamma equal to those ulps, so the solutions
    differ by that times the condition of S, per knot by the grading on top: a few ulps cannot hold.  Measured 5e-16 at the most;
    held to 1e-14, seven orders below the tightest use made of them (1e-7, a tenth of BASELINE's bar)."""
    ulp = float(np.finfo(LD).eps)
    s = ar.system_of(S, C, K, dt)
    dense, blk = ar.reference_of(S, C, K, dt), pr.BlockReference(s, dt)
    lam = ar.random_lambda(S, K, dt)
    eg = pr.lam_error(blk.gamma(), dense.buf["gamma"], S, C, K)
    ez = pr.dz_error(blk.dz(lam), dense.dz(lam), S, C, K)
    eS = float(np.abs(blk.schur() - dense.S_dense).max() / np.abs(dense.S_dense).max())
    el = pr.lam_error(blk.lam_kkt(), dense.lam_kkt, S, C, K)
    ek = pr.dz_error(blk.dz_kkt(), dense.dz_kkt, S, C, K)
    print(f"{S}/{C}/{K} {dt}: gamma {eg / ulp:.1f}, dz {ez / ulp:.1f}, S {eS / ulp:.1f} ulps; lam_kkt {el:.1e}, dz_kkt {ek:.1e}")
    assert eg <= 64 * ulp and ez <= 64 * ulp and eS <= 64 * ulp
    assert el < 1e-14 and ek < 1e-14
    # ... and a new right-hand side goes through the same code as the system's own
    assert np.array_equal(blk.gamma(blk.g, blk.c), blk.gamma()) and np.array_equal(blk.dz(lam, blk.g), blk.dz(lam))


F64_CASES = [c for c in pr.CASES if c.dt == pr.F64]


@pytest.mark.parametrize("case", F64_CASES, ids=names(F64_CASES))
def test_oracle_whole_solve_is_within_a_tenth_of_the_baseline_bar(case):
    """EXIT_TOL and MAX_ITERS of the GPU suite's converged fp64 solves: with them the C oracle's whole solve is within 1e-7 of
    lam_kkt / dz_kkt, in fewer than two thirds of the cap's iterations."""
    S, C, K, dt = case.key
    s, ref = ar.system_of(S, C, K, dt), pr.block_reference_of(S, C, K, dt)
    lam, dz, it = co.linsys_solve(*s.csr_args(), S, C, K, pr.EXIT_TOL, pr.MAX_ITERS, s.rho, dtype=np.float64)
    el, ez = pr.rel(lam, ref.lam_kkt()), float(np.abs(dz - ref.dz_kkt()).max())
    print(f"{case.name}: {it} iterations, lambda {el:.1e} relative, |dz - dz_ref|_inf {ez:.1e}")
    assert 3 * it < 2 * pr.MAX_ITERS and el < pr.BASELINE / 10 and ez < pr.BASELINE / 10
    # the dense solution of the oracle's own matrices, which test_pcg_routes judges the device's converged lambda by
    assert pr.rel(pr.pcg_truth(S, C, K, dt)[1], ref.lam_kkt()) < pr.BASELINE / 10


# ---- mutations of a numpy restatement ------------------------------------------------------------------------------------------------
def smallest_knot(Sb, S, K):
    return int(np.argmin([np.abs(m).max() for m in o.unpack_bd(Sb, S, K)[1]]))


def pcg_mut(Sb, Pb, gamma, S, K, n, mut=None):
    """oracle.gato_oracle.pcg for n iterations, with (a) S.left of knot K // 2 applied transposed, (b) Pinv.right of knot K - 2
    skipped, (c) entry (0, 1) of S.main of the smallest-scale knot zeroed, (d) at the boundary in front of knot K // 2, the halo
    row of p in the S product taken from the iteration before; mut = None: the oracle's bits."""
    dtype = Sb.dtype
    Sl, Sm, Sr = (x.copy(order="K") for x in o.unpack_bd(Sb, S, K))         # (the oracle's memory layout: its products' bits)
    Pl, Pm, Pr = (x.copy(order="K") for x in o.unpack_bd(Pb, S, K))
    kb = K // 2
    if mut == "a":
        Sl[kb] = Sl[kb].T.copy()
    if mut == "b":
        Pr[K - 2] = 0
    if mut == "c":
        Sm[smallest_knot(Sb, S, K)][0, 1] = 0
    lam = np.zeros((K, S), dtype)
    r = np.asarray(gamma, dtype).reshape(K, S).copy()
    rt = o.bt_matvec(Pl, Pm, Pr, r)
    p = rt.copy()
    p_before = None
    eta = dtype.type(np.sum(r * rt, dtype=dtype))
    for it in range(n):
        ups = o.bt_matvec(Sl, Sm, Sr, p)
        if mut == "d" and p_before is not None:
            ups[kb] += Sl[kb] @ (p_before[kb - 1] - p[kb - 1])
        v = dtype.type(np.sum(p * ups, dtype=dtype))
        alpha = eta / v
        lam = lam + alpha * p
        r = r - alpha * ups
        rt = o.bt_matvec(Pl, Pm, Pr, r)
        eta_new = dtype.type(np.sum(r * rt, dtype=dtype))
        beta = eta_new / eta
        p_before = p
        p = rt + beta * p
        eta = eta_new
    return lam.reshape(-1)


def dz_mut(Gi, Cd, g, lam, S, C, K, mut=None):
    """oracle.gato_oracle.compute_dz, with (e) R_k^-1 replaced by its diagonal, (f) B^T lambda_{k+1} dropped for the last control
    block."""
    dtype = Gi.dtype
    n = S + C
    Qi, Ri = o.unpack_G(Gi, S, C, K)
    if mut == "e":
        Ri = Ri * np.eye(C, dtype=dtype)
    A, B = o.unpack_C(Cd, S, C, K)
    g = np.asarray(g, dtype)
    lam = np.asarray(lam, dtype).reshape(K, S)
    dz = np.zeros(n * K - C, dtype)
    for k in range(K):
        t = g[k * n: k * n + S] - lam[k]
        if k < K - 1:
            t = t - A[k].T @ lam[k + 1]
            rk = g[k * n + S: (k + 1) * n]
            dz[k * n + S: (k + 1) * n] = Ri[k] @ (rk if mut == "f" and k == K - 2 else rk - B[k].T @ lam[k + 1])
        dz[k * n: k * n + S] = Qi[k] @ t
    return dz


def gamma_mut(Gi, Cd, g, c, S, C, K, mut=None):
    """gamma as oracle.gato_oracle.form_schur forms it, from the oracle's own Q^-1, R^-1, with (g) B R^-1 using the diagonal
    of R^-1, (h) c_0 dropped."""
    dtype = Gi.dtype
    n = S + C
    Qi, Ri = o.unpack_G(Gi, S, C, K)
    if mut == "g":
        Ri = Ri * np.eye(C, dtype=dtype)
    A, B = o.unpack_C(Cd, S, C, K)
    g = np.asarray(g, dtype)
    c = np.asarray(c, dtype).reshape(K, S)
    q = np.stack([g[k * n: k * n + S] for k in range(K)])
    r = np.stack([g[k * n + S: (k + 1) * n] for k in range(K - 1)])
    gamma = np.zeros((K, S), dtype)
    gamma[0] = (0 if mut == "h" else c[0]) - Qi[0] @ q[0]
    phi = A @ Qi[:-1]
    BR = B @ Ri
    gt = (Qi[1:] @ q[1:, :, None])[..., 0] - c[1:]
    gt = gt + (phi @ q[:-1, :, None])[..., 0] + (BR @ r[:, :, None])[..., 0]
    gamma[1:] = -gt
    return gamma.reshape(-1)


# the case each mutation is shown at
PCG_MUTANTS = dict(a="mixed-f64-14-7-37", b="pair-f32-14-7-19", c="dpp-f64-32-16-5", d="wg13-f64-14-7-50-threads64")
VEC_MUTANTS = dict(e=(14, 7, 20, pr.F64), f=(14, 7, 9, pr.F32), g=(14, 7, 37, pr.F64), h=(32, 16, 5, pr.F32))


@pytest.mark.parametrize("name", sorted(set(PCG_MUTANTS.values())))
def test_the_restated_pcg_is_the_numpy_oracles(name):
    case = pr.BY_NAME[name]
    S, C, K, dt = case.key
    m = pr.chain_of(S, C, K, dt)
    for n in pr.NS:
        assert np.array_equal(pcg_mut(m["S"], m["Pinv"], m["gamma"], S, K, n), o.pcg(m["S"], m["Pinv"], m["gamma"], S, K, 0.0, n)[0])


@pytest.mark.parametrize("mut", sorted(PCG_MUTANTS))
def test_pcg_mutations_break_the_bar(mut):
    case = pr.BY_NAME[PCG_MUTANTS[mut]]
    S, C, K, dt = case.key
    m, (truth, _) = pr.chain_of(S, C, K, dt), pr.pcg_truth(S, C, K, dt)
    e_or = pr.cpu_pcg_errors(case.name)
    broken = []
    for n in pr.NS:
        e = {f"lambda after {n}": pr.lam_error(pcg_mut(m["S"], m["Pinv"], m["gamma"], S, K, n, mut), truth[n - 1], S, C, K)}
        broken.append(bool(ar.judge(f"{case.name} mutation {mut}", dt, e, e_or, factor=pr.PCG_FACTOR[n])))
    # (d) has no iteration before the first to take its halo row from: there it is the oracle's bits
    assert broken == ([False, True, True] if mut == "d" else [True, True, True])


def vector_mutant(mut, s, dt, ref, chains):
    """-> the buffers of mutation mut ('e' .. 'h') on the system s that are past the bar of its two clean CPU orders."""
    S, C, K = s.S, s.C, s.K
    own = chains[1]                                               # the numpy oracle's assembly: what the restatement restates
    g, c = np.asarray(s.g, dt), np.asarray(s.c, dt)
    if mut in "ef":
        lam = ar.random_lambda(S, K, dt)
        truth = ref.dz(lam)
        clean = dz_mut(own["Ginv"], own["C_dense"], g, lam, S, C, K)
        assert np.array_equal(clean, o.compute_dz(own["Ginv"], own["C_dense"], g, lam, S, C, K))
        e = dict(dz=pr.dz_error(dz_mut(own["Ginv"], own["C_dense"], g, lam, S, C, K, mut), truth, S, C, K))
        e_or = tuple(dict(dz=pr.dz_error(x, truth, S, C, K)) for x in pr.cpu_orders_dz(chains, S, C, K, dt, g, lam))
    else:
        truth = ref.gamma()
        assert np.array_equal(gamma_mut(own["Ginv"], own["C_dense"], g, c, S, C, K), own["gamma"])
        e = dict(gamma=pr.lam_error(gamma_mut(own["Ginv"], own["C_dense"], g, c, S, C, K, mut), truth, S, C, K))
        e_or = tuple(dict(gamma=pr.lam_error(x, truth, S, C, K)) for x in pr.cpu_orders_gamma(chains, S, C, K, dt, g, c))
    return [n for n, _, _ in ar.judge(f"{S}/{C}/{K} {dt} mutation {mut}", dt, e, e_or, factor=pr.FACTOR)]


@pytest.mark.parametrize("mut", sorted(VEC_MUTANTS))
def test_dz_and_gamma_mutations_break_the_bar_on_the_hard_inputs(mut):
    S, C, K, dt = VEC_MUTANTS[mut]
    bad = vector_mutant(mut, ar.system_of(S, C, K, dt), dt, pr.block_reference_of(S, C, K, dt), pr.chains_of(S, C, K, dt))
    assert bad == ["dz" if mut in "ef" else "gamma"]


@pytest.mark.parametrize("mut", "egh")
def test_three_mutations_pass_on_the_synthetic_generator(mut):
    """The hole: synth.make_system has diagonal R_k, so R_k^-1 is its own diagonal, and c_0 = 0 - a dz or a gamma that read only
    the diagonal of R_k^-1, or forgot c_0, gives the same bits as the right one on every input the suite had."""
    S, C, K, dt = VEC_MUTANTS[mut]
    s = synth.make_system(S, C, K, seed=3)
    assert np.all(s.c[:S] == 0)
    chains = tuple(ar.chained_stages(ar.OracleBackend(m), s, dt) for m in (co, o))
    assert vector_mutant(mut, s, dt, pr.BlockReference(s, dt), chains) == []
    own, g, c = chains[1], np.asarray(s.g, dt), np.asarray(s.c, dt)
    if mut == "e":
        lam = ar.random_lambda(S, K, dt)
        same = np.array_equal(dz_mut(own["Ginv"], own["C_dense"], g, lam, S, C, K, mut), dz_mut(own["Ginv"], own["C_dense"], g, lam, S, C, K))
    else:
        same = np.array_equal(gamma_mut(own["Ginv"], own["C_dense"], g, c, S, C, K, mut), own["gamma"])
    assert same


# ---- the re-solve's systems are far apart ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.RESOLVE_CASES, ids=names(pr.RESOLVE_CASES))
def test_the_systems_of_a_resolve_case_are_far_apart(case):
    d = pr.distinct(case)
    print(case.name, "%.2e" % d)
    assert d > pr.DISTINCT


# ---- every GPU runner, the C oracle standing in for the device ---------------------------------------------------------------------------
def passes(facts, bad):
    assert [what for what, ok in facts if not ok] == [] and bad == []
    return len(facts)


@pytest.mark.parametrize("case", pr.CASES, ids=names(pr.CASES))
def test_route_runner_with_the_c_order_standing_in(case):
    n = passes(*pr.run_pcg_route(case, pr.StandIn()))
    assert n == len(case.route) + 1 + len(pr.NS) + (2 if case.dt == pr.F64 else 0)


@pytest.mark.parametrize("case", pr.DZ_CASES, ids=names(pr.DZ_CASES))
def test_dz_runner_with_the_c_order_standing_in(case):
    passes(*pr.run_dz_case(case, pr.StandIn()))


@pytest.mark.parametrize("case,nofuse", pr.RESOLVE_RUNS, ids=[f"{c.name}-{'launch' if n else 'epilogue'}" for c, n in pr.RESOLVE_RUNS])
def test_resolve_runner_with_the_c_order_standing_in(case, nofuse):
    passes(*pr.run_resolve_case(case, nofuse, pr.StandIn()))


def test_a_runner_notices_a_wrong_system_offset():
    """The stand-in with the dz of system 1 handed out as system 2's: run_dz_case lists it."""
    class Shifted(pr.StandIn):
        def solve(self, *a, **k):
            out = super().solve(*a, **k)
            out["dz"][2] = out["dz"][1]
            return out
    facts, bad = pr.run_dz_case(pr.DZ_CASES[-1], Shifted())
    assert [n for n, _, _ in bad] == ["dz"]
