"""The numpy reference of soft bounds in the active-set iteration (tests/box_qp_soft_ref.py) on the CPU:
the rule, zero weights equal to box_qp_pdas_ref, the converged point against SLSQP on the penalised objective, the 1 / w
approach to the hard solution, the gradients against finite differences, the stage restatement, and that the seed walks find
a seed for every case of tests/test_gpu_box_qp_soft.py and - with the mixed blocks cover() demands - for every case of
tests/test_gpu_box_qp_soft_sweep.py."""
import os
import re

import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_pdas_ref as D
import box_qp_polish_ref as P
import box_qp_ref as ref
import box_qp_soft_ref as R
import kkt_grad_ref as kgr
from gato_python_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_on_soft_variables():
    """A soft variable is decided from x alone, whatever its act was; a hard one by box_qp_pdas_ref's rule; x_0 and lo == hi
    as there.  The margin takes the distance to the bounds for soft variables, |y| for hard-active ones."""
    S = 1
    #              x0    soft above  soft inside(was active)  soft below  soft eq  hard active y>0  hard active y<=0  soft free-bounds
    lo = np.array([-1.0, -1.0,       -1.0,                    -1.0,       0.5,     -1.0,            -1.0,             -np.inf])
    hi = np.array([1.0,  1.0,        1.0,                     1.0,        0.5,     1.0,             1.0,              np.inf])
    w = np.array([5.0,   5.0,        5.0,                     5.0,        5.0,     0.0,             0.0,              5.0])
    act = np.array([0,   0,          1,                       1,          0,       1,               1,                0], np.int8)
    x = np.array([3.0,   1.25,       0.75,                    -1.5,       0.7,     1.0,             1.0,              9.0])
    y = np.array([0.0,   0.0,        -1.25,                   -12.5,      0.0,     0.3,             -0.2,             0.0])
    assert AS.next_act(act, x, y, lo, hi, S, w).tolist() == [0, 1, 0, -1, -1, 1, 0, 0]
    assert AS.decision_margin(act, x, y, lo, hi, S, w) == pytest.approx(0.2)      # the hard multiplier -0.2
    assert AS.decision_margin(act, x, np.where(w > 0, y, 1.0), lo, hi, S, w) == pytest.approx(0.25)   # x = 1.25 / 0.75 against hi = 1
    assert P.soft_set(act, w).tolist() == [False, False, True, True, False, False, False, False]


def test_point_of_a_soft_active_variable():
    """y = w (x - b), z = x on a soft-active variable, and the reduced solve is the minimiser of the penalised objective with
    the active set held."""
    s, H, Cm, g, c, lo, hi, w = R.soft_problem(4, 2, 5, 0)
    run = AS.iterate(H, Cm, g, c, lo, hi, 4, w)
    assert run["status"] == AS.CONVERGED
    sa = P.soft_set(run["act"], w)
    assert sa.any()
    b = P.bound_values(run["act"], lo, hi)
    assert np.array_equal(run["y"][sa], (w * (run["x"] - b))[sa]) and np.array_equal(run["z"][sa], run["x"][sa])
    assert np.all((run["x"] > hi)[sa & (run["act"] > 0)]) and np.all((run["x"] < lo)[sa & (run["act"] < 0) & (lo != hi)])
    kk = AS.kkt_residuals(H, Cm, g, c, lo, hi, run["x"], run["y"], run["lam"], w)
    print(kk)
    assert max(kk.values()) <= 1e-9


ZERO = [("control", 6, 3, 9), ("control", 14, 7, 3), ("constructed", 4, 2, 9), ("states", 6, 3, 9), ("states", 2, 1, 20)]


@pytest.mark.parametrize("kind,S,C,K", ZERO)
def test_zero_weights_are_the_hard_reference(kind, S, C, K):
    """With w = 0 the reference is box_qp_pdas_ref.pdas exactly: status, act sequence, margins and x - on problems that
    converge and on hard state boxes that do not."""
    if kind == "control":
        p = D.control_box(S, C, K)[0]
    elif kind == "constructed":
        p = D.constructed_cold(S, C, K)[0]
    elif (S, C) == (2, 1):
        s, H, Cm, g, c, lo, hi, _ = R.double_integrator_soft()
        p = dict(H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi)
    else:
        s, H, Cm, g, c, lo, hi, _ = R.soft_problem(S, C, K, 0)
        p = dict(H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi)
    args = tuple(p[k] for k in ("H", "Cm", "g", "c", "lo", "hi"))
    a = AS.iterate(*args, S)
    b = AS.iterate(*args, S, np.zeros(len(p["g"])))
    print(kind, a["status"], a["iters"])
    assert (a["status"], a["iters"]) == (b["status"], b["iters"])
    assert len(a["trace"]) == len(b["trace"])
    for ta, tb in zip(a["trace"], b["trace"]):
        assert np.array_equal(ta["act"], tb["act"]) and ta["changed"] == tb["changed"]
        assert ta["margin"] == tb["margin"] or (np.isnan(ta["margin"]) and np.isnan(tb["margin"]))
    assert np.array_equal(a["x"], b["x"], equal_nan=True) and np.array_equal(a["lam"], b["lam"], equal_nan=True)
    if kind == "states":
        assert a["status"] != AS.CONVERGED


@pytest.mark.parametrize("S,C,K", [(2, 1, 5), (4, 2, 3)])
def test_converged_point_is_the_slsqp_minimum(S, C, K):
    """scipy's SLSQP on the penalised objective (equalities C x = c, the hard bounds as bounds) from x = 0 reaches the
    reference's converged point within 1e-6."""
    from scipy.optimize import minimize
    p = R.soft_box(S, C, K)[0]
    H, Cm, g, c, lo, hi, w = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi", "w"))
    sv = w > 0
    inf = np.full(len(g), np.inf)
    bounds = list(zip(np.where(sv, -inf, lo), np.where(sv, inf, hi)))
    bounds = [(None if not np.isfinite(l) else l, None if not np.isfinite(h) else h) for l, h in bounds]
    f = lambda x: AS.penalised_objective(H, g, lo, hi, x, w)
    out = minimize(f, np.zeros(len(g)), jac=True, method="SLSQP", bounds=bounds,
                   constraints=[dict(type="eq", fun=lambda x: Cm @ x - c, jac=lambda x: Cm)], options=dict(ftol=1e-16, maxiter=2000))
    err = np.abs(out.x - p["run"]["x"]).max()
    print(out.message, out.nit, "x err", err, "objective", out.fun, f(p["run"]["x"])[0])
    assert err <= 1e-6, err


def test_solution_approaches_the_hard_one_as_one_over_w():
    """A constructed problem on which the hard iteration converges, every bound soft with one weight w.  On the active set x(w) -
    b = y(w) / w and y(w) -> y_hard, so x(w) = x_hard + d / w (1 + O(kappa / w)), where d is the move of the hard solution
    for bounds shifted by y_hard (the reduced solve is linear in the bounds: d is exact) and kappa the stiffness the active
    variables see, the largest eigenvalue of the inverse of their block of the unconstrained KKT inverse.  Over w = 1e2, 1e3,
    1e4: the distance to x_hard shrinks, and w (x(w) - x_hard) is d within 2 kappa / w of |d| (2: the norms differ)."""
    S, C, K = 6, 3, 9
    p = D.constructed_cold(S, C, K)[0]
    H, Cm, g, c, lo, hi, act = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi", "act"))
    N, m = len(g), len(c)
    A = np.flatnonzero(act != 0)
    Kxx = np.linalg.inv(np.block([[H, Cm.T], [Cm, np.zeros((m, m))]]))[:N, :N]
    kappa = 1.0 / np.linalg.eigvalsh(Kxx[np.ix_(A, A)]).min()
    eq = lo == hi
    shift = np.where(act != 0, p["y"], 0.0)
    x1, _, _ = P.reduced_solve(H, Cm, g, c, lo + np.where((act < 0) | eq, shift, 0.0), hi + np.where((act > 0) | eq, shift, 0.0), act)
    d = x1 - p["x"]
    errs, devs = [], []
    for wt in (1e2, 1e3, 1e4):
        run = AS.iterate(H, Cm, g, c, lo, hi, S, np.full(N, wt), act0=act)
        assert run["status"] == AS.CONVERGED and np.array_equal(run["act"], act), wt
        errs.append(np.abs(run["x"] - p["x"]).max())
        devs.append(np.abs(wt * (run["x"] - p["x"]) - d).max() / np.abs(d).max())
        print("w", wt, "|x(w) - x_hard|", errs[-1], "deviation from d / w", devs[-1], "bar", 2 * kappa / wt)
        assert devs[-1] <= 2 * kappa / wt
    assert errs[0] > errs[1] > errs[2] > 0 and devs[0] > devs[1] > devs[2]


# ---- gradients ---------------------------------------------------------------------------------------------------------------
FD_STEP = 1e-6
FD_ROUND = 1e-13                                  # test_box_qp_polish_cpu.py: the relative accuracy of these dense solves


def _solve(inp, rho, act, S):
    H, Cm, g, c = P.dense_from_blocks(inp["Q"], inp["R"], inp["A"], inp["B"], inp["q"], inp["r"], inp["c"], rho)
    C, K = inp["R"].shape[-1], inp["Q"].shape[0]
    lo = ref.dz_layout(inp["x_lo"], inp["u_lo"], S, C, K)
    hi = ref.dz_layout(inp["x_hi"], inp["u_hi"], S, C, K)
    w = ref.dz_layout(inp["x_soft"], inp["u_soft"], S, C, K)
    run = AS.iterate(H, Cm, g, c, lo, hi, S, w, act0=act, eps_abs=1e-9, eps_rel=1e-9)
    return run, (H, Cm, g, c, lo, hi, w)


def _fd_problem(S, C, K):
    """The first walked-style seed (weights 3 on the states, 0.5 on every other control: soft controls too) whose final
    point has every margin >= 1e-3 and both a hard-active and a soft-active non-equality variable."""
    for seed in range(AS.WALK_SEEDS):
        s, H, Cm, g, c, lo, hi, w = R.soft_problem(S, C, K, seed, weight=3.0)
        n = S + C
        idx = np.arange(s.N)
        w[(idx % n >= S) & ((idx // n) % 2 == 1)] = 0.5
        run = AS.iterate(H, Cm, g, c, lo, hi, S, w)
        sa = P.soft_set(run["act"], w)
        if (run["status"] == AS.CONVERGED and run["trace"][-1]["margin"] >= 1e-3 and (sa & (lo != hi)).any()
                and ((run["act"] != 0) & ~sa & (lo != hi)).any()):
            return s, lo, hi, w, run
    raise AssertionError("no seed")


def _fd_check(s, lo, hi, w, run0):
    """soft_grads for all thirteen inputs of box_qp_layer (Q, R symmetric; the weights included) against central differences
    of the penalised-QP solution along a random direction per input.  Every perturbed problem is solved by the iteration
    from the unperturbed act and must converge on it at once - the active set is kept, a condition on the inputs (margins >=
    1e-3 against steps of 1e-6), asserted.  The bound is test_box_qp_polish_cpu.py's.  -> the gradients."""
    S, C, K = s.S, s.C, s.K
    Q, Rm, A, B, q, r, c = kgr.blocks_of(s)
    split = lambda v: P.split_states_controls(v, S, C, K)
    inp = dict(Q=Q, R=Rm, A=A, B=B, q=q, r=r, c=c)
    for name, v in (("lo", lo), ("hi", hi), ("soft", w)):
        inp["x_" + name], inp["u_" + name] = split(v)
    act = run0["act"]
    run, (H, Cm, g, cc, lo2, hi2, w2) = _solve(inp, s.rho, act, S)
    assert run["status"] == AS.CONVERGED and run["iters"] == 1 and np.array_equal(lo2, lo) and np.array_equal(w2, w)
    x, lam = run["x"], run["lam"]
    rng = np.random.default_rng(7)
    xbar, lambar = rng.standard_normal(len(x)), rng.standard_normal(len(lam))
    gr = P.grads(H, Cm, act, x, lam, xbar, lambar, S, C, K, w=w, lo=lo, hi=hi)
    sa = P.soft_set(act, w)
    assert not gr["a"][(act != 0) & ~sa].any() and gr["a"][sa].any()
    L = lambda rr: float(xbar @ rr["x"] + lambar @ rr["lam"])
    lmag = float(np.abs(xbar) @ np.abs(x) + np.abs(lambar) @ np.abs(lam))
    for key in ("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi", "x_soft", "u_soft"):
        V = rng.standard_normal(inp[key].shape)
        if key in ("Q", "R"):
            V = 0.5 * (V + np.swapaxes(V, -1, -2))
        partner = None
        if key.endswith(("_lo", "_hi")):
            V = np.where(np.isfinite(inp[key]), V, 0.0)
            eq = inp[key[0] + "_lo"] == inp[key[0] + "_hi"]
            if key.endswith("_hi"):
                V = np.where(eq, 0.0, V)                 # where lo == hi the gradient goes to lo ...
            else:
                partner = (key[0] + "_hi", np.where(eq, V, 0.0))   # ... for a shift of both bounds together
        if key.endswith("_soft"):
            V = np.where(inp[key] > 0, V, 0.0)           # a hard bound stays hard
        vals = []
        for sgn in (1.0, -1.0):
            pert = dict(inp)
            pert[key] = inp[key] + sgn * FD_STEP * V
            if partner is not None:
                pert[partner[0]] = inp[partner[0]] + sgn * FD_STEP * partner[1]
            rp, _ = _solve(pert, s.rho, act, S)
            assert rp["status"] == AS.CONVERGED and rp["iters"] == 1, (key, sgn)
            vals.append(L(rp))
        fd = (vals[0] - vals[1]) / (2 * FD_STEP)
        an = float(np.sum(gr[key] * V))
        tol = 1e-6 * max(1.0, float(np.sum(np.abs(gr[key] * V)))) + FD_ROUND * lmag / FD_STEP
        print(key, an, fd, abs(an - fd), tol)
        assert abs(an - fd) <= tol, (key, an, fd, tol)
    return gr


@pytest.mark.parametrize("S,C,K", [(4, 2, 5), (6, 3, 4)])
def test_gradients_match_finite_differences(S, C, K):
    gr = _fd_check(*_fd_problem(S, C, K))
    assert np.abs(gr["x_soft"]).max() > 0 and np.abs(gr["u_soft"]).max() > 0


def _fd_mixed_problem(S, C, K):
    """The first mixed_problem seed whose final point has every margin >= 1e-3, a soft-active control with lo != hi and a
    hard-active non-equality variable and a soft-active state, and whose final reduced matrix has cond <= 1e7.  A difference quotient divides the
    rounding of two dense solves by the step, and FD_ROUND allows them 1e-13: _fd_problem's matrices have cond 6e5 and keep
    it; 6/3/4 seed 0, next to an active set without LICQ (cond 7e9, |lam| 2e3), is 2e-2 off in R for that reason alone."""
    n = S + C
    for seed in range(AS.WALK_SEEDS):
        s, H, Cm, g, c, lo, hi, w = R.mixed_problem(S, C, K, seed)
        run = AS.iterate(H, Cm, g, c, lo, hi, S, w)
        sa = P.soft_set(run["act"], w)
        if (run["status"] == AS.CONVERGED and run["trace"][-1]["margin"] >= 1e-3
                and (sa & (lo != hi) & (np.arange(s.N) % n >= S)).any() and ((run["act"] != 0) & ~sa & (lo != hi)).any()
                and (sa & (np.arange(s.N) % n < S)).any() and np.linalg.cond(P.reduced_matrix(H, Cm, run["act"], w)) <= 1e7):
            return s, lo, hi, w, run
    raise AssertionError("no seed")


@pytest.mark.parametrize("S,C,K", [(4, 2, 5), (6, 3, 4)])
def test_gradients_match_finite_differences_mixed(S, C, K):
    """_fd_check on a mixed problem: the directions of u_soft, u_lo and u_hi reach a soft-active control, whose expected weight
    and bound gradients are nonzero."""
    s, lo, hi, w, run = _fd_mixed_problem(S, C, K)
    gr = _fd_check(s, lo, hi, w, run)
    sc = P.split_states_controls(P.soft_set(run["act"], w) & (lo != hi), S, C, K)[1] > 0
    assert sc.any() and np.abs(gr["u_soft"][sc]).max() > 0
    assert np.abs(gr["u_lo"][sc]).max() + np.abs(gr["u_hi"][sc]).max() > 0
    assert np.abs(gr["x_soft"]).max() > 0


# ---- the stage restatement and sparse form --------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", [(4, 2, 9), (14, 7, 3)])
def test_stage_path_is_the_reduced_solve(S, C, K):
    """stage_solve in fp64 - the soft rule on the masked Gauss-Jordan inverses and right-hand sides, Schur complement, PCG, dz -
    against the dense solve of the reduced matrix on every act of a walked run.  Bar: test_box_qp_polish_cpu.py's 1e-9."""
    p = R.soft_box(S, C, K)[0]
    for t in p["run"]["trace"]:
        xr, _, lr = P.reduced_solve(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], t["act"], p["w"])
        x, lam, iters = P.reduced_stage_solve(p["s"], p["lo"], p["hi"], t["act"], np.float64, exit_tol=1e-30, w=p["w"])
        ex = np.abs(x - xr).max() / max(1.0, np.abs(xr).max())
        el = np.abs(lam - lr).max() / max(1.0, np.abs(lr).max())
        print("pcg iterations", iters, "x", ex, "lam", el)
        assert ex <= 1e-9 and el <= 1e-9
    status, acts = AS.stage_iterate(p["s"], p["lo"], p["hi"], np.float64, 1e-6, p["w"], exit_tol=1e-30)
    assert status == AS.CONVERGED and len(acts) == p["run"]["iters"]


def test_sparse_reference_equals_dense():
    s, H, Cm, g, c, lo, hi, w = R.soft_problem(4, 2, 9, 1)
    Hs, Cs, gs, cs = ref.sparse_parts(s)
    a = AS.iterate(H, Cm, g, c, lo, hi, 4, w)
    b = AS.iterate(Hs, Cs, gs, cs, lo, hi, 4, w)
    assert a["status"] == b["status"] == AS.CONVERGED and a["iters"] == b["iters"] and np.array_equal(a["act"], b["act"])
    assert np.abs(a["x"] - b["x"]).max() <= 1e-9 and np.abs(a["lam"] - b["lam"]).max() <= 1e-9
    assert all(abs(ta["margin"] - tb["margin"]) <= 1e-9 for ta, tb in zip(a["trace"], b["trace"]))


# ---- the cases of tests/test_gpu_box_qp_soft.py have seeds --------------------------------------------------------------------
COLD = [(S, C, K) for S, C in R.SHAPES for K in R.COLD_K]


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_walk_finds_an_fp64_seed(S, C, K):
    ps = R.soft_box(S, C, K)
    assert ps and ps[0]["seed"] < AS.WALK_SEEDS
    p = ps[0]
    run = p["run"]
    n = S + C
    idx = np.arange(p["s"].N)
    assert np.array_equal(p["w"] > 0, idx % n < S)                               # every state soft, every control hard
    if K >= 3:
        j = (K - 1) * n
        assert p["lo"][j] == p["hi"][j] and p["w"][j] > 0 and run["act"][j] == -1
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "cond", AS.max_cond(run, p["H"], p["Cm"], p["w"]))
    assert AS.walk_ok(run, p["H"], p["Cm"], p["w"], R.soft_active_on_the_way(p))


@pytest.mark.parametrize("S,C,K", R.F32_CASES, ids=["%d-%d-%d" % c for c in R.F32_CASES])
def test_walk_finds_an_fp32_seed(S, C, K):
    ps = R.soft_box(S, C, K, f32=True)
    assert ps and ps[0]["seed"] < AS.WALK_SEEDS
    print("seed", ps[0]["seed"], "solves", ps[0]["run"]["iters"])
    assert AS.f32_ok(ps[0])


def test_the_other_gpu_cases_exist():
    """The batch's two soft seeds with different solve counts, a hard state box that does not converge, the double integrator,
    and the long horizon: CONVERGED, with soft-active and hard-active variables past knot 8192."""
    S, C, K, B = R.BATCH
    a, b = R.soft_box(S, C, K, count=2)
    assert a["run"]["iters"] != b["run"]["iters"]
    s = synth.make_system(S, C, K, seed=0)
    H, Cm, g, c = ref.parts(s)
    lo, hi = P.boxes(s, 1, eq=True, states=True)
    assert AS.iterate(H, Cm, g, c, lo, hi, S)["status"] != AS.CONVERGED
    s, H, Cm, g, c, lo, hi, w = R.double_integrator_soft()
    assert AS.iterate(H, Cm, g, c, lo, hi, 2)["status"] in (AS.MAX_ITERS, AS.NONFINITE)
    run = AS.iterate(H, Cm, g, c, lo, hi, 2, w)
    print("double integrator: solves", run["iters"], "margin", AS.min_margin(run), "cond", AS.max_cond(run, H, Cm, w))
    assert run["status"] == AS.CONVERGED and AS.min_margin(run) >= AS.MARGIN and P.soft_set(run["act"], w).any()
    p = R.soft_long()
    run = p["run"]
    n = 3
    sa = P.soft_set(run["act"], p["w"])
    print("long: solves", run["iters"], "margin", AS.min_margin(run), "|x|", np.abs(run["x"]).max())
    assert run["status"] == AS.CONVERGED
    assert (np.flatnonzero(sa) // n >= 8192).any() and (np.flatnonzero((run["act"] != 0) & ~sa) // n >= 8192).any()


# ---- mixed problems: the cases of tests/test_gpu_box_qp_soft_sweep.py -----------------------------------------------------------
def _issue_need(S, C, K):
    """What the mixed walks must cover at the least, whatever cover_need asks: (a) everywhere, all three for S >= 6 and
    K >= 3, (b) and (c) at 4/2 for K in (3, 9)."""
    full = (S >= 6 and K >= 3) or (S == 4 and K in (3, 9))
    return True, full, full


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_mixed_walk_finds_an_fp64_seed(S, C, K):
    """The walk finds a seed; its weights are drawn per variable, on states and controls alike; the reference run meets the
    seed rule and cover(), recomputed here, meets cover_need and the least this file demands; the final point satisfies the
    penalised KKT system."""
    ps = R.mixed_box(S, C, K)
    assert ps and ps[0]["seed"] < AS.WALK_SEEDS
    p = ps[0]
    run, w, lo, hi = p["run"], p["w"], p["lo"], p["hi"]
    ctl = np.arange(p["s"].N) % (S + C) >= S
    assert (w > 0).any() and (w == 0).any() and np.all((w == 0) | ((w >= 1.0) & (w <= 1e3)))
    if S >= 4:                                                                   # 2/1/2 has a single control
        assert all((w[part] > 0).any() and (w[part] == 0).any() for part in (ctl, ~ctl))
    assert len(np.unique(w[w > 0])) == (w > 0).sum()
    assert AS.walk_ok(run, p["H"], p["Cm"], w, R.soft_active_on_the_way(p))
    cov = R.cover(run, w, lo, hi, S, C, K)
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "cond", AS.max_cond(run, p["H"], p["Cm"], w), "cover", cov)
    assert cov == p["cover"] and R.covers(cov, R.cover_need(S, C, K)) and R.covers(cov, _issue_need(S, C, K))
    assert R.covers(R.cover_need(S, C, K), _issue_need(S, C, K))
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], lo, hi, run["x"], run["y"], run["lam"], w)
    print(kk)
    assert max(kk.values()) <= 1e-9


def test_cover_on_a_hand_made_trace():
    """2/1/3: dz layout x0 x0 u0 | x1 x1 u1 | x2 x2.  (a) needs a soft-active control off lo == hi; (b) a knot's states, (c) a
    knot's controls hard- and soft-active in ONE act - a single control per knot can never be."""
    S, C, K = 2, 1, 3
    lo, hi = -np.ones(8), np.ones(8)
    w = np.array([0, 0, 5.0, 5.0, 0, 0, 0, 5.0])
    tr = lambda *acts: dict(trace=[dict(act=np.array(a, np.int8)) for a in acts])
    assert R.cover(tr([0, 0, 1, 0, 0, 0, 0, 0]), w, lo, hi, S, C, K) == (True, False, False)
    assert R.cover(tr([0, 0, 0, 1, -1, 0, 0, 0]), w, lo, hi, S, C, K) == (False, True, False)
    assert R.cover(tr([0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, -1, 0, 0, 0]), w, lo, hi, S, C, K) == (False, False, False)   # two acts
    assert R.cover(tr([0, 0, 0, 1, 0, 0, -1, 0]), w, lo, hi, S, C, K) == (False, False, False)                              # two knots
    assert R.cover(tr([0, 0, 1, 0, 0, -1, 0, 0]), w, lo, hi, S, C, K) == (True, False, False)                               # two knots
    eq = np.where(np.arange(8) == 2, 1.0, lo)
    assert R.cover(tr([0, 0, -1, 0, 0, 0, 0, 0]), w, eq, hi, S, C, K) == (False, False, False)                              # lo == hi
    w2 = np.array([0, 0, 5.0, 0, 0, 0, 0, 0, 0, 0])                                                                         # 2/2/3
    assert R.cover(tr([0, 0, 1, -1, 0, 0, 0, 0, 0, 0]), w2, -np.ones(10), np.ones(10), 2, 2, 3) == (True, False, True)


def test_mixed_walks_find_their_other_seeds():
    """4/2/3 has two fp64 seeds with mixed states and mixed controls; every shape has an fp32 seed at K = MIXED_F32_K with a
    soft-active control, from 6/3 up with all of cover(), 4/2 with mixed controls; a kept run has a soft-active variable on the
    last knot; the layer cases end on an act with a soft-active control."""
    two = R.mixed_box(4, 2, 3, count=2)
    assert len(two) == 2 and all(p["cover"] == (True, True, True) for p in two)
    last = False
    for S, C in R.SHAPES:
        ps = R.mixed_box(S, C, R.MIXED_F32_K, f32=True)
        assert ps and ps[0]["seed"] < AS.WALK_SEEDS
        p = ps[0]
        print((S, C), "fp32 seed", p["seed"], "solves", p["run"]["iters"], "cover", p["cover"])
        assert AS.f32_ok(p) and p["cover"] == R.cover(p["run"], p["w"], p["lo"], p["hi"], S, C, R.MIXED_F32_K)
        assert p["cover"][0] and (S < 4 or p["cover"][2]) and (S < 6 or p["cover"][1])
        for K in R.COLD_K:
            q = R.mixed_box(S, C, K)[0]
            last |= bool(P.soft_set(q["run"]["act"], q["w"])[(K - 1) * (S + C):].any())
    assert last
    for S, C, K in R.LAYER_CASES:
        p = R.mixed_layer_box(S, C, K)
        assert p is not None
        sa = P.soft_set(p["run"]["act"], p["w"])
        assert (sa & (np.arange(len(sa)) % (S + C) >= S) & (p["lo"] != p["hi"])).any()
        print((S, C, K), "layer seed", p["seed"])


@pytest.mark.parametrize("S,C,K", [(4, 2, 3), (6, 3, 9), (14, 7, 3)])
def test_mixed_point_is_a_minimum_over_feasible_perturbations(S, C, K):
    """The reference's final point of a mixed problem: penalised_objective's gradient is -(C^T lam + y) there (stationarity),
    and no step that keeps C x = c and the hard-active variables on their bounds - small enough to keep every hard free
    variable inside its box - decreases penalised_objective.  Along such a d the first-order term vanishes and f is convex,
    so f(x + t d) - f(x) >= 0 up to the rounding of evaluating f: 1e-12 of the sum of the magnitudes of its terms."""
    from scipy.linalg import null_space
    p = R.mixed_box(S, C, K)[0]
    H, Cm, g, lo, hi, w, run = (p[k] for k in ("H", "Cm", "g", "lo", "hi", "w", "run"))
    x = run["x"]
    f0, grad = AS.penalised_objective(H, g, lo, hi, x, w)
    assert np.abs(grad + Cm.T @ run["lam"] + np.where(w > 0, 0.0, run["y"])).max() <= 1e-9
    hard = (run["act"] != 0) & ~P.soft_set(run["act"], w)
    Z = null_space(np.vstack([Cm, np.eye(len(x))[hard]]))
    assert Z.shape[1] > 0
    hv = ~(w > 0)
    room = np.minimum(x - lo, hi - x)[hv & ~hard].min()
    assert room > 0
    dist = x - np.clip(x, lo, hi)
    mag = 0.5 * np.abs(x) @ np.abs(H) @ np.abs(x) + np.abs(g) @ np.abs(x) + 0.5 * (w * dist * dist).sum()
    rng = np.random.default_rng(3)
    worst = np.inf
    for t in (1e-1, 1e-3, 1e-5):
        for _ in range(20):
            d = Z @ rng.standard_normal(Z.shape[1])
            d[hard] = 0.0                                                        # the null space leaves 1e-18 there
            d *= min(t, 0.5 * room) / np.abs(d).max()
            xp = x + d
            assert np.abs(Cm @ d).max() <= 1e-15 and np.all((xp >= lo)[hv & ~hard]) and np.all((xp <= hi)[hv & ~hard])
            worst = min(worst, AS.penalised_objective(H, g, lo, hi, xp, w)[0] - f0)
    print("smallest f(x + d) - f(x)", worst, "rounding bar", 1e-12 * mag)
    assert worst >= -1e-12 * mag


def test_mixed_converged_point_is_the_slsqp_minimum():
    """test_converged_point_is_the_slsqp_minimum on a mixed problem: hard and soft bounds on states and controls."""
    from scipy.optimize import minimize
    p = R.mixed_box(4, 2, 3)[0]
    H, Cm, g, c, lo, hi, w = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi", "w"))
    sv = w > 0
    inf = np.full(len(g), np.inf)
    bounds = [(None if not np.isfinite(l) else l, None if not np.isfinite(h) else h)
              for l, h in zip(np.where(sv, -inf, lo), np.where(sv, inf, hi))]
    f = lambda x: AS.penalised_objective(H, g, lo, hi, x, w)
    out = minimize(f, np.zeros(len(g)), jac=True, method="SLSQP", bounds=bounds,
                   constraints=[dict(type="eq", fun=lambda x: Cm @ x - c, jac=lambda x: Cm)], options=dict(ftol=1e-16, maxiter=2000))
    err = np.abs(out.x - p["run"]["x"]).max()
    print(out.message, out.nit, "x err", err)
    assert err <= 1e-6, err


@pytest.mark.parametrize("S,C,K", [(4, 2, 9), (6, 3, 3), (14, 7, 3)])
def test_zero_weights_on_a_mixed_box_are_the_hard_reference(S, C, K):
    """On a mixed problem's box with w = 0, over every act its run solved on: reduced_matrix and reduced_solve are
    box_qp_polish_ref's and next_act is box_qp_pdas_ref's, bit for bit (a hard state box can be singular: NaN equals NaN);
    and the whole iteration is box_qp_pdas_ref.pdas."""
    p = R.mixed_box(S, C, K)[0]
    H, Cm, g, c, lo, hi = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi"))
    zero = np.zeros(len(g))
    for t in p["run"]["trace"]:
        act = t["act"]
        assert np.array_equal(P.reduced_matrix(H, Cm, act, zero), P.reduced_matrix(H, Cm, act))
        with np.errstate(all="ignore"):
            got, want = P.reduced_solve(H, Cm, g, c, lo, hi, act, zero), P.reduced_solve(H, Cm, g, c, lo, hi, act)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))
        x, y = np.nan_to_num(want[0]), np.nan_to_num(want[1])
        assert np.array_equal(AS.next_act(act, x, y, lo, hi, S, zero), AS.next_act(act, x, y, lo, hi, S))
    a, b = AS.iterate(H, Cm, g, c, lo, hi, S), AS.iterate(H, Cm, g, c, lo, hi, S, zero)
    assert (a["status"], a["iters"]) == (b["status"], b["iters"]) and len(a["trace"]) == len(b["trace"])
    assert all(np.array_equal(ta["act"], tb["act"]) and ta["changed"] == tb["changed"] for ta, tb in zip(a["trace"], b["trace"]))
    assert np.array_equal(a["x"], b["x"], equal_nan=True) and np.array_equal(a["lam"], b["lam"], equal_nan=True)


def test_the_batch_of_weights_and_the_mixed_long_horizon_exist():
    """The four weight vectors on one 14/7/9 system: a seed below WALK_SEEDS on which all four reference runs converge under
    weight_batch_ok, the vectors as named, the mixed and the scaled run on different points.  mixed_long: CONVERGED, with a
    soft-active control off lo == hi and a hard-active variable among the knots >= 8192."""
    got = R.weight_batch_box()
    assert got is not None and got[0] < AS.WALK_SEEDS
    seed, prob, ws, runs = got
    s, H, Cm, g, c, lo, hi, w = prob
    print("batch seed", seed, [(r["iters"], AS.min_margin(r), AS.max_cond(r, H, Cm, wi)) for wi, r in zip(ws, runs)])
    assert all(r["status"] == AS.CONVERGED for r in runs) and R.weight_batch_ok(prob, ws, runs)
    assert np.array_equal(ws[0], w) and np.array_equal(ws[1], 10.0 * w) and not ws[2].any() and np.array_equal(ws[3], R.state_weights(s))
    ctl = np.arange(s.N) % (s.S + s.C) >= s.S
    assert (w[ctl] > 0).any() and (w[~ctl] > 0).any() and (w == 0).any()
    assert np.abs(runs[0]["x"] - runs[1]["x"]).max() > 1e-3
    assert any(P.soft_set(t["act"], w)[ctl].any() for t in runs[0]["trace"])
    for wi, r in zip(ws, runs):
        kk = AS.kkt_residuals(H, Cm, g, c, lo, hi, r["x"], r["y"], r["lam"], wi)
        assert max(kk.values()) <= 1e-9, kk
    p = R.mixed_long()
    run = p["run"]
    n = 3
    idx = np.arange(p["s"].N)
    sa = P.soft_set(run["act"], p["w"])
    print("long: seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "|x|", np.abs(run["x"]).max())
    assert run["status"] == AS.CONVERGED
    assert (sa & (idx // n >= 8192) & (idx % n >= 2) & (p["lo"] != p["hi"])).any()
    assert ((run["act"] != 0) & ~sa & (idx // n >= 8192)).any()
    ctl = idx % n >= 2
    assert (p["w"][ctl] > 0).any() and (p["w"][ctl] == 0).any() and np.all(p["w"][~ctl] > 0)


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gato_hip.h")).read()
    from gato_python_amd import _lib
    L = _lib.lib()
    for name in ("gato_box_qp_pdas_soft", "gato_box_qp_soft_grad"):
        assert re.search(r"int\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name)
