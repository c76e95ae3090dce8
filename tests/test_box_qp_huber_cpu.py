"""The numpy reference of capped (Huber) soft bounds in the active-set iteration (tests/box_qp_huber_ref.py, DESIGN.md section
3.11) on the CPU: the rule, infinite caps equal to box_qp_soft_ref, the converged point against SLSQP on the Huber objective,
the gradients of all fifteen layer inputs against central differences, the stage restatement, and that the seed walks find a
seed for every case of tests/test_gpu_box_qp_huber.py."""
import os
import re

import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_huber_ref as R
import box_qp_polish_ref as P
import box_qp_ref as ref
import box_qp_soft_ref as SR
import kkt_grad_ref as kgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_on_capped_variables():
    """A soft variable with a finite cap: +-2 where the product w (x - b) passes the cap, +-1 outside its bounds below it, 0
    inside; lo == hi: +-2 or -1; x_0 stays 0; a soft variable without a finite cap and a hard one follow box_qp_soft_ref."""
    S = 1
    #              x0    sat above  quad above  inside  quad below  sat below  eq quad  eq sat+  eq sat-  no cap   hard y>0  cap 0
    lo = np.array([-1.0, -1.0,      -1.0,       -1.0,   -1.0,       -1.0,      0.5,     0.5,     0.5,     -1.0,    -1.0,     -1.0])
    hi = np.array([1.0,  1.0,       1.0,        1.0,    1.0,        1.0,       0.5,     0.5,     0.5,     1.0,     1.0,      1.0])
    w = np.array([4.0,   4.0,       4.0,        4.0,    4.0,        4.0,       4.0,     4.0,     4.0,     4.0,     0.0,      4.0])
    m = np.array([1.0,   1.0,       1.0,        1.0,    1.0,        1.0,       1.0,     1.0,     1.0,     np.inf,  1.0,      0.0])
    act = np.array([0,   0,         2,          1,      0,          -1,        -1,      -1,      2,       0,       1,        0], np.int8)
    x = np.array([9.0,   1.5,       1.125,      0.5,    -1.125,     -1.5,      0.625,   1.0,     0.0,     9.0,     1.0,      1.25])
    y = np.array([0.0,   0.0,       0.0,        0.0,    0.0,        0.0,       0.0,     0.0,     0.0,     0.0,     0.3,      0.0])
    assert AS.next_act(act, x, y, lo, hi, S, w, m).tolist() == [0, 2, 1, 0, -1, -2, -1, 2, -2, 1, 1, 2]
    # a tie is not past the cap: at x = b +- m / w exactly the product equals m and the variable stays quadratic-active
    one = lambda v: np.array([0.0, v])
    tie = lambda xv: AS.next_act(np.zeros(2, np.int8), one(xv), np.zeros(2), one(-1.0), one(1.0), S, one(4.0), one(1.0))[1]
    assert tie(1.25) == 1 and tie(-1.25) == -1
    # the switching points are b +- m / w = b +- 0.25: x = 1.125 is 0.125 from hi and 0.125 from hi + 0.25
    assert AS.decision_margin(act, x, y, lo, hi, S, w, np.where(np.arange(12) == 2, m, np.inf)) == pytest.approx(0.125)
    only = lambda j, cap: np.where(np.arange(12) == j, cap, np.inf)
    assert AS.decision_margin(act, x, y, lo, hi, S, w, only(1, 1.9)) == pytest.approx(0.025)     # x = 1.5 against hi + 1.9 / 4
    assert P.sat_set(act).tolist() == [j in (2, 8) for j in range(12)]
    assert AS.quad_set(act, w).tolist() == [j in (3, 5, 6, 7) for j in range(12)]


def test_point_of_a_saturated_variable():
    """y = s m bit for bit and z = x on a saturated variable, w (x - b) beyond the cap there and within it on the soft
    quadratic-active set; the converged point satisfies the Huber KKT system."""
    p = R.huber_box(6, 3, 9)[0]
    run, w, m, lo, hi = p["run"], p["w"], p["m"], p["lo"], p["hi"]
    sat, quad = P.sat_set(run["act"]), AS.quad_set(run["act"], w)
    assert sat.any() and quad.any()
    assert np.array_equal(run["y"][sat], np.sign(run["act"])[sat] * m[sat]) and np.array_equal(run["z"][sat], run["x"][sat])
    b = P.bound_values(run["act"], lo, hi)
    assert np.all((np.sign(run["act"]) * w * (run["x"] - b))[sat] > m[sat]) and np.all(np.abs(run["y"])[quad] <= m[quad])
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], lo, hi, run["x"], run["y"], run["lam"], w, m)
    print(kk)
    assert max(kk.values()) <= 1e-9


def test_an_act_that_disagrees_with_its_point_fails_the_test():
    """On a converged point: a saturated variable declared quadratic (|y| = w |x - b| > m) and a quadratic one declared
    saturated (s w (x - b) < m) both fail the acceptance test through the capped additions alone."""
    p = R.huber_box(6, 3, 9)[0]
    run, w, m = p["run"], p["w"], p["m"]
    args = tuple(p[k] for k in ("H", "Cm", "g", "c", "lo", "hi"))
    assert AS.point(*args, run["act"], run["x"], run["y"], run["lam"], 1e-6, 1e-6, w, m)[4]
    for frm in (P.sat_set(run["act"]), AS.quad_set(run["act"], w) & (p["lo"] != p["hi"])):
        j = np.flatnonzero(frm)[0]
        act = run["act"].copy()
        act[j] = np.sign(act[j]) * (1 if abs(act[j]) == 2 else 2)
        x, y, lam = P.reduced_solve(*args, act, w, m)
        exc = AS.cap_excess(act, x, y, p["lo"], p["hi"], w, m)
        print(j, "act", run["act"][j], "->", act[j], "excess", exc[j])
        assert exc[j] > 1e-3 and not AS.point(*args, act, x, y, lam, 1e-6, 1e-6, w, m)[4]


NOCAP = [(6, 3, 9, 1e2), (14, 7, 3, 1e2), (4, 2, 9, 1e4), (2, 1, 20, 1e2)]


@pytest.mark.parametrize("S,C,K,weight", NOCAP)
def test_infinite_caps_are_the_soft_reference(S, C, K, weight):
    """With every cap +inf the reference is box_qp_soft_ref.pdas_soft exactly: status, act sequence, margins and x."""
    if (S, C) == (2, 1):
        s, H, Cm, g, c, lo, hi, w = SR.double_integrator_soft()
    else:
        s, H, Cm, g, c, lo, hi, w = SR.soft_problem(S, C, K, 0, weight=weight)
    a = AS.iterate(H, Cm, g, c, lo, hi, S, w)
    b = AS.iterate(H, Cm, g, c, lo, hi, S, w, np.full(len(g), np.inf))
    print(a["status"], a["iters"])
    assert (a["status"], a["iters"]) == (b["status"], b["iters"]) and len(a["trace"]) == len(b["trace"])
    for ta, tb in zip(a["trace"], b["trace"]):
        assert np.array_equal(ta["act"], tb["act"]) and ta["changed"] == tb["changed"]
        assert ta["margin"] == tb["margin"] or (np.isnan(ta["margin"]) and np.isnan(tb["margin"]))
    assert np.array_equal(a["x"], b["x"], equal_nan=True) and np.array_equal(a["lam"], b["lam"], equal_nan=True)


def _slsqp_seed(S, C, K):
    """The first huber_problem seed whose cold run converges on a final act with a saturated variable."""
    for seed in range(AS.WALK_SEEDS):
        s, H, Cm, g, c, lo, hi, w, m = R.huber_problem(S, C, K, seed)
        run = AS.iterate(H, Cm, g, c, lo, hi, S, w, m)
        if run["status"] == AS.CONVERGED and P.sat_set(run["act"]).any():
            return (H, Cm, g, c, lo, hi, w, m), run, seed
    raise AssertionError("no seed")


@pytest.mark.parametrize("S,C,K", [(2, 1, 5), (4, 2, 3)])
def test_converged_point_is_the_slsqp_minimum(S, C, K):
    """scipy's SLSQP on the Huber-penalised objective (equalities C x = c, the hard bounds as bounds) from x = 0 reaches the
    reference's converged point - its final act holds a saturated variable - within 1e-6."""
    from scipy.optimize import minimize
    (H, Cm, g, c, lo, hi, w, m), run, seed = _slsqp_seed(S, C, K)
    sv = w > 0
    inf = np.full(len(g), np.inf)
    bounds = [(None if not np.isfinite(l) else l, None if not np.isfinite(h) else h)
              for l, h in zip(np.where(sv, -inf, lo), np.where(sv, inf, hi))]
    f = lambda x: AS.penalised_objective(H, g, lo, hi, x, w, m)
    out = minimize(f, np.zeros(len(g)), jac=True, method="SLSQP", bounds=bounds,
                   constraints=[dict(type="eq", fun=lambda x: Cm @ x - c, jac=lambda x: Cm)], options=dict(ftol=1e-16, maxiter=2000))
    err = np.abs(out.x - run["x"]).max()
    print("seed", seed, out.message, out.nit, "x err", err, "objective", out.fun, f(run["x"])[0])
    assert err <= 1e-6, err


# ---- gradients ---------------------------------------------------------------------------------------------------------------
FD_STEP = 1e-6
FD_ROUND = 1e-13                                  # test_box_qp_polish_cpu.py: the relative accuracy of these dense solves
KEYS15 = ("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi", "x_soft", "u_soft", "x_soft_max", "u_soft_max")


def _solve(inp, rho, act, S):
    H, Cm, g, c = P.dense_from_blocks(inp["Q"], inp["R"], inp["A"], inp["B"], inp["q"], inp["r"], inp["c"], rho)
    C, K = inp["R"].shape[-1], inp["Q"].shape[0]
    lo = ref.dz_layout(inp["x_lo"], inp["u_lo"], S, C, K)
    hi = ref.dz_layout(inp["x_hi"], inp["u_hi"], S, C, K)
    w = ref.dz_layout(inp["x_soft"], inp["u_soft"], S, C, K)
    m = ref.dz_layout(inp["x_soft_max"], inp["u_soft_max"], S, C, K)
    run = AS.iterate(H, Cm, g, c, lo, hi, S, w, m, act0=act, eps_abs=1e-9, eps_rel=1e-9)
    return run, (H, Cm, g, c, lo, hi, w, m)


def _fd_problem(S, C, K):
    """The first seed (weights 30 on the states with cap 0.3, weight 5 with cap 0.1 on every other control: soft controls too)
    whose final point has every margin >= 1e-3, a saturated state and a saturated control off lo == hi, a soft
    quadratic-active variable and a hard-active one, and a final reduced matrix with cond <= 1e7."""
    n = S + C
    for seed in range(4 * AS.WALK_SEEDS):
        s, H, Cm, g, c, lo, hi, w, m = R.huber_problem(S, C, K, seed, weight=30.0, cap=0.3)
        idx = np.arange(s.N)
        uc = (idx % n >= S) & ((idx // n) % 2 == 1)
        w[uc], m[uc] = 5.0, 0.1
        run = AS.iterate(H, Cm, g, c, lo, hi, S, w, m)
        if run["status"] != AS.CONVERGED or run["trace"][-1]["margin"] < 1e-3:
            continue
        sat, quad = P.sat_set(run["act"]) & (lo != hi), AS.quad_set(run["act"], w)
        hard = (run["act"] != 0) & ~P.soft_set(run["act"], w) & (lo != hi)
        if (sat & (idx % n < S)).any() and (sat & (idx % n >= S)).any() and quad.any() and hard.any() \
                and np.linalg.cond(P.reduced_matrix(H, Cm, run["act"], w)) <= 1e7:
            return s, lo, hi, w, m, run
    raise AssertionError("no seed")


@pytest.mark.parametrize("S,C,K", [(4, 2, 5), (6, 3, 4)])
def test_gradients_match_finite_differences(S, C, K):
    """huber_grads for all fifteen inputs of box_qp_layer (Q, R symmetric; the weights and the caps included) against central
    differences of the Huber-QP solution along a random direction per input.  Every perturbed problem is solved by the
    iteration from the unperturbed act and must converge on it at once (margins >= 1e-3 against steps of 1e-6), asserted.  The
    bound is test_box_qp_soft_cpu.py's."""
    s, lo, hi, w, m, run0 = _fd_problem(S, C, K)
    Q, Rm, A, B, q, r, c = kgr.blocks_of(s)
    split = lambda v: P.split_states_controls(v, S, C, K)
    inp = dict(Q=Q, R=Rm, A=A, B=B, q=q, r=r, c=c)
    for name, v in (("lo", lo), ("hi", hi), ("soft", w), ("soft_max", m)):
        inp["x_" + name], inp["u_" + name] = split(v)
    act = run0["act"]
    run, (H, Cm, g, cc, lo2, hi2, w2, m2) = _solve(inp, s.rho, act, S)
    assert run["status"] == AS.CONVERGED and run["iters"] == 1 and np.array_equal(lo2, lo) and np.array_equal(m2, m)
    x, lam = run["x"], run["lam"]
    rng = np.random.default_rng(7)
    xbar, lambar = rng.standard_normal(len(x)), rng.standard_normal(len(lam))
    gr = P.grads(H, Cm, act, x, lam, xbar, lambar, S, C, K, w=w, m=m, lo=lo, hi=hi)
    sat = P.sat_set(act)
    assert gr["a"][sat].all() and not gr["lo"][sat].any() and not gr["hi"][sat].any() and not gr["w"][sat].any()
    assert np.array_equal(gr["m"] != 0, sat)
    L = lambda rr: float(xbar @ rr["x"] + lambar @ rr["lam"])
    lmag = float(np.abs(xbar) @ np.abs(x) + np.abs(lambar) @ np.abs(lam))
    for key in KEYS15:
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
        if key.endswith("_soft_max"):
            V = np.where(np.isfinite(inp[key]), V, 0.0)  # no cap stays no cap
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
    assert np.abs(gr["x_soft_max"]).max() > 0 and np.abs(gr["u_soft_max"]).max() > 0
    assert np.abs(gr["x_soft"]).max() + np.abs(gr["u_soft"]).max() > 0


# ---- the stage restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", [(4, 2, 9), (14, 7, 3)])
def test_stage_path_is_the_reduced_solve(S, C, K):
    """stage_solve in fp64 - a saturated variable free with g - s m in its row - against the dense solve of the reduced matrix on
    every act of a walked run; the fp64 restatement walks the reference's acts.  Bar: test_box_qp_polish_cpu.py's 1e-9."""
    p = R.huber_box(S, C, K)[0]
    assert any(P.sat_set(t["act"]).any() for t in p["run"]["trace"])
    for t in p["run"]["trace"]:
        xr, _, lr = P.reduced_solve(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], t["act"], p["w"], p["m"])
        x, lam, iters = P.reduced_stage_solve(p["s"], p["lo"], p["hi"], t["act"], np.float64, exit_tol=1e-30, w=p["w"], m=p["m"])
        ex = np.abs(x - xr).max() / max(1.0, np.abs(xr).max())
        el = np.abs(lam - lr).max() / max(1.0, np.abs(lr).max())
        print("pcg iterations", iters, "x", ex, "lam", el)
        assert ex <= 1e-9 and el <= 1e-9
    status, acts = AS.stage_iterate(p["s"], p["lo"], p["hi"], np.float64, 1e-6, p["w"], p["m"], exit_tol=1e-30)
    assert status == AS.CONVERGED and len(acts) == p["run"]["iters"]
    assert all(np.array_equal(a, t["act"]) for a, t in zip(acts, p["run"]["trace"]))


# ---- the cases of tests/test_gpu_box_qp_huber.py have seeds --------------------------------------------------------------------
COLD = [(S, C, K) for S, C in R.SHAPES for K in R.COLD_K]


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_walk_finds_an_fp64_seed(S, C, K):
    """Weight 100 and cap 1 on every state: a seed below WALK_SEEDS whose cold run converges within WALK_SOLVES solves with
    every margin >= MARGIN and cond <= COND_CAP on a final act with a saturated lo != hi variable - and a soft quadratic-active
    one, except in the four cells of MAY_BE_EMPTY, which are too small to promise both and may even have no seed: that is then
    said by name."""
    ps = R.huber_box(S, C, K)
    if not ps:
        assert (S, C, K) in R.MAY_BE_EMPTY, "no seed at %d/%d/%d" % (S, C, K)
        pytest.fail("%d/%d/%d: the walk finds no seed below %d with a saturated variable (a cell that may be empty)"
                    % (S, C, K, AS.WALK_SEEDS))
    p = ps[0]
    run = p["run"]
    sat, quad = R.final_kinds(run, p["w"], p["lo"], p["hi"])
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "cond", AS.max_cond(run, p["H"], p["Cm"], p["w"]),
          "saturated", sat, "quadratic", quad)
    assert p["seed"] < AS.WALK_SEEDS and sat and (quad or (S, C, K) in R.MAY_BE_EMPTY)
    assert AS.walk_ok(run, p["H"], p["Cm"], p["w"])
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], run["x"], run["y"], run["lam"], p["w"], p["m"])
    assert max(kk.values()) <= 1e-9, kk


@pytest.mark.parametrize("S,C,K", R.F32_CASES, ids=["%d-%d-%d" % c for c in R.F32_CASES])
def test_walk_finds_an_fp32_seed(S, C, K):
    """The fp32 restatement, the products w (x - b) formed in float32, walks the reference's acts - and again with every PCG
    stopped one iteration sooner."""
    ps = R.huber_box(S, C, K, f32=True)
    assert ps and ps[0]["seed"] < AS.WALK_SEEDS
    print("seed", ps[0]["seed"], "solves", ps[0]["run"]["iters"])
    assert AS.f32_ok(ps[0]) and P.sat_set(ps[0]["run"]["act"]).any()


def test_the_other_gpu_cases_exist():
    """The mixed cases (a weight and a cap per variable, on states and controls; the final act holds a saturated control), the
    long horizon (CONVERGED, a saturated variable past knot 8192) and the large weight with a small cap on the double
    integrator."""
    for S, C, K in [(6, 3, 9), (14, 7, 3)]:
        p = R.mixed_box(S, C, K)
        assert p is not None
        w, m, run = p["w"], p["m"], p["run"]
        ctl = np.arange(p["s"].N) % (S + C) >= S
        assert (np.isfinite(m) & (w > 0)).any() and (np.isinf(m) & (w > 0)).any() and np.all((m >= 0.1) & ((m <= 10.0) | np.isinf(m)))
        assert (P.sat_set(run["act"]) & ctl & (p["lo"] != p["hi"])).any()
        kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], run["x"], run["y"], run["lam"], w, m)
        print((S, C, K), "mixed seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), kk)
        assert max(kk.values()) <= 1e-9
    p = R.huber_long()
    run = p["run"]
    print("long: solves", run["iters"], "margin", AS.min_margin(run))
    assert run["status"] == AS.CONVERGED and (np.flatnonzero(P.sat_set(run["act"])) // 3 >= 8192).any()
    s, H, Cm, g, c, lo, hi, w = SR.double_integrator_soft(weight=1e6)
    run = AS.iterate(H, Cm, g, c, lo, hi, 2, w, np.where(w > 0, 0.1, np.inf))
    print("double integrator, w = 1e6, cap 0.1: solves", run["iters"], "violation", np.abs(run["x"] - np.clip(run["x"], lo, hi)).max())
    assert run["status"] == AS.CONVERGED


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gato_hip.h")).read()
    from gato_python_amd import _lib
    L = _lib.lib()
    for name in ("gato_box_qp_pdas_huber", "gato_box_qp_huber_grad"):
        assert re.search(r"int\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name)
