"""The reference of the augmented-Lagrangian outer loop (tests/box_qp_alm_ref.py) against SLSQP and
against itself, the problems no earlier method solves, the pinned seed of every case of tests/test_gpu_box_qp_alm.py against the
seed rule, and the argument checks of box_qp(method="alm") that need no device."""
import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_alm_ref as A
import box_qp_polish_ref as P
import box_qp_ref as ref

SLSQP_CASES = [(2, 1, 9), (4, 2, 3), (6, 3, 9)]


@pytest.mark.parametrize("S,C,K", SLSQP_CASES, ids=["%d-%d-%d" % c for c in SLSQP_CASES])
def test_exact_point_is_the_slsqp_minimum_of_the_hard_qp(S, C, K):
    """scipy's SLSQP on the hard QP (equalities C x = c, the box off x_0 as bounds) from x = 0 reaches x* within 1e-6."""
    from scipy.optimize import minimize
    p = A.alm_box(S, C, K)
    H, Cm, g, c = (p[k] for k in ("H", "Cm", "g", "c"))
    lo, hi = A.hard_box(p)
    bounds = [(None if not np.isfinite(l) else l, None if not np.isfinite(h) else h) for l, h in zip(lo, hi)]
    out = minimize(lambda x: (ref.objective(H, g, x), H @ x - g), np.zeros(len(g)), jac=True, method="SLSQP", bounds=bounds,
                   constraints=[dict(type="eq", fun=lambda x: Cm @ x - c, jac=lambda x: Cm)], options=dict(ftol=1e-16, maxiter=2000))
    err = np.abs(out.x - p["exact"]["x"]).max()
    print("seed", p["seed"], out.message, out.nit, "x err", err)
    assert err <= 1e-6, err


def stationarity(p, run):
    """|H x - g + C^T lam + y|_inf of a run's point: the hard QP's stationarity, y being the multipliers and the soft forces."""
    return float(np.abs(p["H"] @ run["x"] - p["g"] + p["Cm"].T @ run["lam"] + run["y"]).max())


def stationarity_bar(p, run):
    """The bar on the stationarity of an accepted reference point: the row-wise residual bound of a backward-stable dense solve of
    the last inner system, 64 N eps max_i (|H| |x| + w' |x| + w' |b'| + |C^T| |lam| + |g|)_i with w' and b' the last step's inner
    weights and shifted bounds on its soft-active set (the 64 of box_qp_linesearch_ref.SLACK), and never more than 1e-7, what the
    device's points are held to."""
    st = run["steps"][-1]
    x, lam, act = np.abs(run["x"]), np.abs(run["lam"]), st["act"]
    on = act != 0
    wb = np.where(on, st["w2"], 0.0)
    b = np.abs(np.where(act > 0, st["hi2"], np.where(act < 0, st["lo2"], 0.0)))
    scale = float((np.abs(p["H"]) @ x + wb * x + wb * np.where(on, b, 0.0) + np.abs(p["Cm"]).T @ lam + np.abs(p["g"])).max())
    return min(1e-7, 64 * len(x) * np.finfo(np.float64).eps * scale)


@pytest.mark.parametrize("name", A.NAMED)
def test_named_problems_converge(name):
    """The three failures of today - both double integrators with a hard velocity bound, 6/3/20 seed 2 - are feasible and end
    CONVERGED at a KKT point of the hard QP: stationarity <= 1e-9, equality <= 1e-11, bound violation within the acceptance bar;
    the violation never rises once the weight has stopped growing; and the hard active-set iteration does not converge on them."""
    p = A.named(name)
    assert A.feasible(p)
    run = A.run_alm(p, max_pdas_iters=60)
    lo, hi = A.hard_box(p)
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], lo, hi, run["x"], run["y"], run["lam"])
    print(name, "outer", run["outer"], "solves", run["iters"], "weight", run["weight"], kk)
    assert run["status"] == A.CONVERGED and run["outer"] <= 9 and run["iters"] <= 31
    assert kk["stat"] <= 1e-9 and kk["eq"] <= 1e-11 and kk["bound"] <= A.bar_of(run, 1e-6)
    assert A.run_alm(p)["iters"] == run["iters"]                          # the default inner cap of 30 solves is not met
    last_growth = max([i for i, st in enumerate(run["steps"]) if st["dec"] == A.GROW], default=-1)
    vs = [st["v"] for st in run["steps"]][last_growth + 1:]
    assert all(b <= a for a, b in zip(vs, vs[1:])), vs
    hard = AS.iterate(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], p["s"].S)
    assert hard["status"] != AS.CONVERGED


def test_infeasible_box_stalls_at_a_constant_violation():
    """2/1/3 seed 1 (linprog: infeasible) at the default settings: MAX_ITERS after 50 steps with the weight at its maximum, the
    violation constant to 1e-9 over the last ten steps.  In exact arithmetic the stalled violation repeats: on the final act
    the multiplier's bounded part converges at the rate 1 / (1 + w m), m = O(1).  The run is taken with the refined dense solve
    (box_qp_alm_ref.refined_solve): the unrefined one of iterate_ls carries an absolute error of about eps cond |b - mu / w|,
    which grows with the step count as mu does, and its violation drifts by a constant -1.30e-9 per step at w = 1e8 (1.17e-8
    over ten steps; -1.2e-10 per step at 1e7, -4.8e-9 at 1e9; x_0 off its pinned value by 1e-8) - rounding, which the refined
    run (0.08766758516910628 on every step, as in 40-digit arithmetic) does not show.  The unrefined run stalls at the same
    violation to well within the solver's eps."""
    p = A.state_problem(2, 1, 3, 1)
    assert not A.feasible(p)
    run, plain = A.run_alm(p, inner=A.refined_inner), A.run_alm(p)
    vs, vp = ([st["v"] for st in r["steps"]] for r in (run, plain))
    print("outer", run["outer"], "weight", run["weight"], "v", vs[-1], "spread", max(vs[-10:]) - min(vs[-10:]),
          "unrefined: v", vp[-1], "spread", max(vp[-10:]) - min(vp[-10:]))
    for r, v in ((run, vs), (plain, vp)):
        assert r["status"] == A.MAX_ITERS and r["outer"] == A.OUTER and r["steps"][-1]["dec"] == A.LAST
        assert r["weight"] >= A.WEIGHT_MAX and v[-1] > 1e-3
    assert max(vs[-10:]) - min(vs[-10:]) <= 1e-9
    assert abs(vp[-1] - vs[-1]) <= 1e-6
    # the unrefined run's own drift: its right-hand side holds w (b - mu / w) to eps relative, a perturbation of the stationarity
    # rows that moves x by at most that over the smallest eigenvalue of H, per step
    st = plain["steps"][-1]
    shifted = max(float(np.abs(t[np.isfinite(t)]).max()) for t in (st["lo2"], st["hi2"]))
    drift = np.finfo(np.float64).eps * st["w"] * shifted / float(np.linalg.eigvalsh(p["H"]).min())
    print("unrefined drift per step at most", drift, "measured", vp[-2] - vp[-1])
    assert max(vp[-10:]) - min(vp[-10:]) <= 10 * drift


REFINED_CASES = [(2, 1, 9), (6, 3, 9), (14, 7, 3)]


def test_refined_inner_is_the_reference_where_the_multiplier_stays_bounded():
    """On feasible problems - the three named ones and three pinned cells - the run over the refined solve has the outer steps,
    solves, weights and acts of the run over iterate_ls, and its point within 1e-9."""
    for p in [A.named(n) for n in A.NAMED] + [A.alm_box(*c) for c in REFINED_CASES]:
        a, b = A.run_alm(p), A.run_alm(p, inner=A.refined_inner)
        assert (a["status"], a["outer"], a["iters"], a["weight"]) == (b["status"], b["outer"], b["iters"], b["weight"])
        for s, t in zip(a["steps"], b["steps"]):
            assert (s["solves"], s["w"], s["dec"]) == (t["solves"], t["w"], t["dec"]) and np.array_equal(s["act"], t["act"])
        assert np.abs(a["x"] - b["x"]).max() <= 1e-9 and np.abs(a["lam"] - b["lam"]).max() <= 1e-9 * max(1.0, np.abs(a["lam"]).max())


def test_step_update_is_the_loop():
    """step_update on the inner points of a reference run gives the run's own decisions, weights and next inner inputs."""
    p = A.alm_box(6, 3, 9)
    run, S = p["run"], p["s"].S
    mu, v_prev = np.zeros(p["s"].N), np.inf
    for st, nxt in zip(run["steps"], run["steps"][1:] + [None]):
        r = st["run"]
        got = A.step_update(r["x"], r["y"], p["lo"], p["hi"], S, None, mu, st["w"], v_prev, 1e-6, 1e-6)
        assert got["v"] == st["v"] and got["dec"] == st["dec"]
        if nxt is not None:
            assert got["w"] == nxt["w"]
            assert all(np.array_equal(got[k], nxt[k]) for k in ("lo2", "hi2", "w2"))
        mu, v_prev = got["mu"], got["v"]


CELLS = [c + (False,) for c in A.F64_CASES] + [c + (True,) for c in A.F32_CASES]


@pytest.mark.parametrize("S,C,K,f32", CELLS, ids=["%d-%d-%d-%s" % (S, C, K, "f32" if f else "f64") for S, C, K, f in CELLS])
def test_pinned_seed_meets_the_seed_rule(S, C, K, f32):
    """Every GPU cell has a pinned seed among the first 20 whose reference run is feasible (also with every bound moved inward by
    1e-3), CONVERGED within 15 outer steps and 60 solves, has a state bound active at x* with |y| >= 1e-3, and keeps the margins
    of the rule but the one PINNED drops for the cell; fp32: the fp32 stage restatement follows it, also with every PCG stopped
    one iteration sooner.  The hard active-set iteration does not converge on it."""
    p = A.alm_box(S, C, K, f32)
    assert p is not None and 0 <= p["seed"] < AS.WALK_SEEDS
    ck = p["checks"]
    print("seed", p["seed"], p["form"], "drops", p["drop"], ck, "outer", p["run"]["outer"], "solves", [st["solves"] for st in p["run"]["steps"]],
          "weight", p["run"]["weight"])
    assert p["drop"] in A.DROPS and ck["converged"] and ck["feasible"] and ck["active_state"]
    assert A.meets(p, p["drop"], f32)
    if p["drop"] == "slack":
        assert not A.f32_follows(p)                                      # a margin is dropped because the seed needs it dropped
    elif p["drop"] is not None:
        assert not ck[p["drop"]]
    own = float(np.abs(p["run"]["x"] - p["exact"]["x"]).max())
    print("|x_ref(eps) - x*|", own)
    assert 0 < own <= 10 * A.bar_of(p["run"], p["eps"])
    stat, bar = stationarity(p, p["run"]), stationarity_bar(p, p["run"])
    print("stationarity", stat, "bar", bar)
    assert stat <= bar and float(np.abs(p["Cm"] @ p["run"]["x"] - p["c"]).max()) <= bar


@pytest.mark.parametrize("S,C,K", [(6, 3, 9), (14, 7, 3)], ids=["6-3-9", "14-7-3"])
def test_hard_controls_with_soft_states_reference(S, C, K):
    """The mixed problems of the GPU test - the pinned problem with weight 100 and cap 1 on every state: the accepted point is
    stationary with y the multipliers on the controls and the capped forces of the unshifted bounds on the states, the controls
    hold their bounds to the bar, and no state has a multiplier."""
    p = dict(A.alm_box(S, C, K))
    n, N = S + C, p["s"].N
    state = (np.arange(N) % n) < S
    p.update(w=np.where(state, 100.0, 0.0), m=np.where(state, 1.0, np.inf))
    run = A.run_alm(p)
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], run["x"], run["y"], run["lam"], p["w"], p["m"])
    stat, bar = stationarity(p, run), stationarity_bar(p, run)
    print("outer", run["outer"], "solves", run["iters"], kk, "stationarity", stat, "bar", bar)
    assert run["status"] == A.CONVERGED
    assert stat <= bar and kk["eq"] <= bar and kk["force"] <= bar and kk["bound"] <= A.bar_of(run, 1e-6)
    assert not A.alm_set(p["lo"], p["hi"], S, p["w"])[state].any() and not run["mu"][state].any()


@pytest.mark.parametrize("S,C", A.SHAPES, ids=["%d-%d" % c for c in A.SHAPES])
def test_hard_iteration_fails_on_a_pinned_case_of_every_shape(S, C):
    """Per shape at least one pinned fp64 problem on which box_qp_active_ref.iterate without weights does not converge."""
    fails = []
    for K in (2, 3, 9):
        p = A.alm_box(S, C, K)
        hard = AS.iterate(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], S)
        fails.append(hard["status"] != AS.CONVERGED)
    print(fails)
    assert any(fails)


def test_default_weight_caps_are_the_references():
    """alm_weight_max=None of Solver.box_qp_alm is the cap the reference runs were walked and pinned at, per dtype."""
    from gato_python_amd import solver
    assert solver.ALM_WEIGHT_MAX == {np.dtype(np.float64): A.WEIGHT_MAX, np.dtype(np.float32): A.F32_WEIGHT_MAX}
    assert all(A.alm_box(*c, True)["alm"] == dict(alm_weight_max=A.F32_WEIGHT_MAX) for c in A.F32_CASES)


# ---- the argument checks that need no device -----------------------------------------------------------------------------------
def test_alm_refusals():
    import torch
    import gato_python_amd
    from gato_python_amd.solver import Solver
    S, C, K = 2, 1, 3
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    blocks = (z(K, S, S), z(K - 1, C, C), z(K - 1, S, S), z(K - 1, S, C), z(K, S), z(K - 1, C), z(K, S))
    call = lambda **kw: gato_python_amd.box_qp(*blocks, -1.0, 1.0, -1.0, 1.0, rho=1e-3, exit_tol=1e-8, max_iters=10, **kw)
    with pytest.raises(ValueError, match="method must be 'admm', 'pdas' or 'alm'"):
        call(method="al")
    for kw, text in ((dict(admm_rho=1.0), "admm_rho is not read by method='alm'"), (dict(sigma=1e-3, max_admm_iters=10), "sigma, max_admm_iters are not read"),
                     (dict(polish_iters=3), "polish_iters is not read"), (dict(line_search=True), "line_search is implied"),
                     (dict(line_search=False), "line_search is implied"), (dict(alm_weight=-1.0), "finite alm_weight > 0"),
                     (dict(alm_weight=float("inf")), "finite alm_weight > 0"), (dict(alm_growth=1.0), "alm_growth > 1"),
                     (dict(alm_weight_max=10.0), "alm_weight_max >= alm_weight"), (dict(max_alm_iters=0), "at least 1"),
                     (dict(max_pdas_iters=0), "at least 1"), (dict(u_soft_max=1.0), "give x_soft or u_soft too"),
                     (dict(polish=True, u_soft=1.0), "hard bounds only")):
        with pytest.raises(ValueError, match=text):
            call(method="alm", **kw)
    for method in ("admm", "pdas"):
        with pytest.raises(ValueError, match="need method='alm'"):
            call(method=method, max_alm_iters=5)
    with pytest.raises(ValueError, match="soft_cap needs soft_weight"):
        Solver.box_qp_alm(None, *(None,) * 6, rho=1e-3, exit_tol=1e-8, max_iters=10, soft_cap=z(3))


def test_c_entries_are_declared_and_exported():
    import os
    from gato_python_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gato_hip.h")).read()
    L = _lib.lib()
    for name in ("gato_box_qp_alm", "gato_box_qp_alm_update"):
        assert ("int %s(" % name) in hdr and name in _lib.SYMBOLS and hasattr(L, name)
