"""The reference of the exact line search (tests/box_qp_linesearch_ref.py) against itself and SLSQP,
the seeds of every case of tests/test_gpu_box_qp_linesearch.py, and the argument checks of the Python entries that need no
device."""
import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_linesearch_ref as L
import box_qp_polish_ref as P


def objective(p, x):
    return AS.penalised_objective(p["H"], p["g"], p["lo"], p["hi"], x, L.off_x0(p["w"], p["s"].S), p.get("m"))[0]


@pytest.mark.parametrize("form", (L.CAPPED, L.UNCAPPED), ids=("capped", "uncapped"))
def test_objective_never_increases(form):
    """phi along the iterates xc of the reference run: every step is an exact minimisation along a descent direction.  The
    iterates are feasible (C x = c), so phi is the whole merit function."""
    for S, C, K in ((2, 1, 9), (6, 3, 9), (14, 7, 9)):
        p = L.ls_box(S, C, K, form)[0]
        xs = [t["xp"] if t["xc"] is None or t["alpha"] == 1.0 else t["xc"] + t["alpha"] * (t["xp"] - t["xc"])
              for t in p["run"]["trace"][:-1]] + [p["run"]["x"]]
        phi = np.array([objective(p, x) for x in xs])
        print(S, C, K, "seed", p["seed"], phi.tolist())
        assert len(phi) >= 3 and np.all(np.diff(phi) <= 1e-9 * np.abs(phi).max())
        assert max(np.abs(p["Cm"] @ x - p["c"]).max() for x in xs) < 1e-8


@pytest.mark.parametrize("S,C,K", [(2, 1, 5), (4, 2, 3)], ids=["2-1-5", "4-2-3"])
@pytest.mark.parametrize("form", (L.CAPPED, L.UNCAPPED), ids=("capped", "uncapped"))
def test_converged_point_is_the_minimiser(S, C, K, form):
    """The converged x against SLSQP on the penalised objective under C x = c, 1e-6: the bar and the method of the soft tests."""
    from scipy.optimize import minimize
    p = next(q for q in (L.ls_problem(S, C, K, seed, *form, undamped=False) for seed in range(AS.WALK_SEEDS))
             if q["run"]["status"] == AS.CONVERGED and L.damped_on_the_way(q["run"]))
    H, Cm, g, c, lo, hi, w, m = (p.get(k) for k in ("H", "Cm", "g", "c", "lo", "hi", "w", "m"))
    w = L.off_x0(w, S)
    scale = 1.0 / w.max()                            # SLSQP's tolerances are absolute: the objective at the scale of the weights
    fun = lambda x: tuple(scale * v for v in AS.penalised_objective(H, g, lo, hi, x, w, m))
    x0 = np.linalg.lstsq(Cm, c, rcond=None)[0]
    got = minimize(fun, x0, jac=True, method="SLSQP", constraints=[dict(type="eq", fun=lambda x: Cm @ x - c, jac=lambda x: Cm)],
                   options=dict(ftol=1e-18, maxiter=2000))
    err = np.abs(got.x - p["run"]["x"]).max()
    print("seed", p["seed"], "solves", p["run"]["iters"], "err", err, got.message)
    assert err < 1e-6


def test_full_steps_are_the_undamped_iteration():
    """With alpha forced to 1, iterate_ls is box_qp_active_ref.iterate exactly."""
    for form in (L.CAPPED, L.UNCAPPED, (10.0, None)):
        p = L.ls_problem(6, 3, 9, 0, *form)
        H, Cm, g, c, lo, hi, w, m = (p.get(k) for k in ("H", "Cm", "g", "c", "lo", "hi", "w", "m"))
        got, want = L.iterate_ls(H, Cm, g, c, lo, hi, 6, w, m, force_alpha=1.0), p["undamped"]
        assert (got["status"], got["iters"]) == (want["status"], want["iters"])
        for k in ("act", "x", "z", "y", "lam"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        for a, b in zip(got["trace"], want["trace"]):
            assert np.array_equal(a["act"], b["act"]) and a["changed"] == b["changed"] and a["margin"] == b["margin"]


def test_exact_alpha_is_the_root():
    p = L.ls_box(6, 3, 9)[0]
    w = L.off_x0(p["w"], 6)
    seen = 0
    for t in p["run"]["trace"]:
        e = t["ls"]
        if e is None or e["alpha"] == 1.0:
            continue
        d = t["xp"] - t["xc"]
        f = lambda a: L.slope(p["H"], p["g"], p["lo"], p["hi"], w, p["m"], t["xc"], d, a)
        assert e["s0"] < 0 < e["s1"] and e["piece"][0] <= e["alpha"] <= e["piece"][1]
        assert abs(f(e["alpha"])) <= 1e-9 * max(-e["s0"], e["s1"])
        grid = np.array([f(a) for a in np.linspace(0, 1, 201)])
        assert np.all(np.diff(grid) >= -1e-9 * np.abs(grid).max())          # non-decreasing
        seen += 1
    assert seen >= 3


# ---- every GPU case has a seed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CAPPED_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_capped_cases_have_seeds(case):
    ps = L.ls_box(*case, L.CAPPED)
    assert ps and L.ls_ok(ps[0]) and ps[0]["undamped"]["status"] != AS.CONVERGED
    for dt in (np.float64, np.float32):
        for form in (L.CAPPED, L.UNCAPPED):
            batch = L.kernel_batch(*case, form, dt)
            assert batch and [0.0 < c[3]["alpha"] < 1.0 for c in batch] == [True, False, True]


@pytest.mark.parametrize("case", L.UNCAPPED_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_uncapped_cases_have_seeds(case):
    ps = L.ls_box(*case, L.UNCAPPED)
    assert ps and AS.max_cond(ps[0]["run"], ps[0]["H"], ps[0]["Cm"], ps[0]["w"]) * np.finfo(np.float64).eps < AS.MARGIN


@pytest.mark.parametrize("case", L.F32_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_fp32_cases_have_seeds(case):
    assert L.ls_box(*case, L.CAPPED, f32=True)


def test_batch_warm_and_layer_cases_have_seeds():
    found = L.ls_box(6, 3, 9, L.CAPPED, count=4)
    assert len(found) == 4 and len({p["run"]["iters"] for p in found}) >= 2
    full = L.full_step_box(6, 3, 9)
    assert full and set(full["run"]["alpha"][:-1]) == {1.0}
    assert all(L.ls_box(*c, L.CAPPED) for c in L.LAYER_CASES)


# ---- the argument checks that need no device ---------------------------------------------------------------------------------
def test_line_search_refusals():
    import torch
    import gato_python_amd
    from gato_python_amd.solver import Solver
    S, C, K = 2, 1, 3
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    blocks = (z(K, S, S), z(K - 1, C, C), z(K - 1, S, S), z(K - 1, S, C), z(K, S), z(K - 1, C), z(K, S))
    kw = dict(rho=1e-3, exit_tol=1e-8, max_iters=10, line_search=True)
    for entry in (gato_python_amd.box_qp, gato_python_amd.box_qp_layer):
        with pytest.raises(ValueError, match="line_search=True needs method='pdas'"):
            entry(*blocks, -1.0, 1.0, -1.0, 1.0, x_soft=1.0, u_soft=1.0, **kw)                       # method="admm"
        with pytest.raises(ValueError, match="line_search=True takes soft bounds only"):
            entry(*blocks, -1.0, 1.0, -1.0, 1.0, method="pdas", **kw)                                # no weights
    with pytest.raises(ValueError, match="line_search=True needs method='pdas' without polish"):
        gato_python_amd.box_qp(*blocks, -1.0, 1.0, -1.0, 1.0, method="pdas", polish=True, **kw)
    with pytest.raises(ValueError, match="line_search=True needs soft_weight"):
        Solver.box_qp_pdas(None, *(None,) * 6, rho=1e-3, exit_tol=1e-8, max_iters=10, line_search=True)
