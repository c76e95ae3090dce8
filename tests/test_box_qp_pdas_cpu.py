"""The reference of the primal-dual active-set iteration (tests/box_qp_pdas_ref.py) checked on the CPU: the seed walks find a
problem for every case of tests/test_gpu_box_qp_pdas.py, the converged points are KKT points of their QPs, the constructed
problems end on their known active set, and the double integrator with velocity bounds - the documented failure - does not
converge."""
import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_pdas_ref as D
import box_qp_polish_ref as P
import box_qp_ref as ref


def kkt_ok(p, run, bar=1e-9):
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], run["x"], run["y"], run["lam"])
    assert max(kk.values()) <= bar, kk


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_walk_finds_control_box_seeds(shape):
    S, C = shape
    for K in D.COLD_K:
        ps = D.control_box(S, C, K)
        assert len(ps) == 1, (S, C, K)
        run = ps[0]["run"]
        print((S, C, K), "seed", ps[0]["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "active", int((run["act"] != 0).sum()))
        assert run["status"] == AS.CONVERGED and AS.min_margin(run) >= AS.MARGIN and (run["act"] != 0).any()
        kkt_ok(ps[0], run)


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_walk_finds_f32_seeds(shape):
    S, C = shape
    ps = D.control_box(S, C, 9, f32=True)
    assert len(ps) == 1
    print(shape, "seed", ps[0]["seed"], "solves", ps[0]["run"]["iters"])


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_constructed_problems_end_on_their_active_set(shape):
    S, C = shape
    for K in (2,) + D.CONSTRUCTED_K:
        ps = D.constructed_cold(S, C, K)
        assert len(ps) == 1, (S, C, K)
        p, run = ps[0], ps[0]["run"]
        print((S, C, K), "seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run))
        assert run["status"] == AS.CONVERGED and np.array_equal(run["act"], p["act"])
        assert np.abs(run["x"] - p["x"]).max() <= 1e-9 * max(1.0, np.abs(p["x"]).max())
        kkt_ok(p, run)


def test_every_constructed_problem_of_the_polish_sweep_converges():
    """Not only the walked ones: on each first constructed problem of the polish sweep the cold run ends on p["act"] and p["x"]."""
    for S, C in D.SHAPES:
        for K in P.SWEEP_SHORT_K:
            p = P.constructed(S, C, K)[0]
            run = AS.iterate(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], S)
            assert run["status"] == AS.CONVERGED and np.array_equal(run["act"], p["act"]), (S, C, K, run["status"], run["iters"])
            assert np.abs(run["x"] - p["x"]).max() <= 1e-9 * max(1.0, np.abs(p["x"]).max())


def test_batch_and_named_cases():
    S, C, K, B = D.BATCH
    ps = D.control_box(S, C, K, count=B)
    assert len(ps) == B
    iters = [p["run"]["iters"] for p in ps]
    print("batch solves", iters)
    assert len(set(iters)) >= 2                   # systems that need different numbers of solves
    for name in ("pendulum", "14_7_50"):
        s, H, Cm, g, c, lo, hi = D.named(name)
        run = AS.iterate(H, Cm, g, c, lo, hi, s.S)
        print(name, "solves", run["iters"], "margin", AS.min_margin(run))
        assert run["status"] == AS.CONVERGED
        kkt_ok(dict(H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi), run)
    act, *_ = P.exact_active("14_7_50")
    assert np.array_equal(run["act"], act)       # the active set ADMM reaches


def test_walk_finds_the_long_horizon_seed():
    """2/1/8197 through the sparse path: a seed whose run converges with margin and has active controls past knot 8192."""
    S, C, K = D.LONG
    ps = D.control_box(S, C, K, sparse=True)
    assert len(ps) == 1
    run = ps[0]["run"]
    print("seed", ps[0]["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "active", int((run["act"] != 0).sum()))
    assert (np.flatnonzero(run["act"]) // (S + C) >= 8192).any()
    kkt_ok(ps[0], run)


def test_polish_iterated_closes_6_3_20_from_50_admm_steps():
    """The facts behind box_qp(polish=True, polish_iters=10) on problem("6_3_20") from 50 x-steps: one polish is rejected,
    the iteration from the same active set converges."""
    s, lo, hi, arho = P.problem("6_3_20")
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, admm_rho=arho, eps_abs=1e-6, eps_rel=1e-6, max_admm_iters=50)
    assert out["status"] == ref.MAX_ITERS
    act = P.active_set(out["z"], out["y"], lo, hi, s.S)
    assert P.polish(H, Cm, g, c, lo, hi, None, None, s.S, act=act)["decision"] == P.REJECTED
    run = AS.iterate(H, Cm, g, c, lo, hi, s.S, act0=act, max_pdas_iters=10)
    print("solves", run["iters"], "margin", AS.min_margin(run))
    assert run["status"] == AS.CONVERGED and 1 < run["iters"] <= 10
    kkt_ok(dict(H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi), run)


def test_velocity_bounded_double_integrator_does_not_converge():
    s, lo, hi, _ = P.problem("double_integrator")                   # v_max = 0.57
    H, Cm, g, c = ref.parts(s)
    run = AS.iterate(H, Cm, g, c, lo, hi, s.S)
    print("status", run["status"], "solves", run["iters"])
    assert run["status"] in (AS.MAX_ITERS, AS.NONFINITE)
    free = ref.double_integrator(K=20, u_max=0.5, v_max=None)       # the control-only box of the same system converges
    Hf, Cf, gf, cf = ref.parts(free[0])
    assert AS.iterate(Hf, Cf, gf, cf, free[1], free[2], 2)["status"] == AS.CONVERGED


def test_rule_edges():
    """next_act on hand-made values: ties stay as they are read (x == hi is inside, y == 0 releases), lo == hi is always
    lower, x_0 always free, an infinite bound never active."""
    lo = np.array([-1, -1, -1.0, -1, -1, -1, 0.5, -np.inf, -1, -1])
    hi = np.array([1, 1, 1.0, 1, 1, 1, 0.5, np.inf, np.inf, 1])
    act = np.array([0, 0, 0, 0, 1, 1, 0, 0, 0, -1], np.int8)
    x = np.array([9, 9, 1.5, 1.0, 1, 1, 0.5, 1e30, 1e30, -1.0])
    y = np.array([0, 0, 0.0, 0.0, 2, 0, 7.0, 0, 0, -3.0])
    want = np.array([0, 0, 1, 0, 1, 0, -1, 0, 0, -1], np.int8)
    assert np.array_equal(AS.next_act(act, x, y, lo, hi, 2), want)
