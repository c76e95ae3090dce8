"""Hard state bounds by the augmented-Lagrangian outer loop on the device (gato_box_qp_alm, gato_box_qp_alm_update,
Solver.box_qp_alm, Solver.box_qp_alm_update, box_qp(method="alm")) against the numpy reference of
tests/box_qp_alm_ref.py (tests/test_box_qp_alm_cpu.py asserts that every pinned seed meets the seed rule).  The kernels alone: v
and |x|_inf bit-equal to numpy's maxima, mu bit-equal to y, the decision, the weight and the shifted bounds equal to the reference
evaluated in the dtype.  End to end: the reference's outer steps, weights and per-step solves, the KKT residuals of the hard QP,
the distance to x* within ten times the reference's own, the same bits on a repeat."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_alm_ref as A                        # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import (CAP, F64, alm_bits, alm_cold_case, alm_point as point, alm_run, check_alm_run as check_run,  # noqa: E402
                           check_alm_steps as check_steps, dev_inputs, math_inputs, sentinels, solver, untouched)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


# ---- 1. the two kernels alone --------------------------------------------------------------------------------------------------
def update_inputs(S, C, K, dt, kind, seed, weights):
    """A synthetic inner point of one system: a box with +-inf entries, an equality and bounds on x_0, user weights on a third
    of the variables (weights; the kernels read no caps), and x placed for the decision `kind`: "accept" (every ALM variable within its bounds but
    one, 1e-9 outside), "grow" (violations up to 0.1, v_prev = 0.2) or "keep" (the same, v_prev = 1)."""
    rng = np.random.default_rng(seed)
    n, N = S + C, (S + C) * K - C
    mid, half = rng.standard_normal(N), rng.uniform(0.1, 1.0, N)
    lo, hi = mid - half, mid + half
    pick = rng.integers(0, 6, N)
    lo[pick == 0], hi[pick == 1] = -np.inf, np.inf
    lo[pick == 2], hi[pick == 2] = -np.inf, np.inf
    lo[S + 1] = hi[S + 1] = mid[S + 1]                                    # an equality, kept an ALM variable below
    w = None
    if weights:
        w = np.where(rng.integers(0, 3, N) == 0, rng.uniform(1.0, 100.0, N), 0.0)
        w[S + 1] = 0.0                                                    # the equality stays an ALM variable
    lo, hi = (np.asarray(t, dt).astype(np.float64) for t in (lo, hi))
    av = A.alm_set(lo, hi, S, w)
    x = np.clip(mid + 0.5 * half * rng.uniform(-1, 1, N), np.where(np.isfinite(lo), lo, -9.0), np.where(np.isfinite(hi), hi, 9.0))
    if kind == "accept":
        j = int(np.flatnonzero(av & np.isfinite(hi))[0])
        x[j] = hi[j] + 1e-9
        v_prev = np.inf
    else:
        out = av & (rng.integers(0, 2, N) == 0)
        x = np.where(out & np.isfinite(hi), hi + rng.uniform(0, 0.1, N), x)
        x[S + 1] = hi[S + 1] + 0.07                                       # at least the equality is violated
        v_prev = 0.2 if kind == "grow" else 1.0
    x[:S] = 10.0 + np.arange(S)                                          # x_0 outside every bound: not an ALM variable, but in |x|_inf
    y, mu, lam = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(S * K)
    r32 = lambda t: np.asarray(t, dt).astype(np.float64)
    return dict(S=S, lo=lo, hi=hi, w=None if w is None else r32(w), x=r32(x), y=r32(y), mu=r32(mu),
                lam=r32(lam), wk=100.0 if kind != "keep" else 1e3, v_prev=v_prev, kind=kind)


def check_update(sol, cases, dt, knots=None):
    """Solver.box_qp_alm_update on the systems `cases`, lo2 at an unaligned address.  knots: only these knots are compared."""
    B, N, S = len(cases), sol.N, sol.S
    eps = 1e-6 if dt == np.float64 else 1e-4
    cat = lambda k: sol.to_device(np.concatenate([c[k] for c in cases]))
    buf = sol.new(B * N + 1).fill_(float("nan"))
    wm = {}
    if cases[0]["w"] is not None:
        wm = dict(soft_weight=cat("w"))
    mu = cat("mu")
    out = sol.box_qp_alm_update(cat("x"), cat("y"), cat("lam"), mu, torch.tensor([c["wk"] for c in cases], dtype=torch.float64, device="cuda"),
                                torch.tensor([c["v_prev"] for c in cases], dtype=torch.float64, device="cuda"), cat("lo"), cat("hi"),
                                eps_abs=eps, eps_rel=eps, alm_weight_max=1e8, lo2=buf[1:], **wm)
    torch.cuda.synchronize()
    assert torch.isnan(buf[0])
    sel = slice(None) if knots is None else np.concatenate([np.arange(k * (S + sol.C), min((k + 1) * (S + sol.C), N)) for k in knots])
    for b, c in enumerate(cases):
        want = A.step_update(c["x"], c["y"], c["lo"], c["hi"], S, c["w"], c["mu"], c["wk"], c["v_prev"], eps, eps, dtype=dt)
        got = {k: t.cpu().numpy().reshape(B, -1)[b] for k, t in out.items()}
        print("system", b, c["kind"], "v", got["v"][0], "xinf", got["xinf"][0], "dec", got["dec"][0], "want", want["dec"])
        assert got["v"][0] == want["v"] and got["xinf"][0] == want["xinf"], (got["v"], want["v"], got["xinf"], want["xinf"])
        assert got["dec"][0] == want["dec"] == dict(accept=A.ACCEPT, grow=A.GROW, keep=A.KEEP)[c["kind"]]
        assert got["mu"].astype(dt)[sel].tobytes() == want["mu"].astype(dt)[sel].tobytes()
        av = want["alm"]
        assert av[S:].any() and not av[:S].any()
        if want["dec"] == A.ACCEPT:
            z = np.where(av, np.clip(c["x"], c["lo"], c["hi"]), c["x"]).astype(dt)
            assert got["z"].astype(dt)[sel].tobytes() == z[sel].tobytes()
            assert np.isnan(got["lo2"]).all() and np.isnan(got["w2"]).all()
            continue
        assert want["w"] == (c["wk"] * 10.0 if c["kind"] == "grow" else c["wk"])
        for k in ("lo2", "hi2", "w2"):
            assert np.isnan(got[k][~av]).all(), k                          # only the ALM variables are written
            assert got[k].astype(dt)[av & _mask(sel, N)].tobytes() == want[k].astype(dt)[av & _mask(sel, N)].tobytes(), k
        assert np.isnan(got["z"]).all()


def _mask(sel, N):
    m = np.zeros(N, bool)
    m[sel] = True
    return m


UPDATE = [(S, C, K, dt) for S, C in A.SHAPES for K in (2, 3, 9) for dt in (np.float64, np.float32)]


@pytest.mark.parametrize("S,C,K,dt", UPDATE, ids=["%d-%d-%d-%s" % (S, C, K, np.dtype(dt).name) for S, C, K, dt in UPDATE])
def test_update_kernels(S, C, K, dt):
    """One system of each decision alone (NULL weights), and the three as a batch with user weights."""
    for i, kind in enumerate(("accept", "grow", "keep")):
        check_update(solver(S, C, K, dt), [update_inputs(S, C, K, dt, kind, i, False)], dt)
    check_update(solver(S, C, K, dt, batch=3), [update_inputs(S, C, K, dt, kind, 10 + i, True) for i, kind in enumerate(("accept", "grow", "keep"))], dt)


def test_update_kernels_past_the_grid_cap():
    """2/1/8197: the knots >= 8192 are the second pass over the grid, compared alone."""
    S, C, K = P.SWEEP_LONG
    assert K > CAP
    check_update(solver(S, C, K, np.float64), [update_inputs(S, C, K, np.float64, "grow", 3, True)], np.float64, knots=range(CAP, K))


# ---- 2. end to end on the pinned seeds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", A.F64_CASES, ids=["%d-%d-%d" % c for c in A.F64_CASES])
def test_converges_on_hard_state_bounds(S, C, K):
    p = A.alm_box(S, C, K)
    assert p is not None, "no pinned seed"
    alm_cold_case(p)


@pytest.mark.parametrize("S,C,K", A.F32_CASES, ids=["%d-%d-%d" % c for c in A.F32_CASES])
def test_fp32_follows_the_reference(S, C, K):
    """fp32 at eps = F32_EPS, the PCG exit tolerance F32_EXIT_TOL and the fp32 weight cap, on the problem rounded to fp32, whose
    fp32 stage restatement follows the reference."""
    p = A.alm_box(S, C, K, f32=True)
    assert p is not None, "no pinned seed"
    sol = solver(S, C, K, np.float32)
    r = alm_run(sol, [p], eps=p["eps"])
    check_run(sol, p, r)
    check_steps(sol, p)
    assert float(r.weight[0]) <= A.F32_WEIGHT_MAX
    assert alm_bits(alm_run(sol, [p], eps=p["eps"]), 0, sol) == alm_bits(r, 0, sol)


# ---- 3. the problems no other method solves ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.NAMED)
def test_named_problems_converge_where_the_active_set_iteration_does_not(name):
    """Both double integrators with a hard velocity bound and 6/3/20 seed 2: box_qp(method="alm") ends CONVERGED at a KKT point of
    the hard QP with the reference's counts; method="pdas" on the same inputs does not converge."""
    import gato_python_amd
    p = A.named(name)
    s, run = p["s"], A.run_alm(p)
    assert run["status"] == A.CONVERGED
    ts = math_inputs(p)
    r = gato_python_amd.box_qp(*ts, rho=s.rho, method="alm", **F64)
    print(name, "outer", int(r.outer), "solves", int(r.iters), "weight", float(r.weight), "reference", run["outer"], run["iters"], run["weight"])
    assert int(r.status) == _lib.QP_CONVERGED
    assert (int(r.outer), int(r.iters), float(r.weight)) == (run["outer"], run["iters"], run["weight"])
    x, y, lam = (t.cpu().numpy() for t in (r.x, r.y, r.lam))
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], *A.hard_box(p), x, y, lam)
    print("kkt", kk)
    assert kk["stat"] <= 1e-7 and kk["eq"] <= 1e-7 and kk["bound"] <= 1e-6 * (1 + np.abs(x).max())
    hard = gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", **F64)
    assert int(hard.status) != _lib.QP_CONVERGED


# ---- 4. a batch ------------------------------------------------------------------------------------------------------------------
def batch_problems():
    """Five 14/7/9 systems of different seeds: the pinned one, three more that converge, and an infeasible one in the middle."""
    S, C, K, B = P.SWEEP_BATCH
    pin = A.alm_box(S, C, K)
    good, bad = [pin], None
    for seed in range(AS.WALK_SEEDS):
        if len(good) == B - 1 and bad is not None:
            break
        if seed == pin["seed"]:
            continue
        p = A.state_problem(S, C, K, seed, "tube" if len(good) < B - 1 else False)
        if len(good) < B - 1:
            p["run"] = A.run_alm(p, max_alm_iters=20)
            if p["run"]["status"] == A.CONVERGED:
                good.append(p)
                continue
        p = A.state_problem(S, C, K, seed)
        if bad is None and not A.feasible(p):
            bad = p
    assert len(good) == B - 1 and bad is not None
    return good[:2] + [bad] + good[2:]


def test_batch_of_five_with_an_infeasible_system():
    S, C, K, B = P.SWEEP_BATCH
    ps = batch_problems()
    sol = solver(S, C, K, np.float64, batch=B)
    outs = sentinels(sol)
    r = alm_run(sol, ps, outs=outs, max_alm_iters=20)
    print("status", r.status.tolist(), "outer", r.outer.tolist(), "iters", r.iters.tolist(), "weight", r.weight.tolist())
    for i, p in enumerate(ps):
        one = solver(S, C, K, np.float64)
        solo = alm_run(one, [p], outs=sentinels(one), max_alm_iters=20)
        assert alm_bits(r, i, sol) == alm_bits(solo, 0, one), i
        if i == 2:
            assert int(r.status[i]) == _lib.QP_MAX_ITERS and untouched(r, i, sol) and int(r.outer[i]) == 20
            assert float(r.res_prim[i]) > 1e-4 and float(r.res_dual[i]) == 0.0
        else:
            assert int(r.status[i]) == _lib.QP_CONVERGED and int(r.iters[i]) == p["run"]["iters"], i


# ---- 5. hard controls with soft states -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", [(6, 3, 9), (14, 7, 3)], ids=["6-3-9", "14-7-3"])
def test_hard_controls_with_soft_states(S, C, K):
    """The pinned problem with weight 100 and cap 1 on every state: the states stay soft bounds - no multiplier and no shift, y is
    the capped force of the unshifted bounds - and the controls are held to the bar."""
    p = dict(A.alm_box(S, C, K))
    n, N = S + C, p["s"].N
    state = (np.arange(N) % n) < S
    p.update(w=np.where(state, 100.0, 0.0), m=np.where(state, 1.0, np.inf))
    run = A.run_alm(p)
    assert run["status"] == A.CONVERGED
    sol = solver(S, C, K, np.float64)
    r = alm_run(sol, [p])
    x, z, y, lam = point(r, 0, sol)
    print("outer", int(r.outer[0]), run["outer"], "iters", int(r.iters[0]), run["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED and (int(r.outer[0]), int(r.iters[0])) == (run["outer"], run["iters"])
    soft = state & (np.isfinite(p["lo"]) | np.isfinite(p["hi"]))
    soft[:S] = False
    force = AS.force(p["lo"], p["hi"], p["w"], p["m"], x)
    assert np.abs(y - force)[soft].max() <= 1e-9 * max(1.0, np.abs(force).max()) and np.abs(force[soft]).max() > 0
    assert np.array_equal(z[soft], x[soft])
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], x, y, lam, p["w"], p["m"])
    print("kkt", kk)
    assert kk["stat"] <= 1e-7 and kk["eq"] <= 1e-7 and kk["bound"] <= 1e-6 * (1 + np.abs(x).max()) and kk["force"] <= 1e-7


# ---- 6. warm starts, polish, refusals ------------------------------------------------------------------------------------------
def test_warm_start_takes_fewer_solves():
    """warm= a previous result: its y starts the multipliers and its act the active set.  The reference's warm run's solves and
    outer steps, fewer solves than cold, the reference's warm point within 1e-7 (a tenth of eps: the two run the same iteration,
    a PCG against an LU) and the cold point within the acceptance bar eps (1 + |x|_inf)."""
    import gato_python_amd
    p = A.alm_box(6, 3, 9)
    ts = math_inputs(p)
    cold = gato_python_amd.box_qp(*ts, rho=p["s"].rho, method="alm", **F64)
    warm = gato_python_amd.box_qp(*ts, rho=p["s"].rho, method="alm", warm=cold, **F64)
    want = A.run_alm(p, act0=p["run"]["act"], mu0=p["run"]["mu"])
    x, lam = warm.x.cpu().numpy(), warm.lam.cpu().numpy()
    bar = 1e-6 * (1 + float(np.abs(x).max()))
    to_ref, to_cold = float(np.abs(x - want["x"]).max()), float((warm.x - cold.x).abs().max())
    print("cold", int(cold.iters), int(cold.outer), "warm", int(warm.iters), int(warm.outer), "reference warm", want["iters"], want["outer"],
          "|x - x_ref warm|", to_ref, "|x warm - x cold|", to_cold, "bar", bar, "reference's own warm - cold", float(np.abs(want["x"] - p["run"]["x"]).max()))
    assert int(warm.status) == _lib.QP_CONVERGED and int(warm.iters) < int(cold.iters)
    assert (int(warm.iters), int(warm.outer), float(warm.weight)) == (want["iters"], want["outer"], want["weight"])
    assert np.array_equal(warm.act.cpu().numpy(), want["act"])
    assert to_ref <= 1e-7 and float(np.abs(lam - want["lam"]).max()) <= 1e-7 * max(1.0, float(np.abs(want["lam"]).max()))
    assert to_cold <= bar


def test_polish_gives_the_vertex():
    """2/1/9 (LICQ holds at its x*): the polish on the point's active set is ACCEPTED and x is within the bar of x*."""
    import gato_python_amd
    p = A.alm_box(2, 1, 9)
    ts = math_inputs(p)
    r = gato_python_amd.box_qp(*ts, rho=p["s"].rho, method="alm", polish=True, **F64)
    x = r.x.cpu().numpy()
    dist = float(np.abs(x - p["exact"]["x"]).max())
    print("polished", int(r.polished), "|x - x*|", dist)
    assert int(r.status) == _lib.QP_CONVERGED and int(r.polished) == _lib.POLISH_ACCEPTED
    assert dist <= 1e-6 * (1 + np.abs(x).max())
    assert float(np.maximum(np.maximum(p["lo"] - x, x - p["hi"]), 0.0)[p["s"].S:].max()) == 0.0       # on the bounds bit for bit


def test_refusals():
    import gato_python_amd
    p = A.alm_box(2, 1, 9)
    s = p["s"]
    ts = math_inputs(p)
    call = lambda **kw: gato_python_amd.box_qp(*ts, rho=s.rho, method="alm", **F64, **kw)
    for kw, text in ((dict(admm_rho=1.0), "admm_rho is not read by method='alm'"), (dict(check_every=5, alpha=1.5), "alpha, check_every are not read"),
                     (dict(line_search=True), "line_search is implied"), (dict(alm_weight=0.0), "finite alm_weight > 0"),
                     (dict(alm_growth=1.0), "alm_growth > 1"), (dict(alm_weight_max=10.0), "alm_weight_max >= alm_weight"),
                     (dict(max_alm_iters=0), "at least 1"), (dict(x_soft_max=1.0), "give x_soft or u_soft too"),
                     (dict(polish=True, x_soft=1.0), "hard bounds only")):
        with pytest.raises(ValueError, match=text):
            call(**kw)
    with pytest.raises(ValueError, match="need method='alm'"):
        gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", alm_weight=10.0, **F64)
    sol = solver(2, 1, 9, np.float64)
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    for kw in (dict(alm_weight=float("nan")), dict(alm_growth=0.5), dict(alm_weight=100.0, alm_weight_max=1.0)):
        with pytest.raises(ValueError, match=r"systems \[0\].*alm_weight > 0.*BAD_BOUNDS"):
            sol.box_qp_alm(*inp, rho=s.rho, **F64, **kw)
    bad = list(inp)
    bad[4] = inp[4].clone()
    bad[4][s.S + s.C] = float("nan")
    with pytest.raises(ValueError, match=r"systems \[0\].*a bound is NaN.*BAD_BOUNDS"):
        sol.box_qp_alm(*bad, rho=s.rho, **F64)
    act = torch.zeros(s.N, dtype=torch.int8, device="cuda")
    act[0] = 1                                                          # a state of x_0
    with pytest.raises(ValueError, match=r"systems \[0\].*BAD_ACTIVE"):
        sol.box_qp_alm(*inp, rho=s.rho, act=act, **F64)
    assert int(alm_run(sol, [p]).status[0]) == _lib.QP_CONVERGED         # and the solver is usable afterwards


def test_stream_capture_is_refused():
    p = A.alm_box(2, 1, 9)
    sol = solver(2, 1, 9, np.float64)
    inp = dev_inputs(sol, [p["s"]], [(p["lo"], p["hi"])])
    alm_run(sol, [p])                                                    # the work area exists: nothing is allocated under capture
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with pytest.raises(_lib.GatoError, match="box_qp_alm: the stream is being captured"):
            with torch.cuda.graph(graph, stream=st):
                sol.box_qp_alm(*inp, rho=p["s"].rho, **F64)
    torch.cuda.synchronize()
