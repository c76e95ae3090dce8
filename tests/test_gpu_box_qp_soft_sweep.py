"""The soft-bound branches of the active-set kernels (gato_polish.hip, gato_pdas.hip, polished_point_knot) and the x_soft /
u_soft surface of qp.py on mixed problems: hard and soft bounds side by side in one Q_k or R_k, soft controls, a weight per
variable (box_qp_soft_ref.mixed_problem; what its walks must find - cover() - is asserted on the CPU by
tests/test_box_qp_soft_cpu.py), batches of different weights on one system, and qp_bound_grad_kernel with weights as a function
of its arrays at every shape, both precisions, two systems and past the grid cap.
Bars: those of tests/test_gpu_box_qp_soft.py - the reference's solves and final act, x and lambda within 1e-6, penalised KKT
residuals <= 1e-7, hard-active x the bounds bit for bit; the gradient kernel 1e-12 * scale * (2 S + C) in fp64 and
tests/f32_parity.py's rule in fp32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_soft_ref as R                       # noqa: E402
from f32_parity import check_f32                  # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import (CAP, F64, SENTINEL, check_point, cold_case, dev_inputs, dev_w, fp32_case, g_and_c, host, math_inputs,  # noqa: E402
                           pdas, point_bits, solver)

SHAPES = R.SHAPES
NAMES = ("lo_bar", "hi_bar", "w_bar")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def describe(p):
    run = p["run"]
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "cover (a, b, c)", p["cover"])


# ---- 1. cold starts on mixed problems -----------------------------------------------------------------------------------------
COLD = [(S, C, K) for S, C in SHAPES for K in R.COLD_K]


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_cold_mixed_box(S, C, K):
    p = R.mixed_box(S, C, K)[0]
    describe(p)
    assert R.covers(p["cover"], R.cover_need(S, C, K))
    cold_case(p)


# ---- 2. fp32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%d-%d-3" % sh)
def test_fp32_mixed_ends_on_the_reference_act(shape):
    """test_fp32_ends_on_the_reference_act on a mixed problem: eps = F32_EPS, PCG exit tolerance F32_EXIT_TOL."""
    S, C = shape
    K = R.MIXED_F32_K
    p = R.mixed_box(S, C, K, f32=True)[0]
    describe(p)
    fp32_case(p)


# ---- the gradient kernel as a function of its arrays ------------------------------------------------------------------------
def grad_scale(H, Cm, w, a, beta):
    return max(1.0, abs(H).max() * np.abs(a).max(), abs(Cm).max() * np.abs(beta).max(), np.abs(w).max() * np.abs(a).max())


def soft_grad_case(S, C, K, B, dt):
    """Per system, everything rounded to dt and of its own draw: a dense-block system, a box with a tenth of the sides infinite
    and a few lo == hi, weights 10 ** uniform(0, 3) on about half the variables and 0 on the rest, a random legal act (0 on
    x_0 and wherever the bound of its side is infinite, -1 where lo == hi), x, xbar, beta, and a with a = 0 on the
    hard-active set (the kernel's contract).  Forced: a soft-active and a hard-active variable among the states of the last
    knot (lanes 0, 1) and, K > 2, of knot 1, and among the controls of knot 0 - 2/1 has one control: soft-active in system
    0, hard-active in the others; the forced sides alternate with the system.  -> dict of [B, .] fp64 arrays and the systems."""
    rng = np.random.default_rng([S, C, K, 23])
    n = S + C
    systems = [P.constructed_system(S, C, K, 40 + b).astype(dt).astype(np.float64) for b in range(B)]
    N, sk = systems[0].N, S * K
    r = lambda v: np.asarray(v, dt).astype(np.float64)
    lo, hi = r(-rng.uniform(0.5, 1.5, (B, N))), r(rng.uniform(0.5, 1.5, (B, N)))
    lo[rng.random((B, N)) < 0.1] = -np.inf
    hi[rng.random((B, N)) < 0.1] = np.inf
    eq = (rng.random((B, N)) < 0.05) & np.isfinite(lo)
    hi[eq] = lo[eq]
    w = r(np.where(rng.random((B, N)) < 0.5, 10.0 ** rng.uniform(0.0, 3.0, (B, N)), 0.0))
    act = rng.integers(-1, 2, (B, N)).astype(np.int8)
    last = (K - 1) * n
    forced = [(last, 1, True), (last + 1, -1, False)]                            # (index, act, soft)
    if K > 2:
        forced += [(n, -1, True), (n + 1, 1, False)]
    for b in range(B):
        ctl = [(S, 1, True), (S + 1, -1, False)] if C > 1 else [(S, 1, b == 0)]
        for j, ai, is_soft in forced + ctl:
            lo[b, j], hi[b, j] = r(-0.75 - 0.01 * b), r(0.8 + 0.01 * b)
            act[b, j] = ai if b % 2 == 0 else -ai                                # 2/1/2 has no other variable: the systems' acts differ
            w[b, j] = r(7.0 + 3.0 * b) if is_soft else 0.0
    act[lo == hi] = -1
    act[(act > 0) & ~np.isfinite(hi)] = 0
    act[(act < 0) & ~np.isfinite(lo)] = 0
    act[:, :S] = 0
    hard = (act != 0) & ~(w > 0)
    x, xbar, beta = r(rng.uniform(-2.0, 2.0, (B, N))), r(rng.standard_normal((B, N))), r(rng.standard_normal((B, sk)))
    a = np.where(hard, 0.0, r(rng.standard_normal((B, N))))
    return dict(systems=systems, act=act, w=w, lo=lo, hi=hi, x=x, xbar=xbar, a=a, beta=beta)


def grad_case_cover(case, S, C, K):
    """Per system (states of one knot mixed, controls of one knot mixed, the last knot mixed); over all systems whether a
    control is soft-active and whether one is hard-active."""
    n = S + C
    out, ctl_soft, ctl_hard = [], False, False
    for act, w in zip(case["act"], case["w"]):
        idx = np.arange(len(act))
        knot, ctl = idx // n, idx % n >= S
        sa = P.soft_set(act, w)
        hard = (act != 0) & ~sa
        mixed = lambda part: np.intersect1d(knot[sa & part], knot[hard & part])
        out.append((mixed(~ctl).size > 0, mixed(ctl).size > 0, K - 1 in mixed(~ctl)))
        ctl_soft |= bool((sa & ctl).any())
        ctl_hard |= bool((hard & ctl).any())
    return out, ctl_soft, ctl_hard


def run_soft_grad(sol, case):
    """gato_box_qp_soft_grad on the case, the three outputs one element into their allocations behind a sentinel.
    -> [lo_bar, hi_bar, w_bar] as [B, N] fp64."""
    B, N = sol.batch, sol.N
    inf = np.full(N, np.inf)
    Gb, Cb = dev_inputs(sol, case["systems"], [(-inf, inf)] * B)[:2]
    d = lambda v: sol.to_device(v.reshape(-1))
    base = [sol.new(B * N + 1).fill_(SENTINEL) for _ in range(3)]
    got = sol.box_qp_soft_grad(Gb, Cb, sol.to_device(case["act"].reshape(-1), np.int8), d(case["w"]), d(case["lo"]), d(case["hi"]),
                               d(case["x"]), d(case["xbar"]), d(case["a"]), d(case["beta"]), *(t[1:] for t in base))
    torch.cuda.synchronize()
    assert all(float(t[0]) == SENTINEL for t in base)
    assert all(g.data_ptr() == t.data_ptr() + t.element_size() for g, t in zip(got, base))
    return [host(g, B, N) for g in got]


def off_the_active_set_is_zero(got, act, w):
    sa = P.soft_set(act, w)
    assert not got[0][act >= 0].any() and not got[1][act <= 0].any() and not got[2][~sa].any()


def grad_oracle32(H, Cm, case, b):
    """box_qp_soft_ref.bound_grads's formulas evaluated in numpy fp32."""
    f = lambda v: np.asarray(v, np.float32)
    act, w, lo, hi = case["act"][b], f(case["w"][b]), f(case["lo"][b]), f(case["hi"][b])
    x, xbar, a, beta = (f(case[k][b]) for k in ("x", "xbar", "a", "beta"))
    sa = P.soft_set(act, w)
    hard = (act != 0) & ~sa
    bnd = np.where(act > 0, hi, np.where(act < 0, lo, np.float32(0)))
    zero = np.float32(0)
    with np.errstate(invalid="ignore"):
        bb = np.where(hard, xbar - (f(H) @ a + f(Cm).T @ beta), np.where(sa, w * a, zero))
        out = [np.where(act < 0, bb, zero), np.where(act > 0, bb, zero), np.where(sa, a * (bnd - x), zero)]
    assert all(o.dtype == np.float32 for o in out)
    return out


# ---- 3. a batch of different weight vectors on one system -------------------------------------------------------------------
def test_batch_of_weight_vectors_on_one_system():
    """14/7/9, four systems with the same matrices and box (box_qp_soft_ref.weight_batch): mixed weights, the same pattern
    times 10, no weights, state_weights.  Each converges after its reference's solves on its reference's act with the bits
    of its solo run; the mixed and the scaled one differ in x as their references do.  Then gato_box_qp_soft_grad on the
    four converged points at once, against bound_grads per system at the direct sweep's bar."""
    seed, (s, H, Cm, g, c, lo, hi, _), ws, runs = R.weight_batch_box()
    S, C, K = s.S, s.C, s.K
    B = len(ws)
    print("seed", seed, "solves", [r["iters"] for r in runs])
    sol = solver(S, C, K, np.float64, batch=B)
    inp = dev_inputs(sol, [s] * B, [(lo, hi)] * B)
    wd = dev_w(sol, ws)
    r = pdas(sol, inp, s.rho, soft_weight=wd)
    acts = r.act.cpu().numpy().reshape(B, -1)
    for i, (w, run) in enumerate(zip(ws, runs)):
        one = solver(S, C, K, np.float64)
        solo = pdas(one, dev_inputs(one, [s], [(lo, hi)]), s.rho, soft_weight=dev_w(one, [w]))
        assert int(r.status[i]) == _lib.QP_CONVERGED and int(r.iters[i]) == run["iters"], (i, r.status.tolist(), r.iters.tolist())
        assert np.array_equal(acts[i], run["act"]), i
        assert point_bits(r, i, sol) == point_bits(solo, 0, one), i
    x = host(r.x, B, sol.N)
    want_gap = np.abs(runs[0]["x"] - runs[1]["x"]).max()
    gap = np.abs(x[0] - x[1]).max()
    print("mixed against scaled: |x - x'|", gap, "reference", want_gap)
    assert want_gap > 1e-3 and gap > 1e-3
    check_point(sol, r, 0, dict(H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, w=ws[0]), runs[0])
    # the gradient kernel over the batch: one act, one weight vector and one point per system
    rng = np.random.default_rng(11)
    W = np.stack(ws)
    hard = (acts != 0) & ~(W > 0)
    xbar, beta = rng.standard_normal((B, sol.N)), rng.standard_normal((B, S * K))
    a = np.where(hard, 0.0, rng.standard_normal((B, sol.N)))
    d = lambda v: sol.to_device(np.ascontiguousarray(v, np.float64).reshape(-1))
    got = sol.box_qp_soft_grad(inp[0], inp[1], r.act, wd, inp[4], inp[5], r.x, d(xbar), d(a), d(beta))
    torch.cuda.synchronize()
    got = [host(t, B, sol.N) for t in got]
    Hg, Cg = (m.toarray() for m in g_and_c(s))
    for i in range(B):
        want = P.bound_grads(Hg, Cg, acts[i], xbar[i], a[i], beta[i], ws[i], lo, hi, x[i])
        bar = 1e-12 * grad_scale(Hg, Cg, ws[i], a[i], beta[i]) * (2 * S + C)
        for name, t, wt in zip(NAMES, got, want):
            err = np.abs(t[i] - wt).max()
            print("system", i, name, err, "of", np.abs(wt).max(), "bar", bar)
            assert err <= bar, (i, name, err)
        off_the_active_set_is_zero([t[i] for t in got], acts[i], ws[i])
    assert np.abs(got[2][0]).max() > 0 and np.abs(got[2][1]).max() > 0 and not got[2][2].any()


# ---- 4. qp_bound_grad_kernel with weights, every shape, two systems, both precisions --------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("K", [2, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_soft_grad_direct(shape, K, dt):
    """fp64: against box_qp_soft_ref.bound_grads at test_soft_grad_kernel's bar, 1e-12 * scale * (2 S + C).  fp32: against the
    fp64 formula on the fp32-rounded inputs, held to check_f32's rule beside the same formula in numpy fp32.  Every entry off
    the active set is exactly 0."""
    S, C = shape
    B = 2
    case = soft_grad_case(S, C, K, B, dt)
    cov, ctl_soft, ctl_hard = grad_case_cover(case, S, C, K)
    print("mixed (states, controls, last knot) per system", cov)
    assert all(st and last and (ct or C == 1) for st, ct, last in cov) and ctl_soft and ctl_hard
    assert not np.array_equal(case["act"][0], case["act"][1]) and not np.array_equal(case["w"][0], case["w"][1])
    sol = solver(S, C, K, dt, batch=B)
    got = run_soft_grad(sol, case)
    for b, s in enumerate(case["systems"]):
        H, Cm = (m.toarray() for m in g_and_c(s))
        act, w = case["act"][b], case["w"][b]
        off_the_active_set_is_zero([t[b] for t in got], act, w)
        want = P.bound_grads(H, Cm, act, case["xbar"][b], case["a"][b], case["beta"][b], w, case["lo"][b], case["hi"][b], case["x"][b])
        assert all(np.abs(t).max() > 0 for t in want)
        if dt == np.float64:
            bar = 1e-12 * grad_scale(H, Cm, w, case["a"][b], case["beta"][b]) * (2 * S + C)
            for name, t, wt in zip(NAMES, got, want):
                err = np.abs(t[b] - wt).max()
                print("system", b, name, err, "of", np.abs(wt).max(), "bar", bar)
                assert err <= bar, (b, name, err)
        else:
            for name, t, o32, wt in zip(NAMES, got, grad_oracle32(H, Cm, case, b), want):
                check_f32("soft grad %s %d/%d/%d system %d" % (name, S, C, K, b), t[b], o32, wt)


# ---- 5. qp_bound_grad_kernel with weights past the grid cap ---------------------------------------------------------------------
def test_soft_grad_long_horizon():
    S, C, K = D.LONG
    n = S + C
    case = soft_grad_case(S, C, K, 1, np.float64)
    sol = solver(S, C, K, np.float64)
    got = run_soft_grad(sol, case)
    act, w = case["act"][0], case["w"][0]
    off_the_active_set_is_zero([t[0] for t in got], act, w)
    H, Cm = g_and_c(case["systems"][0])
    want = P.bound_grads(H, Cm, act, case["xbar"][0], case["a"][0], case["beta"][0], w, case["lo"][0], case["hi"][0], case["x"][0])
    bar = 1e-12 * grad_scale(H, Cm, w, case["a"][0], case["beta"][0]) * (2 * S + C)
    tail = slice(CAP * n, None)
    for name, t, wt in zip(NAMES, got, want):
        whole, end = np.abs(t[0] - wt).max(), np.abs(t[0][tail] - wt[tail]).max()
        print(name, "whole", whole, "knots >= 8192", end, "bar", bar)
        assert wt[tail].any()
        assert whole <= bar and end <= bar, (name, whole, end)


# ---- 6. the iteration past the grid cap, soft controls ------------------------------------------------------------------------
def test_long_horizon_mixed_second_grid_pass():
    """2/1/8197 (box_qp_soft_ref.mixed_long) from the reference's final act: CONVERGED in one solve, x within 1e-6 of the
    sparse reference over the whole vector and over the knots >= 8192 alone, the penalised KKT residuals <= 1e-7; a
    soft-active control and a hard-active variable lie among the knots >= 8192."""
    p = R.mixed_long()
    s, run = p["s"], p["run"]
    S, C, K = D.LONG
    n = S + C
    assert run["status"] == AS.CONVERGED
    sa = P.soft_set(run["act"], p["w"])
    idx = np.arange(s.N)
    tail = idx // n >= CAP
    assert (sa & tail & (idx % n >= S) & (p["lo"] != p["hi"])).any() and ((run["act"] != 0) & ~sa & tail).any()
    sol = solver(S, C, K, np.float64)
    r = pdas(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), s.rho, soft_weight=dev_w(sol, [p["w"]]), act=run["act"], max_iters=20000)
    print("seed", p["seed"], "solves", int(r.iters[0]), "reference", run["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED and int(r.iters[0]) == 1
    assert np.array_equal(r.act.cpu().numpy(), run["act"])
    x, y, lam = host(r.x, 1, sol.N)[0], host(r.y, 1, sol.N)[0], host(r.lam, 1, sol.sizes["sk"])[0]
    whole, end = np.abs(x - run["x"]).max(), np.abs(x[CAP * n:] - run["x"][CAP * n:]).max()
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], x, y, lam, p["w"])
    print("x err whole", whole, "knots >= 8192", end, "kkt", kk)
    assert whole < 1e-6 and end < 1e-6
    assert max(kk.values()) <= 1e-7, kk


# ---- 7. the Python surface with u_soft ----------------------------------------------------------------------------------------
def test_box_qp_u_soft_is_the_solver_call():
    import gato_python_amd
    p = R.mixed_box(6, 3, 9)[0]
    s = p["s"]
    ts = math_inputs(p)
    ts, ws = ts[:11], ts[11:]
    assert ws[1].shape == (s.K - 1, s.C) and (ws[1] > 0).any() and (ws[1] == 0).any() and (ws[0] > 0).any()
    sol = solver(s.S, s.C, s.K, np.float64)
    direct = pdas(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), s.rho, soft_weight=dev_w(sol, [p["w"]]))
    assert int(direct.status[0]) == _lib.QP_CONVERGED and int(direct.iters[0]) == p["run"]["iters"]
    names = ("x", "z", "y", "lam", "res_prim", "res_dual", "act")
    res = gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", x_soft=ws[0], u_soft=ws[1], **F64)
    assert int(res.status) == _lib.QP_CONVERGED and res.x.shape == (s.N,)
    for name in names:
        assert getattr(res, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name
    many = gato_python_amd.box_qp(*(t[None] for t in ts), rho=s.rho, method="pdas", x_soft=ws[0][None], u_soft=ws[1][None], **F64)
    assert many.x.shape == (1, s.N) and many.status.tolist() == [_lib.QP_CONVERGED]
    for name in names:
        assert getattr(many, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name


# ---- 8. layer gradients with soft controls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", R.LAYER_CASES, ids=["%d-%d-%d" % c for c in R.LAYER_CASES])
def test_layer_gradients_with_soft_controls(S, C, K):
    """box_qp_layer(x_soft=, u_soft=) on a mixed problem whose final act holds a soft-active control off lo == hi, against
    box_qp_soft_ref.soft_grads over all thirteen inputs at test_layer_gradients_weights_included's bar."""
    import gato_python_amd
    p = R.mixed_layer_box(S, C, K)
    describe(p)
    s, run = p["s"], p["run"]
    ts = math_inputs(p, requires_grad=True)
    ws = ts[11:]
    x, lam, info = gato_python_amd.box_qp_layer(*ts[:11], rho=s.rho, method="pdas", x_soft=ws[0], u_soft=ws[1], **F64)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and int(info.iters) == run["iters"]
    assert np.array_equal(info.act.cpu().numpy(), run["act"])
    rng = np.random.default_rng(7)
    xbar, lbar = rng.standard_normal(s.N), rng.standard_normal(S * K)
    ((x * torch.from_numpy(xbar).cuda()).sum() + (lam * torch.from_numpy(lbar).cuda()).sum()).backward()
    want = P.grads(p["H"], p["Cm"], run["act"], x.detach().cpu().numpy(), lam.detach().cpu().numpy(), xbar, lbar, S, C, K,
                   w=p["w"], lo=p["lo"], hi=p["hi"])
    names = ("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi", "x_soft", "u_soft")
    for k, t in zip(names, ts):
        err = np.abs(t.grad.cpu().numpy() - want[k]).max()
        print(k, err, np.abs(want[k]).max())
        assert err < 1e-6 * max(1.0, np.abs(want[k]).max()), (k, err)
    sc = P.split_states_controls(P.soft_set(run["act"], p["w"]) & (p["lo"] != p["hi"]), S, C, K)[1] > 0
    assert sc.any() and np.abs(want["u_lo"][sc]).max() + np.abs(want["u_hi"][sc]).max() > 0
    assert np.abs(want["u_soft"]).max() > 0 and np.abs(want["x_soft"]).max() > 0 and np.abs(want["R"]).max() > 0
