"""Capped (Huber) soft bounds in the active-set iteration on the device (gato_box_qp_pdas_huber, gato_box_qp_huber_grad,
Solver.box_qp_pdas(soft_cap=), Solver.box_qp_huber_grad, box_qp / box_qp_layer(method="pdas", x_soft_max=, u_soft_max=)) against
the numpy reference of tests/box_qp_active_ref.py: the reference's number of solves and final act, +-2 included, on walked
problems (tests/test_box_qp_huber_cpu.py asserts that the walks find them), no caps equal to gato_box_qp_pdas_soft bit for bit,
batches, warm starts, the grid cap, fp32, gradients.  Bars: those of tests/test_gpu_box_qp_soft.py - fp64 parity 1e-6 in the
infinity norm, Huber KKT residuals <= 1e-7."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_huber_ref as R                      # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_soft_ref as SR                      # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import (CAP, F64, SENTINEL, check_point, cold_case, dev_inputs, dev_w, fp32_case, host, math_inputs, pdas, point_bits,  # noqa: E402
                           raw_pdas, sentinels, solver, untouched)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def huber(sol, inp, w, m, rho, **kw):
    """Solver.box_qp_pdas with the weights w and the caps m (device tensors; m None: no caps) through box_qp_device.pdas."""
    return pdas(sol, inp, rho, soft_weight=w, soft_cap=m, **kw)


# ---- 1. cold starts: capped soft state boxes, hard control boxes ----------------------------------------------------------------
COLD = [(S, C, K) for S, C in R.SHAPES for K in R.COLD_K]


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_cold_capped_state_box(S, C, K):
    ps = R.huber_box(S, C, K)
    assert ps, "the walk finds no seed at %d/%d/%d" % (S, C, K)
    p = ps[0]
    run = p["run"]
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "kinds", R.final_kinds(run, p["w"], p["lo"], p["hi"]))
    assert P.sat_set(run["act"]).any()
    cold_case(p)


@pytest.mark.parametrize("S,C,K", [(6, 3, 9), (14, 7, 3)], ids=["6-3-9", "14-7-3"])
def test_cold_mixed_weights_and_caps(S, C, K):
    """A weight and a cap per variable, on states and controls: the final act holds a saturated control."""
    p = R.mixed_box(S, C, K)
    s, run = p["s"], p["run"]
    assert (P.sat_set(run["act"]) & (np.arange(s.N) % (S + C) >= S) & (p["lo"] != p["hi"])).any()
    sol = solver(S, C, K, np.float64)
    r = huber(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), dev_w(sol, [p["w"]]), dev_w(sol, [p["m"]]), s.rho)
    check_point(sol, r, 0, p, run)


# ---- 2. fp32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", R.F32_CASES, ids=["%d-%d-%d" % c for c in R.F32_CASES])
def test_fp32_ends_on_the_reference_act(S, C, K):
    """fp32 under the fp32 seed rule at eps = F32_EPS, PCG exit tolerance F32_EXIT_TOL (box_qp_soft_ref): the reference's solves
    and act, the hard bounds and y = +-m on the saturated set bit for bit."""
    p = R.huber_box(S, C, K, f32=True)[0]
    assert P.sat_set(p["run"]["act"]).any()
    fp32_case(p)


# ---- 3. no caps: gato_box_qp_pdas_soft, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_no_caps_is_box_qp_pdas_soft(shape):
    """A walked soft problem: a NULL cap pointer, a tensor of +inf, finite caps on the variables with w = 0 (the controls) and
    on the soft variables that never leave their bounds on the way give every output of gato_box_qp_pdas_soft bit for bit."""
    S, C = shape
    p = SR.soft_box(S, C, 9)[0]
    s, w = p["s"], p["w"]
    sol = solver(S, C, 9, np.float64)
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    wd = dev_w(sol, [w])
    want = raw_pdas(sol, inp, wd, None, "gato_box_qp_pdas_soft", s.rho)[1]
    assert want == point_bits(pdas(sol, inp, s.rho, soft_weight=wd), 0, sol)
    assert raw_pdas(sol, inp, wd, None, "gato_box_qp_pdas_huber", s.rho) == (0, want)
    assert raw_pdas(sol, inp, wd, dev_w(sol, [np.inf]), "gato_box_qp_pdas_huber", s.rho) == (0, want)
    assert point_bits(huber(sol, inp, wd, dev_w(sol, [np.inf]), s.rho), 0, sol) == want
    inside = (w > 0) & ~np.any([t["act"] != 0 for t in p["run"]["trace"]], axis=0)
    bounded = inside & (np.isfinite(p["lo"]) | np.isfinite(p["hi"])) & (np.arange(s.N) >= S + C)
    print("caps on", int((w == 0).sum()), "hard variables and", int(bounded.sum()), "bounded soft variables that stay inside")
    assert bounded.any() or S == 2                  # 2/1/9: each of its eight bounded states is active on some solve
    idle = np.where((w == 0) | inside, 0.5, np.inf)
    assert raw_pdas(sol, inp, wd, dev_w(sol, [idle]), "gato_box_qp_pdas_huber", s.rho) == (0, want)
    # without weights the caps are not read at all: gato_box_qp_pdas
    hard = raw_pdas(sol, inp, None, None, "gato_box_qp_pdas_soft", s.rho)[1]
    assert raw_pdas(sol, inp, None, dev_w(sol, [np.nan]), "gato_box_qp_pdas_huber", s.rho) == (0, hard)


# ---- 4. batches -------------------------------------------------------------------------------------------------------------
def test_batch_of_capped_soft_hard_frozen_and_bad_systems():
    """Five 14/7/9 systems: a capped soft state box (0), an uncapped soft one (1), an all-hard control box (2), a hard state box
    that does not converge (3) and a second capped one (4).  With a NaN cap in system 4 the call raises and writes nothing; with
    good caps every converged system has the bits of its solo run - the uncapped one those of gato_box_qp_pdas_soft - and
    system 3 keeps its sentinels."""
    S, C, K, B = SR.BATCH
    a, b = R.huber_box(S, C, K, count=2)
    inf = np.full(a["s"].N, np.inf)
    unc = dict(SR.soft_box(S, C, K)[0], m=inf)
    ctl = dict(D.control_box(S, C, K)[0], w=np.zeros(a["s"].N), m=inf)
    ps = [a, unc, ctl, dict(SR.hard_state_box_that_fails(S, C, K), m=inf), b]
    sol = solver(S, C, K, np.float64, batch=B)
    inp = dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps])
    rho = a["s"].rho
    wd = dev_w(sol, [p["w"] for p in ps])
    bad = b["m"].copy()
    bad[S + C] = np.nan
    assert b["w"][S + C] > 0
    outs = sentinels(sol)
    with pytest.raises(ValueError, match=r"systems \[4\].*BAD_BOUNDS"):
        huber(sol, inp, wd, dev_w(sol, [p["m"] for p in ps[:4]] + [bad]), rho, outs=outs)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs.values()) and sol.get_option("assembly_valid") == 0
    r = huber(sol, inp, wd, dev_w(sol, [p["m"] for p in ps]), rho, outs=outs)
    print("status", r.status.tolist(), "iters", r.iters.tolist())
    assert int(r.status[3]) in (_lib.QP_MAX_ITERS, _lib.QP_NONFINITE) and untouched(r, 3, sol)
    for i in (0, 1, 2, 4):
        p = ps[i]
        one = solver(S, C, K, np.float64)
        one_inp = dev_inputs(one, [p["s"]], [(p["lo"], p["hi"])])
        solo = huber(one, one_inp, dev_w(one, [p["w"]]), dev_w(one, [p["m"]]), rho, outs=sentinels(one))
        assert int(r.status[i]) == _lib.QP_CONVERGED and int(r.iters[i]) == p["run"]["iters"]
        assert point_bits(r, i, sol) == point_bits(solo, 0, one), i
        if i == 1:
            assert point_bits(pdas(one, one_inp, rho, soft_weight=dev_w(one, [p["w"]])), 0, one) == point_bits(solo, 0, one)
    check_point(sol, r, 0, a, a["run"])
    check_point(sol, r, 4, b, b["run"])
    assert a["run"]["iters"] != b["run"]["iters"] or a["run"]["iters"] != unc["run"]["iters"]      # the systems freeze at different solves


# ---- 5. warm starts and refusals --------------------------------------------------------------------------------------------------
def test_warm_start_from_a_saturated_act_and_refusals():
    p = R.huber_box(6, 3, 9)[0]
    s, run, w, m, lo, hi = p["s"], p["run"], p["w"], p["m"], p["lo"], p["hi"]
    n = s.S + s.C
    sol = solver(6, 3, 9, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    wd, md = dev_w(sol, [w]), dev_w(sol, [m])
    cold = huber(sol, inp, wd, md, s.rho)
    assert P.sat_set(cold.act.cpu().numpy()).any()
    warm = huber(sol, inp, wd, md, s.rho, act=cold.act.cpu().numpy())
    assert int(warm.status[0]) == _lib.QP_CONVERGED and int(warm.iters[0]) == 1
    check_point(sol, warm, 0, p, dict(run, iters=1))
    outs = sentinels(sol)
    # +-2 through gato_box_qp_pdas_soft, on a variable without a weight, without a finite cap, with an infinite bound, on x_0
    with pytest.raises(ValueError, match="BAD_ACTIVE"):
        pdas(sol, inp, s.rho, soft_weight=wd, act=run["act"], outs=outs)
    sat = int(np.flatnonzero(P.sat_set(run["act"]))[0])
    control = int(np.flatnonzero((w == 0) & np.isfinite(hi) & (np.arange(s.N) >= n))[0])
    free_state = int(np.flatnonzero(~np.isfinite(hi) & (np.arange(s.N) >= n) & (w > 0))[0])
    for j, v, caps in ((control, 2, m), (sat, 2, np.where(np.arange(s.N) == sat, np.inf, m)), (free_state, 2, m), (0, 2, m),
                       (sat, 3, m), (sat, -3, m)):
        act = np.zeros(s.N, np.int8)
        act[j] = v
        with pytest.raises(ValueError, match="BAD_ACTIVE"):
            huber(sol, inp, wd, dev_w(sol, [caps]), s.rho, act=act, outs=outs)
        assert sol.get_option("assembly_valid") == 0
    for v in (np.nan, -1.0, -np.inf):
        with pytest.raises(ValueError, match="BAD_BOUNDS"):
            huber(sol, inp, wd, dev_w(sol, [np.where(np.arange(s.N) == sat, v, m)]), s.rho, outs=outs)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs.values())
    with pytest.raises(ValueError, match="soft_weight"):
        sol.box_qp_pdas(*inp, rho=s.rho, soft_cap=md, **F64)
    # a bad cap on a variable without a weight is not read; a cap of 0 takes the bound away: the problem without any state bound
    ok = huber(sol, inp, wd, dev_w(sol, [np.where(w == 0, np.nan, m)]), s.rho)
    assert point_bits(ok, 0, sol) == point_bits(cold, 0, sol)
    zero = huber(sol, inp, wd, dev_w(sol, [0.0]), s.rho)
    H, Cm, g, c = (p[k] for k in ("H", "Cm", "g", "c"))
    want = AS.iterate(H, Cm, g, c, lo, hi, s.S, w, np.zeros(s.N))
    free = AS.iterate(H, Cm, g, c, np.where(w > 0, -np.inf, lo), np.where(w > 0, np.inf, hi), s.S, w)
    assert want["status"] == free["status"] == AS.CONVERGED and np.abs(want["x"] - free["x"]).max() < 1e-9
    assert int(zero.status[0]) == _lib.QP_CONVERGED and np.abs(host(zero.x, 1, sol.N)[0] - want["x"]).max() < 1e-6
    assert not host(zero.y, 1, sol.N)[0][w > 0].any()


# ---- 6. K past the grid cap -------------------------------------------------------------------------------------------------
def test_long_horizon_second_grid_pass():
    """2/1/8197 with capped soft state boxes, from the reference's final act: CONVERGED in one solve on that act, x within 1e-6
    of the sparse reference over the whole vector and over the knots >= 8192 alone, the Huber KKT residuals <= 1e-7, y = +-m
    bit for bit on the saturated set - which reaches past knot 8192."""
    p = R.huber_long()
    s, run = p["s"], p["run"]
    S, C, K = D.LONG
    n = S + C
    assert run["status"] == AS.CONVERGED
    sat = P.sat_set(run["act"])
    assert (np.flatnonzero(sat) // n >= CAP).any()
    sol = solver(S, C, K, np.float64)
    r = huber(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), dev_w(sol, [p["w"]]), dev_w(sol, [p["m"]]), s.rho, act=run["act"],
              max_iters=20000)
    print("solves", int(r.iters[0]), "reference", run["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED and int(r.iters[0]) == 1
    assert np.array_equal(r.act.cpu().numpy(), run["act"])
    x, y, lam = host(r.x, 1, sol.N)[0], host(r.y, 1, sol.N)[0], host(r.lam, 1, sol.sizes["sk"])[0]
    whole, tail = np.abs(x - run["x"]).max(), np.abs(x[CAP * n:] - run["x"][CAP * n:]).max()
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], x, y, lam, p["w"], p["m"])
    print("x err whole", whole, "knots >= 8192", tail, "kkt", kk)
    assert whole < 1e-6 and tail < 1e-6
    assert max(kk.values()) <= 1e-7, kk
    assert np.array_equal(y[sat], np.sign(run["act"])[sat] * p["m"][sat])


# ---- 7. gradients -----------------------------------------------------------------------------------------------------------
def grad_problem(K):
    if K == D.LONG[2]:
        return R.huber_long()
    return R.huber_box(6, 3, K)[0]


GRAD = [(K, dt) for K in (2, 9, D.LONG[2]) for dt in (np.float64, np.float32)]


@pytest.mark.parametrize("K,dt", GRAD, ids=["%d-%s" % (K, np.dtype(dt).name) for K, dt in GRAD])
def test_huber_grad_kernel(K, dt):
    """gato_box_qp_huber_grad as a function of its arrays: a walked problem's final act and point (rounded to the dtype) with a
    random upstream gradient and adjoint (a = 0 on the hard-active set, as an adjoint is), outputs at unaligned addresses,
    against the reference's bound gradients and m_bar = -s a on the saturated set.  Bar: every output is a sum of at most n = 2 S
    + C + 2 products and sums in the dtype, each rounded once (unit roundoff u = eps / 2) relative to a partial sum of at most n
    terms of the largest size: n^2 u times that size."""
    p = grad_problem(K)
    s, act = p["s"], p["run"]["act"]
    S, C = s.S, s.C
    rnd = lambda v: np.asarray(v, dt).astype(np.float64)
    w, m, lo, hi, x = [rnd(p[k]) for k in ("w", "m", "lo", "hi")] + [rnd(p["run"]["x"])]
    rng = np.random.default_rng(5)
    sa, sat = P.soft_set(act, w), P.sat_set(act)
    hard = (act != 0) & ~sa
    xbar, a, beta = rnd(rng.standard_normal(s.N)), rnd(np.where(hard, 0.0, rng.standard_normal(s.N))), rnd(rng.standard_normal(S * K))
    sol = solver(S, C, K, dt)
    Gb, Cb = dev_inputs(sol, [s], [(lo, hi)])[:2]
    Gh, Ch = host(Gb, 1, Gb.numel())[0], host(Cb, 1, Cb.numel())[0]               # the blocks as the device holds them
    dev = lambda v: sol.to_device(np.ascontiguousarray(v, np.float64).astype(dt))
    # H = G + rho I serves for G: rho multiplies a_i, which is 0 wherever the hard formula is evaluated
    want = P.bound_grads(p["H"], p["Cm"], P.unsaturated(act), xbar, a, beta, w, lo, hi, x)
    want = list(want) + [np.where(sat, -np.sign(act) * a, 0.0)]
    outs = [sol.new(s.N + 1).fill_(SENTINEL)[1:] for _ in range(4)]
    got = sol.box_qp_huber_grad(Gb, Cb, torch.from_numpy(act).cuda(), dev(w), dev(m), dev(lo), dev(hi), dev(x), dev(xbar), dev(a),
                                dev(beta), *outs)
    torch.cuda.synchronize()
    n = 2 * S + C + 2
    size = max(1.0, np.abs(Gh).max() * np.abs(a).max(), np.abs(Ch).max() * np.abs(beta).max(), np.abs(w).max() * np.abs(a).max(),
               np.abs(xbar).max(), np.abs(a).max() * np.abs(lo[np.isfinite(lo)]).max(), np.abs(a).max() * np.abs(x).max())
    bar = n * n * 0.5 * np.finfo(dt).eps * size
    for name, g, t in zip(("lo_bar", "hi_bar", "w_bar", "cap_bar"), got, want):
        err = np.abs(g.cpu().numpy().astype(np.float64) - t).max()
        print(name, err, np.abs(t).max(), "bar", bar)
        assert err <= bar, (name, err, bar)
    assert sat.any() and np.all(want[3][sat] != 0) and not np.any(got[3].cpu().numpy()[~sat])
    for t in got[:3]:
        assert not np.any(t.cpu().numpy()[sat])                                  # exactly 0 on the saturated set
    # no caps (a NULL cap pointer) on the act without +-2: box_qp_soft_grad's outputs bit for bit, cap_bar zero
    a1 = torch.from_numpy(P.unsaturated(act)).cuda()
    l1, h1, w1 = sol.box_qp_soft_grad(Gb, Cb, a1, dev(w), dev(lo), dev(hi), dev(x), dev(xbar), dev(a), dev(beta))
    l2, h2, w2, c2 = sol.box_qp_huber_grad(Gb, Cb, a1, dev(w), None, dev(lo), dev(hi), dev(x), dev(xbar), dev(a), dev(beta))
    assert torch.equal(l1, l2) and torch.equal(h1, h2) and torch.equal(w1, w2) and not c2.any()


LAYER = [(6, 3, 9, False), (6, 3, 9, True), (14, 7, 3, False), (14, 7, 3, True)]


@pytest.mark.parametrize("S,C,K,stale", LAYER, ids=["%d-%d-%d-%s" % (S, C, K, "stale" if st else "fresh") for S, C, K, st in LAYER])
def test_layer_gradients_caps_included(S, C, K, stale):
    """box_qp_layer(x_soft=, u_soft=, x_soft_max=, u_soft_max=) on a mixed problem (its final act holds a saturated control):
    all fifteen gradients against the reference, err < 1e-6 max(1, |want|).  stale: another solve on the cached solver between
    the forward and the backward pass, which then rebuilds its assembly from the saved act, +-2 included, with one assembly."""
    import gato_python_amd
    p = R.mixed_box(S, C, K)
    s, run = p["s"], p["run"]
    ts = math_inputs(p, requires_grad=True)
    ws = ts[11:]
    x, lam, info = gato_python_amd.box_qp_layer(*ts[:11], rho=s.rho, method="pdas", x_soft=ws[0], u_soft=ws[1], x_soft_max=ws[2],
                                                u_soft_max=ws[3], **F64)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and int(info.iters) == run["iters"]
    assert np.array_equal(info.act.cpu().numpy(), run["act"]) and P.sat_set(run["act"]).any()
    if stale:
        from gato_python_amd import autograd
        sol = autograd._SOLVERS[(S, C, K, 1, torch.float64, torch.cuda.current_device())]     # the layer's cached solver
        gen = sol.get_option("assembly_gen")
        q = D.control_box(S, C, K)[0]
        other = gato_python_amd.box_qp(*math_inputs(q), rho=q["s"].rho, method="pdas", **F64)
        assert int(other.status) == _lib.QP_CONVERGED and sol.get_option("assembly_gen") == gen + q["run"]["iters"]
        gen = sol.get_option("assembly_gen")
    rng = np.random.default_rng(7)
    xbar, lbar = rng.standard_normal(s.N), rng.standard_normal(S * K)
    ((x * torch.from_numpy(xbar).cuda()).sum() + (lam * torch.from_numpy(lbar).cuda()).sum()).backward()
    if stale:
        assert sol.get_option("assembly_gen") == gen + 1 and sol.get_option("assembly_valid") == 1
    want = P.grads(p["H"], p["Cm"], run["act"], x.detach().cpu().numpy(), lam.detach().cpu().numpy(), xbar, lbar, S, C, K,
                   w=p["w"], m=p["m"], lo=p["lo"], hi=p["hi"])
    for k, t in zip(R.HUBER_KEYS, ts):
        err = np.abs(t.grad.cpu().numpy() - want[k]).max()
        print(k, err, np.abs(want[k]).max())
        assert err < 1e-6 * max(1.0, np.abs(want[k]).max()), (k, err)
    assert np.abs(want["u_soft_max"]).max() > 0 and np.abs(want["x_soft"]).max() + np.abs(want["u_soft"]).max() > 0


# ---- 8. the Python surface ----------------------------------------------------------------------------------------------------
def test_box_qp_caps_are_the_solver_call():
    import gato_python_amd
    p = R.huber_box(6, 3, 9)[0]
    s = p["s"]
    ts = math_inputs(p)
    ts, ws = ts[:11], ts[11:]
    kw = dict(x_soft=ws[0], u_soft=ws[1], x_soft_max=ws[2], u_soft_max=ws[3])
    res = gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", **kw, **F64)
    assert int(res.status) == _lib.QP_CONVERGED and int(res.iters) == p["run"]["iters"] and res.x.shape == (s.N,)
    assert np.array_equal(res.act.cpu().numpy(), p["run"]["act"])
    sol = solver(s.S, s.C, s.K, np.float64)
    direct = huber(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), dev_w(sol, [p["w"]]), dev_w(sol, [p["m"]]), s.rho)
    for name in ("x", "z", "y", "lam", "res_prim", "res_dual", "act"):
        assert getattr(res, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name
    # numbers broadcast like the weights (u_soft_max None: no cap there); batched input; warm.act carries +-2
    again = gato_python_amd.box_qp(*(t[None] for t in ts), rho=s.rho, method="pdas", x_soft=R.WEIGHT, x_soft_max=R.CAP, warm=res, **F64)
    assert again.x.shape == (1, s.N) and again.iters.tolist() == [1] and again.status.tolist() == [_lib.QP_CONVERGED]
    assert again.x[0].cpu().numpy().tobytes() == res.x.cpu().numpy().tobytes()
    for bad in (dict(method="admm"), dict(method="admm", polish=True), dict(method="pdas", polish=True)):
        with pytest.raises(ValueError, match="x_soft_max"):
            gato_python_amd.box_qp(*ts, rho=s.rho, x_soft=1.0, x_soft_max=1.0, **bad, **F64)
    with pytest.raises(ValueError, match="x_soft_max"):
        gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", u_soft_max=1.0, **F64)       # a cap without any weight
    with pytest.raises(ValueError, match="x_soft_max"):
        gato_python_amd.box_qp_layer(*ts, rho=s.rho, x_soft=1.0, u_soft_max=1.0, **F64)    # method="admm"
    with pytest.raises(ValueError, match="x_soft_max"):
        gato_python_amd.box_qp_layer(*ts, rho=s.rho, method="pdas", x_soft_max=1.0, **F64)
