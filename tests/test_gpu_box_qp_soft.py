"""Soft bounds in the active-set iteration on the device (gato_box_qp_pdas_soft, gato_box_qp_soft_grad, Solver.box_qp_pdas(
soft_weight=), Solver.box_qp_soft_grad, box_qp / box_qp_layer(method="pdas", x_soft=, u_soft=)) against the numpy reference of
tests/box_qp_active_ref.py: the reference's number of solves and final act on walked problems (tests/test_box_qp_soft_cpu.py
asserts that the walks find them), no weights equal to gato_box_qp_pdas bit for bit, batches, the grid cap, fp32, gradients.
Bars: those of tests/test_gpu_box_qp_pdas.py - fp64 parity 1e-6 in the infinity norm, penalised KKT residuals <= 1e-7."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_soft_ref as R                       # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import (CAP, F64, SENTINEL, check_point, cold_case, dev_inputs, dev_w, fp32_case, host, math_inputs, pdas, point_bits,  # noqa: E402
                           raw_pdas, sentinels, solver, untouched)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def soft(sol, inp, w, rho, **kw):
    """Solver.box_qp_pdas with the weights w (a device tensor or None) through box_qp_device.pdas."""
    return pdas(sol, inp, rho, soft_weight=w, **kw)


# ---- 1. cold starts: soft state boxes, hard control boxes ---------------------------------------------------------------------
COLD = [(S, C, K) for S, C in R.SHAPES for K in R.COLD_K]


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_cold_soft_state_box(S, C, K):
    p = R.soft_box(S, C, K)[0]
    print("seed", p["seed"], "solves", p["run"]["iters"], "margin", AS.min_margin(p["run"]))
    cold_case(p)


def test_soft_bounds_converge_where_hard_bounds_do_not():
    """double_integrator(v_max=0.57): the hard iteration meets a singular reduced system (reference and device: MAX_ITERS or
    NONFINITE, nothing written); with the velocity bound soft the device converges as the reference does."""
    s, H, Cm, g, c, lo, hi, w = R.double_integrator_soft()
    assert AS.iterate(H, Cm, g, c, lo, hi, s.S)["status"] in (AS.MAX_ITERS, AS.NONFINITE)
    run = AS.iterate(H, Cm, g, c, lo, hi, s.S, w)
    assert run["status"] == AS.CONVERGED and AS.min_margin(run) >= AS.MARGIN
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    hard = pdas(sol, inp, s.rho, outs=sentinels(sol))
    assert int(hard.status[0]) in (_lib.QP_MAX_ITERS, _lib.QP_NONFINITE) and untouched(hard, 0, sol)
    r = soft(sol, inp, dev_w(sol, [w]), s.rho)
    check_point(sol, r, 0, dict(H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, w=w), run)
    assert P.soft_set(run["act"], w).any()


# ---- 2. fp32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", R.F32_CASES, ids=["%d-%d-%d" % c for c in R.F32_CASES])
def test_fp32_ends_on_the_reference_act(S, C, K):
    """fp32 under the fp32 seed rule at eps = F32_EPS, PCG exit tolerance box_qp_soft_ref.F32_EXIT_TOL (see there: at 1e-8
    the device takes the reference's nine acts at 14/7/9 and then misses the primal bar on the last one, 3.8e-4 against 3.0e-4)."""
    p = R.soft_box(S, C, K, f32=True)[0]
    fp32_case(p)


# ---- 3. no weights: gato_box_qp_pdas, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_no_weights_is_box_qp_pdas(shape):
    """A control-only walked problem: a NULL weight pointer, a tensor of zeros, and positive weights on variables that can never
    be active (the states: unbounded, or of x_0) give every output of gato_box_qp_pdas bit for bit."""
    S, C = shape
    p = D.control_box(S, C, 9)[0]
    s = p["s"]
    sol = solver(S, C, 9, np.float64)
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    want = point_bits(pdas(sol, inp, s.rho), 0, sol)
    assert raw_pdas(sol, inp, None, None, "gato_box_qp_pdas_soft", s.rho) == (0, want)
    assert raw_pdas(sol, inp, dev_w(sol, [0.0]), None, "gato_box_qp_pdas_soft", s.rho) == (0, want)
    assert point_bits(soft(sol, inp, dev_w(sol, [0.0]), s.rho), 0, sol) == want
    assert not np.isfinite(p["lo"][R.state_weights(s) > 0]).any()
    assert point_bits(soft(sol, inp, dev_w(sol, [R.state_weights(s, 50.0)]), s.rho), 0, sol) == want


# ---- 4. batches -------------------------------------------------------------------------------------------------------------
def test_batch_of_soft_hard_frozen_and_bad_systems():
    """Five 14/7/9 systems: soft state boxes (0, 3, 4), an all-hard control box (1) and a hard state box that does not converge
    (2).  With a NaN weight in system 4 the call raises and writes nothing; with good weights every converged system has the
    bits of its solo run and system 2 keeps its sentinels."""
    S, C, K, B = R.BATCH
    a, b = R.soft_box(S, C, K, count=2)
    ctl = dict(D.control_box(S, C, K)[0], w=np.zeros(a["s"].N))
    ps = [a, ctl, R.hard_state_box_that_fails(S, C, K), b, a]
    sol = solver(S, C, K, np.float64, batch=B)
    inp = dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps])
    rho = a["s"].rho
    bad = a["w"].copy()
    bad[S + C] = np.nan
    outs = sentinels(sol)
    with pytest.raises(ValueError, match=r"systems \[4\].*BAD_BOUNDS"):
        soft(sol, inp, dev_w(sol, [p["w"] for p in ps[:4]] + [bad]), rho, outs=outs)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs.values()) and sol.get_option("assembly_valid") == 0
    r = soft(sol, inp, dev_w(sol, [p["w"] for p in ps]), rho, outs=outs)
    print("status", r.status.tolist(), "iters", r.iters.tolist())
    assert int(r.status[2]) in (_lib.QP_MAX_ITERS, _lib.QP_NONFINITE) and untouched(r, 2, sol)
    for i in (0, 1, 3, 4):
        p = ps[i]
        one = solver(S, C, K, np.float64)
        solo = soft(one, dev_inputs(one, [p["s"]], [(p["lo"], p["hi"])]), dev_w(one, [p["w"]]), rho, outs=sentinels(one))
        assert int(r.status[i]) == _lib.QP_CONVERGED and int(r.iters[i]) == p["run"]["iters"]
        assert point_bits(r, i, sol) == point_bits(solo, 0, one), i
    check_point(sol, r, 3, b, b["run"])


# ---- 5. K past the grid cap -------------------------------------------------------------------------------------------------
def test_long_horizon_second_grid_pass():
    """2/1/8197 with soft state boxes, from the reference's final act (its run has margins below the seed rule, so the
    sequence is not demanded): CONVERGED in one solve, x within 1e-6 of the sparse reference over the whole vector and over
    the knots >= 8192 alone, the penalised KKT residuals <= 1e-7."""
    p = R.soft_long()
    s, run = p["s"], p["run"]
    S, C, K = D.LONG
    n = S + C
    assert run["status"] == AS.CONVERGED
    sa = P.soft_set(run["act"], p["w"])
    assert (np.flatnonzero(sa) // n >= CAP).any() and (np.flatnonzero((run["act"] != 0) & ~sa) // n >= CAP).any()
    sol = solver(S, C, K, np.float64)
    r = soft(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), dev_w(sol, [p["w"]]), s.rho, act=run["act"], max_iters=20000)
    print("solves", int(r.iters[0]), "reference", run["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED and int(r.iters[0]) == 1
    assert np.array_equal(r.act.cpu().numpy(), run["act"])
    x, y, lam = host(r.x, 1, sol.N)[0], host(r.y, 1, sol.N)[0], host(r.lam, 1, sol.sizes["sk"])[0]
    whole, tail = np.abs(x - run["x"]).max(), np.abs(x[CAP * n:] - run["x"][CAP * n:]).max()
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], x, y, lam, p["w"])
    print("x err whole", whole, "knots >= 8192", tail, "kkt", kk)
    assert whole < 1e-6 and tail < 1e-6
    assert max(kk.values()) <= 1e-7, kk


# ---- 6. gradients -----------------------------------------------------------------------------------------------------------
GRAD = [(S, C, K) for S, C in R.SHAPES for K in R.GRAD_K]


@pytest.mark.parametrize("S,C,K", GRAD, ids=["%d-%d-%d" % c for c in GRAD])
def test_soft_grad_kernel(S, C, K):
    """gato_box_qp_soft_grad on a walked problem's final act and point with a random upstream gradient and adjoint (a = 0 on
    the hard-active set, as an adjoint is), outputs at unaligned addresses, against box_qp_soft_ref.bound_grads.  Bar: the
    kernel evaluates sums of at most 2 S + C products in fp64, 1e-12 relative to the largest term is generous."""
    p = R.soft_box(S, C, K)[0]
    s, act, w, lo, hi, x = p["s"], p["run"]["act"], p["w"], p["lo"], p["hi"], p["run"]["x"]
    rng = np.random.default_rng(5)
    sa = P.soft_set(act, w)
    hard = (act != 0) & ~sa
    xbar, a, beta = rng.standard_normal(s.N), np.where(hard, 0.0, rng.standard_normal(s.N)), rng.standard_normal(S * K)
    want = P.bound_grads(p["H"], p["Cm"], act, xbar, a, beta, w, lo, hi, x)
    sol = solver(S, C, K, np.float64)
    Gb, Cb = dev_inputs(sol, [s], [(lo, hi)])[:2]
    dev = lambda v: sol.to_device(np.ascontiguousarray(v, np.float64))
    outs = [sol.new(s.N + 1).fill_(SENTINEL)[1:] for _ in range(3)]
    got = sol.box_qp_soft_grad(Gb, Cb, torch.from_numpy(act).cuda(), dev(w), dev(lo), dev(hi), dev(x), dev(xbar), dev(a), dev(beta), *outs)
    torch.cuda.synchronize()
    scale = max(1.0, np.abs(p["H"]).max() * np.abs(a).max(), np.abs(p["Cm"]).max() * np.abs(beta).max(), np.abs(w).max() * np.abs(a).max())
    for name, g, t in zip(("lo_bar", "hi_bar", "w_bar"), got, want):
        err = np.abs(g.cpu().numpy() - t).max()
        print(name, err, np.abs(t).max())
        assert err <= 1e-12 * scale * (2 * S + C), (name, err)
    assert np.any(want[2] != 0) and (not hard.any() or np.any(want[0][hard] != 0) or np.any(want[1][hard] != 0))
    assert hard.any() or (S, C, K) == (2, 1, 2)                                  # 2/1/2: its one control is not active
    # all hard (a NULL weight pointer): box_qp_bound_grad's outputs bit for bit, w_bar zero
    lb, hb = sol.box_qp_bound_grad(Gb, Cb, torch.from_numpy(act).cuda(), dev(xbar), dev(a), dev(beta))
    l2, h2, w2 = sol.box_qp_soft_grad(Gb, Cb, torch.from_numpy(act).cuda(), None, dev(lo), dev(hi), dev(x), dev(xbar), dev(a), dev(beta))
    assert torch.equal(lb, l2) and torch.equal(hb, h2) and not w2.any()


@pytest.mark.parametrize("S,C,K", R.LAYER_CASES, ids=["%d-%d-%d" % c for c in R.LAYER_CASES])
def test_layer_gradients_weights_included(S, C, K):
    import gato_python_amd
    p = R.soft_box(S, C, K)[0]
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
    assert np.abs(want["x_soft"]).max() > 0


# ---- 7. the Python surface and refusals ---------------------------------------------------------------------------------------
def test_box_qp_soft_is_the_solver_call():
    import gato_python_amd
    p = R.soft_box(6, 3, 9)[0]
    s = p["s"]
    ts = math_inputs(p)
    ts, ws = ts[:11], ts[11:]
    res = gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", x_soft=ws[0], u_soft=ws[1], **F64)
    assert int(res.status) == _lib.QP_CONVERGED and int(res.iters) == p["run"]["iters"] and res.x.shape == (s.N,)
    sol = solver(s.S, s.C, s.K, np.float64)
    direct = soft(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), dev_w(sol, [p["w"]]), s.rho)
    for name in ("x", "z", "y", "lam", "res_prim", "res_dual", "act"):
        assert getattr(res, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name
    # a number broadcasts like a bound; batched input; a warm start from the result's act is accepted on its first solve
    again = gato_python_amd.box_qp(*(t[None] for t in ts), rho=s.rho, method="pdas", x_soft=R.WEIGHT, warm=res, **F64)
    assert again.x.shape == (1, s.N) and again.iters.tolist() == [1] and again.status.tolist() == [_lib.QP_CONVERGED]
    assert again.x[0].cpu().numpy().tobytes() != b"" and np.abs(again.x[0].cpu().numpy() - p["run"]["x"]).max() < 1e-6
    for kw in (dict(method="admm"), dict(method="admm", polish=True), dict(method="pdas", polish=True)):
        with pytest.raises(ValueError, match="x_soft"):
            gato_python_amd.box_qp(*ts, rho=s.rho, x_soft=1.0, **kw, **F64)
    with pytest.raises(ValueError, match="x_soft"):
        gato_python_amd.box_qp_layer(*ts, rho=s.rho, u_soft=1.0, **F64)


def test_refusals():
    p = R.soft_box(4, 2, 9)[0]
    s, lo, hi, w = p["s"], p["lo"], p["hi"], p["w"]
    n = s.S + s.C
    sol = solver(4, 2, 9, np.float64, batch=2)
    inp = dev_inputs(sol, [s, s], [(lo, hi), (lo, hi)])
    outs = sentinels(sol)
    for j, v in ((n, np.nan), (n + s.S, -1.0), (0, np.inf), (2 * n + 1, -np.inf)):
        bad = w.copy()
        bad[j] = v
        with pytest.raises(ValueError, match=r"systems \[1\].*BAD_BOUNDS"):
            soft(sol, inp, dev_w(sol, [w, bad]), s.rho, outs=outs)
        assert sol.get_option("assembly_valid") == 0
    # the start act of a soft variable: a state of x_0, an infinite bound
    free_state = int(np.flatnonzero(~np.isfinite(lo) & (np.arange(s.N) >= n) & (w > 0))[0])
    for j, v in ((0, 1), (free_state, -1)):
        act = np.zeros((2, s.N), np.int8)
        act[1, j] = v
        with pytest.raises(ValueError, match=r"systems \[1\].*BAD_ACTIVE"):
            soft(sol, inp, dev_w(sol, [w, w]), s.rho, act=act, outs=outs)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs.values())
    # NULL pointers (d_soft_w may be NULL), a parameter out of range, a captured stream: nothing enqueued
    L = _lib.lib()
    prm = _lib.BoxQpParams()
    L.gato_box_qp_default_params(prm)
    prm.rho, prm.exit_tol, prm.max_iters = s.rho, F64["exit_tol"], F64["max_iters"]
    wd = dev_w(sol, [w, w])
    act = torch.zeros(2 * s.N, dtype=torch.int8, device="cuda")
    iters, status = sol.new(2, torch.int32).fill_(7), sol.new(2, torch.int32).fill_(7)
    res = torch.zeros(4, dtype=torch.float64, device="cuda")
    ptr = lambda t: ct.c_void_p(t.data_ptr())
    args = [ptr(t) for t in inp] + [ptr(wd), ptr(act), ct.byref(prm), 30] + [ptr(outs[k]) for k in ("x", "z", "y", "lam")] + \
           [ptr(iters), ptr(status), ptr(res), sol._stream()]
    gen = sol.get_option("assembly_gen")
    for i in range(len(args) - 1):
        if i in (6, 8, 9):                                                       # d_soft_w, the parameters (below), the count
            continue
        a2 = list(args)
        a2[i] = None
        assert L.gato_box_qp_pdas_soft(sol._h, *a2) == -1, i
    for i, v in ((8, None), (9, 0)):
        a2 = list(args)
        a2[i] = v
        assert L.gato_box_qp_pdas_soft(sol._h, *a2) == -1
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.GatoError, match="captured"):
            with torch.cuda.graph(gr, stream=st):
                _lib.check(L.gato_box_qp_pdas_soft(sol._h, *args[:-1], ct.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    assert status.tolist() == [7, 7] and sol.get_option("assembly_gen") == gen
    assert all((t == SENTINEL).all() for t in outs.values())
    assert L.gato_box_qp_pdas_soft(sol._h, *args) == 0                          # and the same arguments run
    torch.cuda.synchronize()
    assert status.tolist() == [_lib.QP_CONVERGED] * 2 and iters.tolist() == [p["run"]["iters"]] * 2
