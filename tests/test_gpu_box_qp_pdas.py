"""The primal-dual active-set iteration on the device (gato_box_qp_pdas, Solver.box_qp_pdas, box_qp(method="pdas"),
box_qp(polish_iters=), box_qp_layer(method="pdas")) against the numpy reference of tests/box_qp_active_ref.py: the same number of
reduced solves and the same final active set on problems whose every decision has a margin (the seed walks,
tests/test_box_qp_pdas_cpu.py), one solve equal to the polish bit for bit, frozen systems, batches, the grid cap, fp32.
Bars: those of tests/test_gpu_box_qp_polish.py - fp64 parity 1e-6 in the infinity norm, qp_kkt_residuals <= 1e-7."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
from box_qp_device import (CAP, F64, SENTINEL, admm, check_point, cold_case, dev_inputs, fp32_case, host, math_inputs, pdas, point_bits,  # noqa: E402
                           polish, sentinels, solver, untouched)
from gato_python_amd import _lib                  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


# ---- 1. cold starts on control-only boxes -------------------------------------------------------------------------------
COLD = [(S, C, K) for S, C in D.SHAPES for K in D.COLD_K]


@pytest.mark.parametrize("S,C,K", COLD, ids=["%d-%d-%d" % c for c in COLD])
def test_cold_control_box(S, C, K):
    p = D.control_box(S, C, K)[0]
    print("seed", p["seed"], "solves", p["run"]["iters"], "margin", AS.min_margin(p["run"]))
    cold_case(p)


@pytest.mark.parametrize("name", ["pendulum", "14_7_50"])
def test_cold_named_problem(name):
    s, H, Cm, g, c, lo, hi = D.named(name)
    run = AS.iterate(H, Cm, g, c, lo, hi, s.S)
    assert run["status"] == AS.CONVERGED
    cold_case(AS.as_problem(s, H, Cm, g, c, lo, hi, run, None))


# ---- 2. constructed problems: active states, dense Q and R ----------------------------------------------------------------
CONSTRUCTED = [(S, C, K) for S, C in D.SHAPES for K in D.CONSTRUCTED_K]


@pytest.mark.parametrize("S,C,K", CONSTRUCTED, ids=["%d-%d-%d" % c for c in CONSTRUCTED])
def test_cold_constructed(S, C, K):
    p = D.constructed_cold(S, C, K)[0]
    assert np.array_equal(p["run"]["act"], p["act"])
    n = S + C
    assert ((p["act"] != 0) & (np.arange(len(p["act"])) % n < S)).any()          # an active state
    cold_case(p)


# ---- 3. one solve is the polish ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_one_solve_is_the_polish(shape):
    """max_pdas_iters = 1 from the exact act: x, z, y, lambda and the residuals of box_qp_polish on the same act, bit for bit.
    With one sign flipped: MAX_ITERS after one solve, the caller's outputs untouched, act the caller's."""
    S, C = shape
    K = 9
    p = P.constructed(S, C, K)[0]
    s = p["s"]
    a, b = solver(S, C, K, np.float64), solver(S, C, K, np.float64)
    inp = dev_inputs(a, [s], [(p["lo"], p["hi"])])
    want = admm(a, inp, s.rho, max_admm_iters=1)
    assert polish(a, inp, p["act"], want, s.rho).tolist() == [_lib.POLISH_ACCEPTED]
    got = pdas(b, inp, s.rho, act=p["act"], max_pdas_iters=1, outs=sentinels(b))
    assert int(got.status[0]) == _lib.QP_CONVERGED and int(got.iters[0]) == 1
    for name in ("x", "z", "y", "lam", "res_prim", "res_dual"):
        assert getattr(got, name).cpu().numpy().tobytes() == getattr(want, name).cpu().numpy().tobytes(), name
    assert np.array_equal(got.act.cpu().numpy(), p["act"])
    flipped, _ = P.wrong_sign(p)
    gen = b.get_option("assembly_gen")
    r = pdas(b, inp, s.rho, act=flipped, max_pdas_iters=1, outs=sentinels(b))
    assert int(r.status[0]) == _lib.QP_MAX_ITERS and int(r.iters[0]) == 1 and int(r.polished[0]) == _lib.POLISH_REJECTED
    assert untouched(r, 0, b) and np.array_equal(r.act.cpu().numpy(), flipped)
    assert b.get_option("assembly_gen") == gen + 1


# ---- 4. batches: every system as it is alone ---------------------------------------------------------------------------------
def solo_bits(p_or_sys, bounds, rho, outs=False):
    s = p_or_sys
    sol = solver(s.S, s.C, s.K, np.float64)
    r = pdas(sol, dev_inputs(sol, [s], [bounds]), rho, outs=sentinels(sol) if outs else None)
    return point_bits(r, 0, sol)


def test_batch_systems_equal_their_solo_runs():
    S, C, K, B = D.BATCH
    ps = D.control_box(S, C, K, count=B)
    want = [p["run"]["iters"] for p in ps]
    assert len(set(want)) >= 2
    sol = solver(S, C, K, np.float64, batch=B)
    r = pdas(sol, dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps]), ps[0]["s"].rho)
    assert r.iters.tolist() == want and r.status.tolist() == [_lib.QP_CONVERGED] * B
    for b, p in enumerate(ps):
        check_point(sol, r, b, p, p["run"])
        assert point_bits(r, b, sol) == solo_bits(p["s"], (p["lo"], p["hi"]), p["s"].rho), b


def test_batch_with_a_system_that_does_not_converge():
    """2/1/20 double integrators: two with bounded controls alone (different starts), between them the velocity-bounded one
    whose reduced system goes singular.  The two equal their solo runs; the third ends MAX_ITERS or NONFINITE (a singular
    Gauss-Jordan may give huge finite values) with its outputs untouched."""
    good0 = ref.double_integrator(K=20, u_max=0.5, v_max=None)
    bad = ref.double_integrator(K=20, u_max=0.5, v_max=0.57)
    good1 = ref.double_integrator(K=20, u_max=0.5, v_max=None, x0=(0.8, 0.3))
    trio = [good0, bad, good1]
    for sy in (good0, good1):
        H, Cm, g, c = ref.parts(sy[0])
        assert AS.iterate(H, Cm, g, c, sy[1], sy[2], 2)["status"] == AS.CONVERGED
    sol = solver(2, 1, 20, np.float64, batch=3)
    r = pdas(sol, dev_inputs(sol, [t[0] for t in trio], [(t[1], t[2]) for t in trio]), good0[0].rho, outs=sentinels(sol))
    print("status", r.status.tolist(), "iters", r.iters.tolist())
    assert int(r.status[1]) in (_lib.QP_MAX_ITERS, _lib.QP_NONFINITE) and untouched(r, 1, sol)
    for b in (0, 2):
        assert int(r.status[b]) == _lib.QP_CONVERGED
        assert point_bits(r, b, sol) == solo_bits(trio[b][0], (trio[b][1], trio[b][2]), good0[0].rho, outs=True), b


# ---- 5. K past the grid cap -------------------------------------------------------------------------------------------------
def test_long_horizon_second_grid_pass():
    """2/1/8197, control-only box: CONVERGED, x within 1e-6 max(1, |x|) of the sparse reference over the whole vector and over
    the knots >= 8192 alone.  Only x is compared: it is unique, act may differ where a multiplier is near 0."""
    S, C, K = D.LONG
    p = D.control_box(S, C, K, sparse=True)[0]
    s, run = p["s"], p["run"]
    n = S + C
    assert (np.flatnonzero(run["act"]) // n >= CAP).any()
    sol = solver(S, C, K, np.float64)
    r = pdas(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), s.rho, max_iters=20000)
    print("seed", p["seed"], "solves", int(r.iters[0]), "reference", run["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED
    x = host(r.x, 1, sol.N)[0]
    bar = 1e-6 * max(1.0, np.abs(run["x"]).max())
    whole, tail = np.abs(x - run["x"]).max(), np.abs(x[CAP * n:] - run["x"][CAP * n:]).max()
    print("x err whole", whole, "knots >= 8192", tail, "bar", bar)
    assert whole <= bar and tail <= bar


# ---- 6. fp32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_fp32_ends_on_the_reference_act(shape):
    S, C = shape
    K = 9
    p = D.control_box(S, C, K, f32=True)[0]
    fp32_case(p, iters=False)


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------
def test_box_qp_method_pdas_is_the_solver_call():
    import gato_python_amd
    p = D.control_box(6, 3, 9)[0]
    s = p["s"]
    ts = math_inputs(p)
    res = gato_python_amd.box_qp(*ts, rho=s.rho, method="pdas", **F64)
    assert int(res.status) == _lib.QP_CONVERGED and int(res.iters) == p["run"]["iters"] and res.x.shape == (s.N,)
    assert res.act.shape == (s.N,) and np.array_equal(res.act.cpu().numpy(), p["run"]["act"])
    sol = solver(s.S, s.C, s.K, np.float64)
    direct = pdas(sol, dev_inputs(sol, [s], [(p["lo"], p["hi"])]), s.rho)
    for name in ("x", "z", "y", "lam", "res_prim", "res_dual"):
        assert getattr(res, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name
    # warm: from the previous result's act the first solve is accepted (an MPC shift starts here)
    again = gato_python_amd.box_qp(*(t[None] for t in ts), rho=s.rho, method="pdas", warm=res, **F64)
    assert again.x.shape == (1, s.N) and again.iters.tolist() == [1] and again.status.tolist() == [_lib.QP_CONVERGED]
    with pytest.raises(ValueError, match="method"):
        gato_python_amd.box_qp(*ts, rho=s.rho, method="ipm", **F64)


def test_polish_iters_closes_what_one_polish_rejects():
    """problem("6_3_20") after 50 ADMM x-steps: one polish is rejected (the ADMM result stays), ten reduced solves converge."""
    import gato_python_amd
    s, lo, hi, arho = P.problem("6_3_20")
    H, Cm, g, c = ref.parts(s)
    ts = math_inputs(dict(s=s, lo=lo, hi=hi))
    kw = dict(rho=s.rho, admm_rho=arho, max_admm_iters=50, polish=True, **F64)
    one = gato_python_amd.box_qp(*ts, **kw)
    assert int(one.polished) == _lib.POLISH_REJECTED and int(one.status) == _lib.QP_MAX_ITERS and one.act is None
    ten = gato_python_amd.box_qp(*ts, polish_iters=10, **kw)
    assert int(ten.polished) == _lib.POLISH_ACCEPTED and int(ten.status) == _lib.QP_CONVERGED and int(ten.iters) == 50
    x, y, lam = (t.cpu().numpy() for t in (ten.x, ten.y, ten.lam))
    kk = ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam)
    xr, _, lr = P.reduced_solve(H, Cm, g, c, lo, hi, ten.act.cpu().numpy())
    print("kkt", kk, "x err", np.abs(x - xr).max())
    assert max(kk.values()) <= 1e-7 and np.abs(x - xr).max() < 1e-6 and np.abs(lam - lr).max() < 1e-6


def test_layer_method_pdas_gradients():
    import gato_python_amd
    S, C, K = 6, 3, 9
    p = D.constructed_cold(S, C, K)[0]
    s = p["s"]
    ts = math_inputs(p, requires_grad=True)
    x, lam, info = gato_python_amd.box_qp_layer(*ts, rho=s.rho, method="pdas", **F64)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and int(info.iters) == p["run"]["iters"]
    assert np.array_equal(info.act.cpu().numpy(), p["act"])
    rng = np.random.default_rng(7)
    xbar, lbar = rng.standard_normal(s.N), rng.standard_normal(S * K)
    ((x * torch.from_numpy(xbar).cuda()).sum() + (lam * torch.from_numpy(lbar).cuda()).sum()).backward()
    want = P.grads(p["H"], p["Cm"], p["act"], x.detach().cpu().numpy(), lam.detach().cpu().numpy(), xbar, lbar, S, C, K)
    for k, t in zip(("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi"), ts):
        err = np.abs(t.grad.cpu().numpy() - want[k]).max()
        print(k, err, np.abs(want[k]).max())
        assert err < 1e-6 * max(1.0, np.abs(want[k]).max()), (k, err)


def test_refusals():
    p = D.control_box(4, 2, 9)[0]
    s, lo, hi = p["s"], p["lo"], p["hi"]
    sol = solver(4, 2, 9, np.float64, batch=2)
    # bounds
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[s.S + 1], hi2[s.S + 1] = 1.0, -1.0
    outs = sentinels(sol)
    with pytest.raises(ValueError, match=r"systems \[1\].*BAD_BOUNDS"):
        pdas(sol, dev_inputs(sol, [s, s], [(lo, hi), (lo2, hi2)]), s.rho, outs=outs)
    lo3 = lo.copy()
    lo3[s.S] = np.nan
    with pytest.raises(ValueError, match=r"systems \[0\].*BAD_BOUNDS"):
        pdas(sol, dev_inputs(sol, [s, s], [(lo3, hi), (lo, hi)]), s.rho, outs=outs)
    # the start act: a state of x_0, an infinite bound (the states are free), a value that is no sign
    inp = dev_inputs(sol, [s, s], [(lo, hi), (lo, hi)])
    n = s.S + s.C
    for j, v in ((0, 1), (n, -1), (s.S, 2)):
        act = np.zeros((2, s.N), np.int8)
        act[1, j] = v
        with pytest.raises(ValueError, match=r"systems \[1\].*BAD_ACTIVE"):
            pdas(sol, inp, s.rho, act=act, outs=outs)
        assert sol.get_option("assembly_valid") == 0
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs.values())
    # NULL pointers, a parameter out of range, a captured stream: nothing enqueued
    L = _lib.lib()
    prm = _lib.BoxQpParams()
    L.gato_box_qp_default_params(prm)
    prm.rho, prm.exit_tol, prm.max_iters = s.rho, F64["exit_tol"], F64["max_iters"]
    act = torch.zeros(2 * s.N, dtype=torch.int8, device="cuda")
    iters, status = sol.new(2, torch.int32).fill_(7), sol.new(2, torch.int32).fill_(7)
    res = torch.zeros(4, dtype=torch.float64, device="cuda")
    ptr = lambda t: ct.c_void_p(t.data_ptr())
    args = [ptr(t) for t in inp] + [ptr(act), ct.byref(prm), 30] + [ptr(outs[k]) for k in ("x", "z", "y", "lam")] + \
           [ptr(iters), ptr(status), ptr(res), sol._stream()]
    gen = sol.get_option("assembly_gen")
    for i in range(len(args) - 1):
        if i in (7, 8):
            continue
        a2 = list(args)
        a2[i] = None
        assert L.gato_box_qp_pdas(sol._h, *a2) == -1
    a2 = list(args)
    a2[8] = 0
    assert L.gato_box_qp_pdas(sol._h, *a2) == -1
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.GatoError, match="captured"):
            with torch.cuda.graph(gr, stream=st):
                _lib.check(L.gato_box_qp_pdas(sol._h, *args[:-1], ct.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    assert status.tolist() == [7, 7] and sol.get_option("assembly_gen") == gen
    assert all((t == SENTINEL).all() for t in outs.values())
    assert L.gato_box_qp_pdas(sol._h, *args) == 0                               # and the same arguments run
    torch.cuda.synchronize()
    assert status.tolist() == [_lib.QP_CONVERGED] * 2 and iters.tolist() == [p["run"]["iters"]] * 2
