"""Box-constrained QP solves on the device (gato_box_qp_solve, Solver.box_qp, gato_python_amd.box_qp) against the numpy
reference of tests/box_qp_ref.py: the iteration itself, converged solutions, determinism, warm starts, edge cases and the
solver state the entry leaves behind."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_ref as ref                          # noqa: E402
from box_qp_device import PARITY, admm_host, admm_run, bits, dev_inputs, rel, solver   # noqa: E402
from box_qp_polish_ref import boxes               # noqa: E402
from gato_python_amd import _lib, synth           # noqa: E402

SYN = dict(admm_rho=10.0)          # the synthetic systems' scale (Q up to 1e3) wants a stiffer penalty than the default 0.1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


# ---- 1. free bounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", [((2, 1, 5), np.float64), ((14, 7, 50), np.float64), ((14, 7, 50), np.float32)])
def test_free_bounds_is_the_whole_solve(shape, dt):
    S, C, K = shape
    s = synth.make_system(S, C, K, seed=1)
    inf = np.full(s.N, np.inf)
    a, b = solver(S, C, K, dt), solver(S, C, K, dt)
    inp = dev_inputs(a, [s], [(-inf, inf)])
    lam, dz = a.new(S * K), a.new(a.N)
    tol, eps = (1e-20, 1e-6) if dt == np.float64 else (1e-9, 1e-3)
    a.linsys_blocks(inp[0], inp[1], inp[2], inp[3], tol, 500, s.rho, lam, dz)
    r = admm_run(b, inp, s.rho, sigma=0.0, alpha=1.0, exit_tol=tol, eps_abs=eps, eps_rel=eps)
    assert int(r.iters[0]) == 1 and int(r.status[0]) == _lib.QP_CONVERGED
    assert r.x.cpu().numpy().tobytes() == dz.cpu().numpy().tobytes()
    assert r.lam.cpu().numpy().tobytes() == lam.cpu().numpy().tobytes()
    assert not r.y.any()


# ---- 2. iterate parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 5), (4, 2, 30), (14, 7, 50)])
def test_iterates_match_reference(shape):
    S, C, K = shape
    s = synth.make_system(S, C, K, seed=2) if shape != (2, 1, 5) else synth.pendulum_system()
    lo, hi = boxes(s, 3)
    sol = solver(S, C, K, np.float64)
    r = admm_run(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, **PARITY)
    got = admm_host(r, 0, sol)
    H, Cm, g, c = ref.parts(s)
    want = ref.admm(H, Cm, g, c, lo, hi, eps_abs=0.0, eps_rel=0.0, max_admm_iters=25)
    assert got["status"] == want["status"] == ref.MAX_ITERS and got["iters"] == want["iters"] == 25
    for k in ("x", "z", "y", "lam"):
        assert rel(got[k], want[k]) <= 1e-8, (k, rel(got[k], want[k]))


def test_iterates_match_reference_batch():
    S, C, K, B = 4, 2, 12, 8
    systems = [synth.make_system(S, C, K, seed=40 + b) for b in range(B)]
    bounds = [boxes(s, 50 + b, eq=b % 2 == 0) for b, s in enumerate(systems)]
    sol = solver(S, C, K, np.float64, batch=B)
    r = admm_run(sol, dev_inputs(sol, systems, bounds), systems[0].rho, **PARITY)
    for b, s in enumerate(systems):
        H, Cm, g, c = ref.parts(s)
        want = ref.admm(H, Cm, g, c, *bounds[b], eps_abs=0.0, eps_rel=0.0, max_admm_iters=25)
        got = admm_host(r, b, sol)
        assert got["iters"] == 25 and got["status"] == ref.MAX_ITERS
        for k in ("x", "z", "y", "lam"):
            assert rel(got[k], want[k]) <= 1e-8, (b, k, rel(got[k], want[k]))


# ---- 3. converged solves ---------------------------------------------------------------------------------------------
def check_converged(sol, r, b, s, lo, hi, eps):
    got = admm_host(r, b, sol)
    assert got["status"] == _lib.QP_CONVERGED, got
    H, Cm, g, c = ref.parts(s)
    rp, rd, sp, sd = ref.residuals(H, Cm, g, c, got["x"], got["z"], got["y"], got["lam"])
    tp, td = eps + eps * sp, eps + eps * sd
    slack = 1.0 if sol.np_dtype == np.float64 else 2.0            # fp32 outputs re-evaluated in fp64
    kk = ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, got["x"], got["y"], got["lam"])
    assert kk["stat"] <= slack * td and kk["eq"] <= slack * tp, (kk, tp, td)
    assert kk["bound"] <= slack * tp and kk["comp"] <= slack * tp * max(np.abs(got["y"]).max(), 1.0), kk
    zd = r.z.cpu().numpy().reshape(-1, sol.N)[b]
    lod, hid = (np.asarray(v).astype(sol.np_dtype) for v in (lo, hi))
    assert np.all(zd >= lod) and np.all(zd <= hid)
    tol = 1e-9 if sol.np_dtype == np.float64 else 1e-5
    assert abs(got["res_prim"] - rp) <= tol * max(sp, 1.0) and abs(got["res_dual"] - rd) <= tol * max(sd, 1.0), \
        (got["res_prim"], rp, got["res_dual"], rd)
    assert got["res_prim"] <= tp and got["res_dual"] <= td
    return got


@pytest.mark.parametrize("dt,eps", [(np.float64, 1e-7), (np.float32, 1e-4)])
def test_converged_solves(dt, eps):
    s, lo, hi, _ = ref.double_integrator(K=20, u_max=0.5, v_max=0.6)
    sol = solver(2, 1, 20, dt)
    r = admm_run(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, eps_abs=eps, eps_rel=eps)
    got = check_converged(sol, r, 0, s, lo, hi, eps)
    assert np.any(got["y"] != 0)
    s = synth.make_system(14, 7, 50, seed=5)
    lo, hi = boxes(s, 6)
    sol = solver(14, 7, 50, dt)
    r = admm_run(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, eps_abs=eps, eps_rel=eps, **SYN)
    check_converged(sol, r, 0, s, lo, hi, eps)


# ---- 4. determinism --------------------------------------------------------------------------------------------------
def test_check_every_and_batch_order_do_not_change_bits():
    S, C, K, B = 14, 7, 20, 16
    systems = [synth.make_system(S, C, K, seed=70 + b) for b in range(B)]
    bounds = [boxes(s, 90 + b) for b, s in enumerate(systems)]
    sol = solver(S, C, K, np.float64, batch=B)
    inp = dev_inputs(sol, systems, bounds)
    kw = dict(SYN, max_admm_iters=1000)
    r1 = admm_run(sol, inp, systems[0].rho, check_every=1, **kw)
    r25 = admm_run(sol, inp, systems[0].rho, check_every=25, **kw)
    assert bits(r1) == bits(r25)
    conv = r1.iters[r1.status == _lib.QP_CONVERGED].tolist()
    assert len(conv) >= 4 and len(set(conv)) > 1               # systems froze at different iterations
    perm = np.random.default_rng(0).permutation(B)
    rp = admm_run(sol, dev_inputs(sol, [systems[i] for i in perm], [bounds[i] for i in perm]), systems[0].rho, check_every=7, **kw)
    N, sk = sol.N, sol.sizes["sk"]
    for j, i in enumerate(perm):
        for a, b, n in ((r1.x, rp.x, N), (r1.z, rp.z, N), (r1.y, rp.y, N), (r1.lam, rp.lam, sk)):
            assert a.view(B, n)[i].cpu().numpy().tobytes() == b.view(B, n)[j].cpu().numpy().tobytes()
        assert int(r1.iters[i]) == int(rp.iters[j]) and float(r1.res_dual[i]) == float(rp.res_dual[j])


# ---- 5. warm start ---------------------------------------------------------------------------------------------------
def test_warm_start():
    s, lo, hi, blocks = ref.double_integrator(K=30, u_max=0.5)
    sol = solver(2, 1, 30, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm_run(sol, inp, s.rho)
    assert int(r.status[0]) == _lib.QP_CONVERGED
    cold_iters = int(r.iters[0])
    again = admm_run(sol, inp, s.rho, z=r.z.clone(), y=r.y.clone(), lam=r.lam.clone(), warm=True)
    assert int(again.status[0]) == _lib.QP_CONVERGED and int(again.iters[0]) <= 5, int(again.iters[0])
    # an MPC step: the initial state moves a little
    s2, _, _, _ = ref.double_integrator(K=30, u_max=0.5, x0=(0.97, -0.05))
    inp2 = dev_inputs(sol, [s2], [(lo, hi)])
    cold = admm_run(sol, inp2, s.rho)
    warm = admm_run(sol, inp2, s.rho, z=r.z.clone(), y=r.y.clone(), lam=r.lam.clone(), warm=True)
    assert int(cold.status[0]) == int(warm.status[0]) == _lib.QP_CONVERGED
    assert int(warm.iters[0]) < int(cold.iters[0]), (int(warm.iters[0]), int(cold.iters[0]), cold_iters)


def test_math_shaped_entry_and_warm_result():
    import gato_python_amd
    s, lo, hi, (Q, R, A, B, q, r, c) = ref.double_integrator(K=20, u_max=0.5, v_max=0.6)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")
    Qt = t(Q).requires_grad_(True)
    res = gato_python_amd.box_qp(Qt, t(R), t(A), t(B), t(q), t(r), t(c), t([-np.inf, -0.6]), t([np.inf, 0.6]), -0.5, 0.5,
                                 rho=s.rho, exit_tol=1e-12, max_iters=500, eps_abs=1e-7, eps_rel=1e-7)
    assert int(res.status) == _lib.QP_CONVERGED and res.x.shape == (s.N,) and res.lam.shape == (s.S * s.K,)
    assert res.x.grad_fn is None and not res.x.requires_grad
    sol = solver(2, 1, 20, np.float64)
    direct = admm_run(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, exit_tol=1e-12, eps_abs=1e-7, eps_rel=1e-7)
    assert res.x.cpu().numpy().tobytes() == direct.x.cpu().numpy().tobytes()
    again = gato_python_amd.box_qp(t(Q)[None], t(R)[None], t(A)[None], t(B)[None], t(q)[None], t(r)[None], t(c)[None],
                                   t([-np.inf, -0.6]), t([np.inf, 0.6]), -0.5, 0.5, rho=s.rho, exit_tol=1e-12,
                                   max_iters=500, eps_abs=1e-7, eps_rel=1e-7, warm=res)
    assert again.x.shape == (1, s.N) and int(again.iters[0]) <= 5


# ---- 6. edge cases ---------------------------------------------------------------------------------------------------
def test_infeasible_box_leaves_neighbours_alone():
    S, C, K = 4, 2, 10
    systems = [synth.make_system(S, C, K, seed=100 + b) for b in range(3)]
    bounds = [boxes(s, 110 + b) for b, s in enumerate(systems)]
    sol = solver(S, C, K, np.float64, batch=3)
    ok = admm_run(sol, dev_inputs(sol, systems, bounds), systems[0].rho, max_admm_iters=300, **SYN)
    bad = synth.KKTSystem(S, C, K, systems[1].G_row, systems[1].G_col, systems[1].G_val, systems[1].C_row,
                          systems[1].C_col, systems[1].C_val, systems[1].g, systems[1].c.copy(), systems[1].rho)
    bad.c[:S] = 5.0
    blo, bhi = bounds[1][0].copy(), bounds[1][1].copy()
    blo[:S], bhi[:S] = -1.0, 1.0                                    # x_0 = c_0 = 5 lies outside the box
    r = admm_run(sol, dev_inputs(sol, [systems[0], bad, systems[2]], [bounds[0], (blo, bhi), bounds[2]]), systems[0].rho,
            max_admm_iters=300, **SYN)
    assert int(r.status[1]) == _lib.QP_MAX_ITERS and int(r.iters[1]) == 300
    N, sk = sol.N, sol.sizes["sk"]
    for t, n in ((r.x, N), (r.z, N), (r.y, N), (r.lam, sk)):
        assert torch.isfinite(t.view(3, n)[1]).all()
    for b in (0, 2):
        for a, w, n in ((ok.x, r.x, N), (ok.z, r.z, N), (ok.y, r.y, N), (ok.lam, r.lam, sk)):
            assert a.view(3, n)[b].cpu().numpy().tobytes() == w.view(3, n)[b].cpu().numpy().tobytes()
        assert int(ok.iters[b]) == int(r.iters[b]) and int(ok.status[b]) == int(r.status[b])
    assert int(ok.status[0]) == _lib.QP_CONVERGED and int(ok.iters[0]) < 300


def test_bad_bounds_raise_and_trivial_qp():
    s = synth.make_system(4, 2, 8, seed=7)
    lo, hi = boxes(s, 8)
    sol = solver(4, 2, 8, np.float64, batch=2)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[s.S + 1], hi2[s.S + 1] = 1.0, -1.0
    with pytest.raises(ValueError, match=r"systems \[1\]"):
        admm_run(sol, dev_inputs(sol, [s, s], [(lo, hi), (lo2, hi2)]), s.rho)
    lo3 = lo.copy()
    lo3[s.S + 2] = np.nan
    with pytest.raises(ValueError, match=r"systems \[0\]"):
        admm_run(sol, dev_inputs(sol, [s, s], [(lo3, hi), (lo, hi)]), s.rho)
    zero = synth.KKTSystem(s.S, s.C, s.K, s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, np.zeros_like(s.g),
                           np.zeros_like(s.c), s.rho)
    r = admm_run(sol, dev_inputs(sol, [zero, s], [boxes(s, 8, eq=False), (lo, hi)]), s.rho, **SYN)   # 0 inside the box
    assert int(r.status[0]) == _lib.QP_CONVERGED and int(r.iters[0]) == 1
    N, sk = sol.N, sol.sizes["sk"]
    for t, n in ((r.x, N), (r.z, N), (r.y, N), (r.lam, sk)):
        assert not t.view(2, n)[0].any()
    assert int(r.status[1]) == _lib.QP_CONVERGED and int(r.iters[1]) > 1


# ---- 7. solver state -------------------------------------------------------------------------------------------------
def test_solver_state_and_refusals():
    s = synth.make_system(14, 7, 20, seed=9)
    lo, hi = boxes(s, 10)
    sol = solver(14, 7, 20, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    for tws in (0, 1):
        sol.set_option("true_warm_start", tws)
        gen = sol.get_option("assembly_gen")
        r = admm_run(sol, inp, s.rho, max_admm_iters=50)
        assert int(r.iters[0]) > 1
        assert sol.get_option("assembly_gen") == gen + 1
        assert sol.get_option("true_warm_start") == tws
    assert sol.box_qp_pcg_iters()[0] > 0
    # a re-solve after the call re-solves the QP's x-step matrix (no error, no re-assembly)
    gen = sol.get_option("assembly_gen")
    sol.solve_rhs(inp[2], inp[3], 1e-10, 300)
    torch.cuda.synchronize()
    assert sol.get_option("assembly_gen") == gen
    # nothing enqueued on a refusal: the outputs keep their fill
    x = sol.new(sol.N).fill_(7.0)
    torch.cuda.synchronize()

    def refused(fn):
        gen = sol.get_option("assembly_gen")
        with pytest.raises(_lib.GatoError):
            fn()
        torch.cuda.synchronize()
        assert float(x.min()) == 7.0 and float(x.max()) == 7.0 and sol.get_option("assembly_gen") == gen

    refused(lambda: sol.box_qp(*inp, rho=s.rho, exit_tol=1e-10, max_iters=100, alpha=2.0, x=x))
    refused(lambda: sol.box_qp(*inp, rho=s.rho, exit_tol=1e-10, max_iters=100, admm_rho=0.0, x=x))
    refused(lambda: sol.box_qp(*inp, rho=s.rho, exit_tol=1e-10, max_iters=100, check_every=0, x=x))
    L = _lib.lib()
    p = _lib.BoxQpParams()
    L.gato_box_qp_default_params(p)
    refused(lambda: _lib.check(L.gato_box_qp_solve(sol._h, *[ct.c_void_p(t.data_ptr()) for t in inp[:5]], None,
                                                   ct.byref(p), ct.c_void_p(x.data_ptr()), *([None] * 6), sol._stream())))
    _lib.check(L.gato_cluster_create(sol._h, 0, 1, None))
    refused(lambda: sol.box_qp(*inp, rho=s.rho, exit_tol=1e-10, max_iters=100, x=x))
    _lib.check(L.gato_cluster_destroy(sol._h))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.GatoError):
            with torch.cuda.graph(gr, stream=st):
                sol.box_qp(*inp, rho=s.rho, exit_tol=1e-10, max_iters=100, x=x)
    torch.cuda.synchronize()
    assert float(x.min()) == 7.0 and float(x.max()) == 7.0


# ---- 8. a multi-workgroup system -------------------------------------------------------------------------------------
def test_multi_workgroup_system_fp32():
    s = synth.make_system(14, 7, 512, seed=11)
    lo, hi = boxes(s, 12)
    sol = solver(14, 7, 512, np.float32)
    r = admm_run(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, eps_abs=1e-4, eps_rel=1e-4, **SYN)
    assert sol.get_option("last_groups") > 1
    check_converged(sol, r, 0, s, lo, hi, 1e-4)
