"""Box-QP polish and the differentiable layer on the device (gato_box_qp_active_set / _polish / _bound_grad, Solver.box_qp_polish,
gato_python_amd.box_qp(polish=True), gato_python_amd.box_qp_layer) against the numpy reference of tests/box_qp_polish_ref.py:
polished solutions from a given and from an ADMM active set, rejected guesses left bit for bit, free bounds, batches, gradients
and refusals.  Bars: fp64 parity 1e-6 in the infinity norm, qp_kkt_residuals <= 1e-7; fp32 by tests/f32_parity.py."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
from box_qp_device import F64, admm, bits, check_polished, dev_inputs, host, polish, solver   # noqa: E402
from f32_parity import check_f32                  # noqa: E402
from gato_python_amd import _lib, synth           # noqa: E402
from oracle import gato_oracle as o               # noqa: E402

_EXACT = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def exact(name):
    if name not in _EXACT:
        _EXACT[name] = P.exact_active(name)
    return _EXACT[name]


# ---- 1. the exact active set given ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.PROBLEMS)
def test_exact_active_set_f64(name):
    e = exact(name)
    act, lo, hi = e[0], e[5], e[6]
    s, _, _, arho = P.problem(name)
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, admm_rho=arho, max_admm_iters=1)
    gen = sol.get_option("assembly_gen")
    codes = polish(sol, inp, act, r, s.rho)
    assert codes.tolist() == [_lib.POLISH_ACCEPTED]
    assert sol.get_option("assembly_gen") == gen + 1 and sol.get_option("assembly_valid") == 1
    check_polished(sol, r, 0, e, act)


# ---- 2. ADMM stopped early, then polished -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,its", [("pendulum", 10), ("pendulum", 25), ("pendulum", 50), ("6_3_20", 1200),
                                      ("6_3_20", 1500), ("6_3_20", 2000)])
def test_admm_then_polish(name, its):
    e = exact(name)
    act, lo, hi = e[0], e[5], e[6]
    s, _, _, arho = P.problem(name)
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, admm_rho=arho, max_admm_iters=its)
    assert int(r.status[0]) == _lib.QP_MAX_ITERS
    act_d = sol.box_qp_active_set(r.z, r.y, inp[4], inp[5])
    assert np.array_equal(act_d.cpu().numpy(), act)
    codes = polish(sol, inp, act_d, r, s.rho)
    assert codes.tolist() == [_lib.POLISH_ACCEPTED]
    check_polished(sol, r, 0, e, act)


def test_box_qp_polish_flag():
    """gato_python_amd.box_qp(polish=True) on the 6/3/20 problem, where plain ADMM ends in MAX_ITERS; without the flag
    the result is what it was (polished None)."""
    import gato_python_amd
    e = exact("6_3_20")
    s, lo, hi, arho = P.problem("6_3_20")
    Q, R, A, B, q, r_, c = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in kgr.blocks_of(s))
    xl, ul = (torch.from_numpy(t).cuda() for t in P.split_states_controls(lo, s.S, s.C, s.K))
    xh, uh = (torch.from_numpy(t).cuda() for t in P.split_states_controls(hi, s.S, s.C, s.K))
    kw = dict(rho=s.rho, exit_tol=1e-20, max_iters=1000, admm_rho=arho, max_admm_iters=1500)
    plain = gato_python_amd.box_qp(Q, R, A, B, q, r_, c, xl, xh, ul, uh, **kw)
    assert plain.polished is None and int(plain.status) == _lib.QP_MAX_ITERS
    res = gato_python_amd.box_qp(Q, R, A, B, q, r_, c, xl, xh, ul, uh, polish=True, **kw)
    assert int(res.polished) == _lib.POLISH_ACCEPTED and int(res.status) == _lib.QP_CONVERGED
    xr, _, lr = P.reduced_solve(*e[1:7], e[0])
    assert np.abs(res.x.cpu().numpy() - xr).max() < 1e-6 and np.abs(res.lam.cpu().numpy() - lr).max() < 1e-6


# ---- 3. a wrong guess is left bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,its", [("pendulum", 1), ("pendulum", 2), ("pendulum", 3), ("pendulum", 4), ("pendulum", 5),
                                      ("6_3_20", 100)])
def test_rejected_guess_leaves_admm_result(name, its):
    s, lo, hi, arho = P.problem(name)
    H, Cm, g, c = ref.parts(s)
    want = ref.admm(H, Cm, g, c, lo, hi, admm_rho=arho, eps_abs=0.0, eps_rel=0.0, max_admm_iters=its)
    pr = P.polish(H, Cm, g, c, lo, hi, want["z"], want["y"], s.S)
    assert pr["decision"] == P.REJECTED
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, admm_rho=arho, eps_abs=0.0, eps_rel=0.0, max_admm_iters=its)
    before = bits(r)
    act_d = sol.box_qp_active_set(r.z, r.y, inp[4], inp[5])
    assert np.array_equal(act_d.cpu().numpy(), pr["act"])
    codes = polish(sol, inp, act_d, r, s.rho)
    assert codes.tolist() == [_lib.POLISH_REJECTED]
    assert bits(r) == before


# ---- 4. free bounds: the whole solve's bits -----------------------------------------------------------------------------
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
    r = admm(b, inp, s.rho, max_admm_iters=1, exit_tol=tol, max_iters=500)
    codes = polish(b, inp, np.zeros(s.N, np.int8), r, s.rho, eps=eps, exit_tol=tol, max_iters=500)
    assert codes.tolist() == [_lib.POLISH_ACCEPTED]
    assert r.x.cpu().numpy().tobytes() == dz.cpu().numpy().tobytes()
    assert r.lam.cpu().numpy().tobytes() == lam.cpu().numpy().tobytes()
    assert r.z.cpu().numpy().tobytes() == dz.cpu().numpy().tobytes() and not r.y.any()


# ---- 5. a batch ---------------------------------------------------------------------------------------------------------
def test_batch_decisions_and_permutation():
    """Four copies of the 6/3/20 problem (its box has a lo == hi control) with the exact active set, the exact set with an
    active control freed (a bound violation), with an upper bound swapped for the lower one, and the exact set again on a
    shifted right-hand side: each system's decision is the reference's, and permuting the systems permutes the bits."""
    act0, H, Cm, g, c, lo, hi = exact("6_3_20")
    s, _, _, arho = P.problem("6_3_20")
    A = np.nonzero(act0)[0]
    up = A[act0[A] > 0]
    a_free, a_flip = act0.copy(), act0.copy()
    a_free[up[0]] = 0
    a_flip[up[-1]] = -1
    s3 = synth.make_system(6, 3, 20, seed=2)
    s3.g = s3.g * 1.001
    systems, acts = [s, s, s, s3], [act0, a_free, a_flip, act0]
    want = []
    for sy, a in zip(systems, acts):
        Hs, Cs, gs, cs = ref.parts(sy)
        want.append(P.polish(Hs, Cs, gs, cs, lo, hi, np.zeros(sy.N), np.zeros(sy.N), s.S, act=a)["decision"])
    print("reference decisions", want)
    assert P.ACCEPTED in want and P.REJECTED in want
    outs = []
    for perm in ([0, 1, 2, 3], [2, 0, 3, 1]):
        sol = solver(6, 3, 20, np.float64, batch=4)
        inp = dev_inputs(sol, [systems[i] for i in perm], [(lo, hi)] * 4)
        r = admm(sol, inp, s.rho, admm_rho=arho, max_admm_iters=300)
        before = [host(t, 4, n) for t, n in ((r.x, sol.N), (r.lam, sol.sizes["sk"]))]
        codes = polish(sol, inp, np.stack([acts[i] for i in perm]), r, s.rho)
        assert codes.tolist() == [want[i] for i in perm]
        for j, i in enumerate(perm):
            if want[i] == P.REJECTED:
                assert np.array_equal(host(r.x, 4, sol.N)[j], before[0][j]) and np.array_equal(host(r.lam, 4, sol.sizes["sk"])[j], before[1][j])
            else:
                check_polished(sol, r, j, (None,) + tuple(ref.parts(systems[i])) + (lo, hi), acts[i])
        outs.append((perm, [t.cpu().numpy().reshape(4, -1) for t in (r.x, r.z, r.y, r.lam)], codes))
    (p0, o0, c0), (p1, o1, c1) = outs
    for j, i in enumerate(p1):
        for t0, t1 in zip(o0, o1):
            assert t0[i].tobytes() == t1[j].tobytes()


# ---- 6. the differentiable layer ----------------------------------------------------------------------------------------
def layer_inputs(name, requires_grad=True):
    s, lo, hi, arho = P.problem(name)
    blocks = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in kgr.blocks_of(s)]
    bounds = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in
              (*P.split_states_controls(lo, s.S, s.C, s.K)[:1], *P.split_states_controls(hi, s.S, s.C, s.K)[:1],
               P.split_states_controls(lo, s.S, s.C, s.K)[1], P.split_states_controls(hi, s.S, s.C, s.K)[1])]
    ts = blocks + bounds
    for t in ts:
        t.requires_grad_(requires_grad)
    return s, ts, arho


KEYS = ("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi")


def layer_grads_vs_reference(name, ts, s, arho, rng):
    import gato_python_amd
    x, lam, info = gato_python_amd.box_qp_layer(*ts, rho=s.rho, exit_tol=1e-20, max_iters=1000, admm_rho=arho)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and info.x.grad_fn is None
    act, H, Cm, g, c, lo, hi = exact(name)
    xbar, lbar = rng.standard_normal(x.shape[-1]), rng.standard_normal(lam.shape[-1])
    loss = (x * torch.from_numpy(xbar).cuda()).sum() + (lam * torch.from_numpy(lbar).cuda()).sum()
    return loss, x, lam, act, H, Cm, xbar, lbar


@pytest.mark.parametrize("name", P.PROBLEMS)
def test_layer_gradients_match_reference(name):
    s, ts, arho = layer_inputs(name)
    loss, x, lam, act, H, Cm, xbar, lbar = layer_grads_vs_reference(name, ts, s, arho, np.random.default_rng(3))
    loss.backward()
    want = P.grads(H, Cm, act, x.detach().cpu().numpy(), lam.detach().cpu().numpy(), xbar, lbar, s.S, s.C, s.K)
    for k, t in zip(KEYS, ts):
        err = np.abs(t.grad.cpu().numpy() - want[k]).max()
        print(name, k, err, np.abs(want[k]).max())
        assert err < 1e-6 * max(1.0, np.abs(want[k]).max()), (k, err)


def test_layer_gradient_after_another_forward():
    import gato_python_amd
    s, ts, arho = layer_inputs("14_7_50")
    loss, x, lam, act, H, Cm, xbar, lbar = layer_grads_vs_reference("14_7_50", ts, s, arho, np.random.default_rng(5))
    s2, ts2, _ = layer_inputs("14_7_50", requires_grad=False)
    with torch.no_grad():
        ts2[6].mul_(0.5)                                              # another c, same shape: the cached solver re-assembles
    gato_python_amd.box_qp_layer(*ts2, rho=s.rho, exit_tol=1e-20, max_iters=1000, admm_rho=arho)
    loss.backward()
    want = P.grads(H, Cm, act, x.detach().cpu().numpy(), lam.detach().cpu().numpy(), xbar, lbar, s.S, s.C, s.K)
    for k, t in zip(KEYS, ts):
        assert np.abs(t.grad.cpu().numpy() - want[k]).max() < 1e-6 * max(1.0, np.abs(want[k]).max()), k


def test_layer_rejected_polish_raises():
    import gato_python_amd
    s, ts, arho = layer_inputs("pendulum")
    x, lam, info = gato_python_amd.box_qp_layer(*ts, rho=s.rho, exit_tol=1e-20, max_iters=1000, eps_abs=0.0, eps_rel=0.0,
                                                max_admm_iters=3)
    assert int(info.polished) == _lib.POLISH_REJECTED
    with pytest.raises(RuntimeError, match="not accepted"):
        (x.sum() + lam.sum()).backward(retain_graph=True)
    (0.0 * x.sum()).backward()                                       # a zero upstream gradient: zeros, no re-solve
    assert all(t.grad is not None and not t.grad.any() for t in ts)


def _small_di():
    """A double integrator small enough for gradcheck: K = 8, |u| <= 0.5, |v| <= 0.8 (states bounded too)."""
    return ref.double_integrator(K=8, u_max=0.5, v_max=0.8)


def test_layer_gradcheck_small_double_integrator():
    """torch.autograd.gradcheck on a K = 8 double integrator; its margins (free coordinates from their bounds, active
    multipliers from zero) are checked on the CPU first, so that gradcheck's steps of 1e-6 keep the active set."""
    import gato_python_amd
    s, lo, hi, blocks = _small_di()
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, eps_abs=0.0, eps_rel=0.0, max_admm_iters=3000)
    act = P.active_set(out["z"], out["y"], lo, hi, s.S)
    x, y, lam = P.reduced_solve(H, Cm, g, c, lo, hi, act)
    assert max(ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam).values()) <= 1e-9
    F, eq = act == 0, lo == hi
    with np.errstate(invalid="ignore"):
        mfree = np.min(np.minimum(x - lo, hi - x)[F])
    ymin = np.abs(y[(act != 0) & ~eq]).min()
    print("margins", mfree, ymin, int((act != 0).sum()))
    assert (act != 0).any() and mfree > 1e-3 and ymin > 1e-3
    S, C, K = s.S, s.C, s.K
    ts = [torch.from_numpy(np.ascontiguousarray(t, np.float64)).cuda().requires_grad_() for t in blocks]
    bnd = [torch.from_numpy(np.ascontiguousarray(t)).cuda().requires_grad_() for t in
           (P.split_states_controls(lo, S, C, K)[0], P.split_states_controls(hi, S, C, K)[0],
            P.split_states_controls(lo, S, C, K)[1], P.split_states_controls(hi, S, C, K)[1])]

    def f(*a):                           # Q, R symmetrised: the layer takes them as symmetric
        sym = lambda t: 0.5 * (t + t.transpose(-1, -2))
        xx, ll, info = gato_python_amd.box_qp_layer(sym(a[0]), sym(a[1]), *a[2:], rho=s.rho, exit_tol=1e-22, max_iters=1000,
                                                    max_admm_iters=4000)
        assert int(info.polished) == _lib.POLISH_ACCEPTED
        return xx, ll

    assert torch.autograd.gradcheck(f, tuple(ts + bnd), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_layer_batch_of_64():
    """64 control-boxed 14/7/50 systems in one call against per-system references (the reference's reduced solve on the
    active set of the returned point, itself checked as a KKT point of the QP)."""
    import gato_python_amd
    Bn = 64
    systems = [synth.make_system(14, 7, 50, seed=100 + b) for b in range(Bn)]
    bounds = [P.boxes(sy, 200 + b, eq=False, states=False) for b, sy in enumerate(systems)]
    S, C, K = 14, 7, 50
    mats = [kgr.blocks_of(sy) for sy in systems]
    ts = [torch.from_numpy(np.stack([m[i] for m in mats])).cuda().requires_grad_() for i in range(7)]
    bnd = [torch.from_numpy(np.stack([P.split_states_controls(b[j], S, C, K)[i] for b in bounds])).cuda().requires_grad_()
           for i, j in ((0, 0), (0, 1), (1, 0), (1, 1))]
    x, lam, info = gato_python_amd.box_qp_layer(*ts, *bnd, rho=systems[0].rho, exit_tol=1e-20, max_iters=1000, admm_rho=1.0)
    assert info.polished.tolist() == [_lib.POLISH_ACCEPTED] * Bn
    rng = np.random.default_rng(11)
    xbar, lbar = rng.standard_normal(tuple(x.shape)), rng.standard_normal(tuple(lam.shape))
    ((x * torch.from_numpy(xbar).cuda()).sum() + (lam * torch.from_numpy(lbar).cuda()).sum()).backward()
    xs, zs, ys, ls = (t.cpu().numpy() for t in (x.detach(), info.z, info.y, lam.detach()))
    for b in range(Bn):
        lo, hi = bounds[b]
        H, Cm, g, c = ref.parts(systems[b])
        act = P.active_set(zs[b], ys[b], lo, hi, S)
        xr, yr, lr = P.reduced_solve(H, Cm, g, c, lo, hi, act)
        assert max(ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, xr, yr, lr).values()) <= 1e-7, b
        assert np.abs(xs[b] - xr).max() < 1e-6 and np.abs(ls[b] - lr).max() < 1e-6, b
        want = P.grads(H, Cm, act, xs[b], ls[b], xbar[b], lbar[b], S, C, K)
        for k, t in zip(KEYS, ts + bnd):
            err = np.abs(t.grad[b].cpu().numpy() - want[k]).max()
            assert err < 1e-6 * max(1.0, np.abs(want[k]).max()), (b, k, err)


# ---- 7. fp32 against the fp32 oracle ------------------------------------------------------------------------------------
def test_fp32_control_boxes_beside_the_oracle():
    """With only controls bounded the reduced system is an ordinary one: R_k's active rows and columns the identity, B_k's
    active columns 0, the right-hand side shifted (g'_A = 0).  The fp32 oracle solves it; the polish is held to
    err_gpu <= 2 err_oracle + 5e-6 against the fp64 dense reduced solve on the fp32-rounded inputs."""
    act, *_ = exact("14_7_50")
    s, lo, hi, arho = P.problem("14_7_50")
    S, C, K, n = s.S, s.C, s.K, s.S + s.C
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    Q, R, A, B, q, r, c = (f32(t) for t in kgr.blocks_of(s))
    lo32, hi32 = f32(lo), f32(hi)
    rho = float(np.float32(s.rho))
    H, Cm, g, cc = P.dense_from_blocks(Q, R, A, B, q, r, c, rho)
    xt, _, lt = P.reduced_solve(H, Cm, g, cc, lo32, hi32, act)
    # the ordinary system of the oracle, in fp32
    b = P.bound_values(act, lo32, hi32)
    on = act != 0
    Rr, Br = R.copy(), B.copy()
    for k in range(K - 1):
        a = on[k * n + S: (k + 1) * n]
        Rr[k][a, :] = 0.0
        Rr[k][:, a] = 0.0
        Rr[k][a, a] = 1.0
        Br[k][:, a] = 0.0
    gp = g - H[:, on] @ b[on]
    gp[on] = 0.0
    cp = cc - Cm[:, on] @ b[on]
    Qr = Q + rho * np.eye(S)
    Rr = Rr + rho * np.eye(C) * (~on[np.arange(K - 1)[:, None] * n + S + np.arange(C)])[:, None, :]
    Gd32 = o.pack_G(Qr, Rr).astype(np.float32)
    Cd32 = kgr.pack_C(A, Br).astype(np.float32)
    S_bd, P_bd, gam, Ginv = o.form_schur(Gd32, Cd32, gp.astype(np.float32), cp.astype(np.float32), S, C, K)
    P_bd = o.form_ss(S_bd, P_bd, S, K)
    lam_o, _ = o.pcg(S_bd, P_bd, gam, S, K, 1e-8, 1000)[:2]
    dz_o = o.compute_dz(Ginv, Cd32, gp.astype(np.float32), lam_o, S, C, K)
    x_o = np.where(on, b, dz_o)
    sol = solver(S, C, K, np.float32)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, admm_rho=arho, max_admm_iters=1)
    codes = polish(sol, inp, act, r, s.rho, eps=1e-4, exit_tol=1e-8, max_iters=1000)
    assert codes.tolist() == [_lib.POLISH_ACCEPTED]
    x, lam = r.x.cpu().numpy(), r.lam.cpu().numpy()
    assert np.array_equal(x[on], b[on].astype(np.float32))
    check_f32("polish x 14/7/50 control box", x, x_o, xt)
    check_f32("polish lam 14/7/50 control box", lam, lam_o, lt)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_bad_active_and_refusals():
    s, lo, hi, arho = P.problem("pendulum")
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, admm_rho=arho, max_admm_iters=20)
    act = sol.box_qp_active_set(r.z, r.y, inp[4], inp[5])
    torch.cuda.synchronize()
    before = bits(r)
    for i in (0, 1):                     # the states of x_0
        bad = act.clone()
        bad[i] = 1
        with pytest.raises(ValueError, match="BAD_ACTIVE"):
            sol.box_qp_polish(*inp, bad, r, rho=s.rho, **F64)
        assert bits(r) == before and sol.get_option("assembly_valid") == 0
    bad = act.clone()
    bad[s.S + s.C] = 1                   # a state of x_1: infinite bounds in the pendulum's box
    with pytest.raises(ValueError, match="BAD_ACTIVE"):
        sol.box_qp_polish(*inp, bad, r, rho=s.rho, **F64)
    assert bits(r) == before
    L = _lib.lib()
    p = _lib.BoxQpParams()
    L.gato_box_qp_default_params(p)
    codes = sol.new(1, torch.int32).fill_(7)
    res2 = r.res_prim._base
    ptr = lambda t: ct.c_void_p(t.data_ptr())
    args = [ptr(t) for t in inp] + [ptr(act), ct.byref(p), ptr(r.x), ptr(r.z), ptr(r.y), ptr(r.lam), ptr(r.status), ptr(res2),
                                     ptr(codes), sol._stream()]
    torch.cuda.synchronize()

    def refused(call):
        gen = sol.get_option("assembly_gen")
        assert call() == -1
        torch.cuda.synchronize()
        assert bits(r) == before and int(codes[0]) == 7 and sol.get_option("assembly_gen") == gen

    for i in range(len(args) - 1):
        if i == 7:
            continue                     # the params struct
        a2 = list(args)
        a2[i] = None
        refused(lambda: L.gato_box_qp_polish(sol._h, *a2))
    assert L.gato_box_qp_active_set(sol._h, None, ptr(r.y), ptr(inp[4]), ptr(inp[5]), ptr(act), sol._stream()) == -1
    assert L.gato_box_qp_bound_grad(sol._h, ptr(inp[0]), ptr(inp[1]), ptr(act), None, ptr(r.x), ptr(r.lam), ptr(r.x),
                                    ptr(r.x), sol._stream()) == -1
    _lib.check(L.gato_cluster_create(sol._h, 0, 1, None))
    refused(lambda: L.gato_box_qp_polish(sol._h, *args))
    assert L.gato_box_qp_active_set(sol._h, ptr(r.z), ptr(r.y), ptr(inp[4]), ptr(inp[5]), ptr(act), sol._stream()) == -1
    _lib.check(L.gato_cluster_destroy(sol._h))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.GatoError):
            with torch.cuda.graph(gr, stream=st):
                _lib.check(L.gato_box_qp_polish(sol._h, *args[:-1], ct.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    assert bits(r) == before and int(codes[0]) == 7
