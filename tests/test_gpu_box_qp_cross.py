"""Box QPs with a state-control cross term on the device (gato_box_qp_solve_cross, Solver.box_qp_cross, box_qp(M=...); DESIGN.md
section 3.16) against box_qp_ref.admm on the dense H with M in place (tests/box_qp_cross_ref.py): the iteration itself at every
shape and knot edge, degenerate M, converged solutions, determinism, the knot stride, unaligned arrays, warm starts, frozen
systems, the solver state the entry leaves behind and the math-shaped entry.  tests/test_box_qp_cross_cpu.py shows on the CPU
that these problems tell an iteration with M from one without, and that the reference meets the converged cases' caps."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_cross_ref as XR                     # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import cross_ref as X                             # noqa: E402
from box_qp_device import CAP, PARITY, SENTINEL, admm_host, admm_run, bits, dev_inputs, rel, sentinels, solver   # noqa: E402
from gato_python_amd import _lib, synth           # noqa: E402

RHO = XR.RHO
SYN = dict(admm_rho=XR.ADMM_RHO)
key_id = lambda k: "%d-%d-%d" % k[:3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def dev_M(sol, Ms):
    return sol.to_device(np.concatenate([X.pack_M(M) for M in Ms]).astype(sol.np_dtype))


def inputs(sol, ps):
    """(G, C, g, c, lo, hi) of dev_inputs and M_blocks of the problems ps, stacked."""
    return dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps]), dev_M(sol, [p["M"] for p in ps])


def cross_run(sol, inp, Mb, **kw):
    """Solver.box_qp_cross at the ADMM tests' PCG settings (box_qp_device.admm_run's)."""
    kw.setdefault("exit_tol", 1e-16 if sol.np_dtype == np.float64 else 1e-8)
    kw.setdefault("max_iters", 500)
    r = sol.box_qp_cross(inp[0], Mb, *inp[1:], rho=RHO, **kw)
    torch.cuda.synchronize()
    return r


def system_bits(r, b, sol):
    B = sol.batch
    return [t.cpu().numpy().reshape(B, -1)[b].tobytes() for t in (r.x, r.z, r.y, r.lam, r.iters, r.status, r.res_prim, r.res_dual)]


# ---- 1. iterate parity: the kernel's main test ---------------------------------------------------------------------------------
def check_parity(got, want, iters, tag):
    assert got["status"] == want["status"] == ref.MAX_ITERS and got["iters"] == want["iters"] == iters
    rels = {k: rel(got[k], want[k]) for k in ("x", "z", "y", "lam")}
    print(tag, rels)
    for k, v in rels.items():
        assert v <= 1e-8, (tag, k, v)


@pytest.mark.parametrize("key", XR.parity_keys(), ids=key_id)
def test_iterates_match_reference(key):
    """25 iterations at eps 0 against the reference on the cross H, full boxes (state clips, one lo == hi control): 1e-8, the
    bar of test_gpu_box_qp.py's test of the same name."""
    S, C, K = key[:3]
    p = XR.problem(*key)
    sol = solver(S, C, K, np.float64)
    inp, Mb = inputs(sol, [p])
    r = cross_run(sol, inp, Mb, **PARITY)
    want = XR.parity_reference(key)
    assert np.any(want["y"] != 0) and np.any(want["z"] != want["x"])
    check_parity(admm_host(r, 0, sol), want, XR.PARITY_ITERS, key_id(key))


def test_iterates_match_reference_batch():
    """B = 3 different systems in one call: one with dense Q blocks, one with M = 0."""
    keys = XR.batch_keys()
    S, C, K = keys[0][:3]
    ps = [XR.problem(*k) for k in keys]
    sol = solver(S, C, K, np.float64, batch=3)
    inp, Mb = inputs(sol, ps)
    r = cross_run(sol, inp, Mb, **PARITY)
    for b, k in enumerate(keys):
        check_parity(admm_host(r, b, sol), XR.parity_reference(k), XR.PARITY_ITERS, "system %d" % b)


# ---- 2. degenerate M ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [(4, 2, 3), (14, 7, 9)], ids=lambda c: "%d-%d-%d" % c)
def test_zero_M_is_box_qp(cell):
    """M = 0: W = 0, the transformed blocks are the caller's and every term the kernel adds is a fused multiply-add of a zero
    product - the values of Solver.box_qp (array_equal: the sign of a zero may differ)."""
    S, C, K = cell
    p = XR.problem(S, C, K, 3, False, "full", True)
    a, b = solver(S, C, K, np.float64), solver(S, C, K, np.float64)
    inp, Mb = inputs(a, [p])
    assert not Mb.any()
    kw = dict(SYN, max_admm_iters=60)
    got = cross_run(a, inp, Mb, **kw)
    want = admm_run(b, inp, RHO, **kw)
    assert int(want.iters[0]) > 5
    for name in ("x", "z", "y", "lam", "iters", "status", "res_prim", "res_dual"):
        g, w = getattr(got, name).cpu().numpy(), getattr(want, name).cpu().numpy()
        assert np.array_equal(g, w), (name, np.abs(g - w).max())
    assert a.box_qp_pcg_iters().tolist() == b.box_qp_pcg_iters().tolist()


def test_one_knot_without_M_is_box_qp():
    """K = 1 has no M: Mb=None (a NULL d_M_blocks) gives the bits of box_qp."""
    S, C = 4, 2
    Q, _, _, _, q, _, c = synth.make_blocks(S, C, 1, seed=5, dense_q=True)
    a, b = solver(S, C, 1, np.float64), solver(S, C, 1, np.float64)
    d = lambda v: a.to_device(np.asarray(v, np.float64).reshape(-1))
    x0 = c[0] + np.array([0.3, -0.2, 0.1, 0.4])                          # the box holds x_0 = c_0 and cuts none of it off
    inp = (d(Q[0].T), a.new(0), d(q[0]), d(c[0]), d(np.minimum(x0, c[0]) - 0.5), d(np.maximum(x0, c[0]) + 0.5))
    got = a.box_qp_cross(inp[0], None, *inp[1:], rho=RHO, exit_tol=1e-16, max_iters=100)
    want = b.box_qp(*inp, rho=RHO, exit_tol=1e-16, max_iters=100)
    torch.cuda.synchronize()
    assert int(want.status[0]) == _lib.QP_CONVERGED
    assert bits(got) == bits(want)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_fused_maps_equal_the_launches_they_replace(dt):
    """Option qp_cross_unfused = 1 runs cross_finish and cross_rhs as launches of their own around every re-solve and gives the
    update kernel a W of zeros: the maps the kernel fuses are those kernels' chains, so every output has the same value
    (array_equal: a product with a zero W may change the sign of a zero) and the PCG does the same work."""
    keys = XR.batch_keys()
    S, C, K = keys[0][:3]
    ps = [XR.problem(*k) for k in keys]
    a, b = solver(S, C, K, dt, batch=3), solver(S, C, K, dt, batch=3)
    b.set_option("qp_cross_unfused", 1)
    inp, Mb = inputs(a, ps)
    kw = dict(SYN, max_admm_iters=40, eps_abs=0.0, eps_rel=0.0)
    fused, unfused = cross_run(a, inp, Mb, **kw), cross_run(b, inp, Mb, **kw)
    assert fused.iters.tolist() == [40] * 3
    for name in ("x", "z", "y", "lam", "iters", "status", "res_prim", "res_dual"):
        g, w = getattr(fused, name).cpu().numpy(), getattr(unfused, name).cpu().numpy()
        assert np.array_equal(g, w), (name, np.abs(g - w).max())
    assert a.box_qp_pcg_iters().tolist() == b.box_qp_pcg_iters().tolist()


# ---- 3. converged solves -------------------------------------------------------------------------------------------------------
def check_converged(sol, r, b, p, eps):
    """test_gpu_box_qp.py's check_converged, restated with the cross H: a reported residual formed with an H x without M misses
    the agreement with ref.residuals."""
    got = admm_host(r, b, sol)
    assert got["status"] == _lib.QP_CONVERGED, got
    H, Cm, g, c, lo, hi = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi"))
    rp, rd, sp, sd = ref.residuals(H, Cm, g, c, got["x"], got["z"], got["y"], got["lam"])
    tp, td = eps + eps * sp, eps + eps * sd
    slack = 1.0 if sol.np_dtype == np.float64 else 2.0            # fp32 outputs re-evaluated in fp64
    kk = ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, got["x"], got["y"], got["lam"])
    print("iters", got["iters"], "kkt", kk, "tol", tp, td, "res", got["res_prim"], rp, got["res_dual"], rd)
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


# The PCG exit tolerance of the fp32 converged cases.  The PCG stops on |r^T P r| < exit_tol (absolute; P ~ S^-1, S = C G'^-1 C^T the
# Schur complement), which bounds the x-step's equality residual |C x - c| = |r| only by sqrt(exit_tol lambda_max(S)).  The free
# states of these cells have G' ~ Q >= 0.1, so lambda_max(S) is 20 and more: at exit_tol = 1e-8 that is 4.5e-4, above the primal
# bar eps (1 + |x|) = 2.3e-4 of 2/1/3 at eps = 1e-4 - whether the ADMM test then passes is left to the rounding (measured on
# 2/1/3 with M: res_prim wanders between 3.5e-4 and 7.3e-4 over 1000 iterations and a torch ADMM loop over whole cross solves at
# 1e-8 does the same; without M it happens to stop at 6e-5).  An x-step error a tenth of the bar needs exit_tol <= (1e-5)^2 / 20 =
# 5e-12.  At 1e-12 the device converges in the reference's 21 .. 22 iterations.
F32_EXIT_TOL = 1e-12


@pytest.mark.parametrize("dt,eps", [(np.float64, 1e-7), (np.float32, 1e-4)], ids=["fp64", "fp32"])
@pytest.mark.parametrize("key", XR.converged_keys(seeds=(0,)), ids=key_id)
def test_converged_solves(key, dt, eps):
    """Control-only boxes at admm_rho = 10 (with bounded states many of these cells do not converge in 4000 iterations).
    The fp32 x-steps run at the PCG exit tolerance F32_EXIT_TOL, not at the other fp32 tests' 1e-8: see there."""
    S, C, K = key[:3]
    p = XR.problem(*key)
    sol = solver(S, C, K, dt)
    inp, Mb = inputs(sol, [p])
    pcg = dict(exit_tol=F32_EXIT_TOL) if dt == np.float32 else {}
    r = cross_run(sol, inp, Mb, eps_abs=eps, eps_rel=eps, **pcg, **SYN)
    got = check_converged(sol, r, 0, p, eps)
    assert np.any(got["y"] != 0)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------
def test_same_bits_twice_for_every_check_every_and_batch_order():
    S, C, K, B = 14, 7, 9, 6
    ps = [XR.problem(S, C, K, 17 * b, False, "controls") for b in range(B)]
    sol = solver(S, C, K, np.float64, batch=B)
    inp, Mb = inputs(sol, ps)
    kw = dict(SYN, max_admm_iters=1000)
    r1 = cross_run(sol, inp, Mb, check_every=1, **kw)
    again = cross_run(sol, inp, Mb, check_every=1, **kw)
    r25 = cross_run(sol, inp, Mb, check_every=25, **kw)
    assert bits(r1) == bits(again) and bits(r1) == bits(r25)
    conv = r1.iters[r1.status == _lib.QP_CONVERGED].tolist()
    assert len(conv) >= 4 and len(set(conv)) > 1               # systems froze at different iterations
    perm = np.random.default_rng(0).permutation(B)
    pin, pM = inputs(sol, [ps[i] for i in perm])
    rp = cross_run(sol, pin, pM, check_every=7, **kw)
    for j, i in enumerate(perm):
        assert system_bits(r1, i, sol) == system_bits(rp, j, sol), (i, j)


# ---- 5. the knot stride --------------------------------------------------------------------------------------------------------
def test_knot_stride_long_horizon():
    """2/1/8197: the knots >= 8192 are a second pass of the knot loop in every workgroup's LDS.  Three iterations against the
    sparse reference, the whole vectors and those knots alone: 1e-6 relative, the bar of the long horizons in
    test_gpu_qp_kernel_sweep.py (the sparse reference's own residual at this size is 6e-15; a knot skipped, or one that read
    the W or M of the first pass, errs at order 1)."""
    S, C, K = XR.STRIDE_CELL
    n = S + C
    key = (S, C, K, 2, False, "full", False, True)
    p = XR.problem(*key)
    want = XR.parity_reference(key, iters=XR.STRIDE_ITERS)
    sol = solver(S, C, K, np.float64)
    inp, Mb = inputs(sol, [p])
    r = cross_run(sol, inp, Mb, eps_abs=0.0, eps_rel=0.0, max_admm_iters=XR.STRIDE_ITERS, exit_tol=1e-20, max_iters=1000)
    got = admm_host(r, 0, sol)
    print("pcg iterations of the x-steps", sol.box_qp_pcg_iters().tolist())
    assert got["status"] == want["status"] == ref.MAX_ITERS and got["iters"] == want["iters"] == XR.STRIDE_ITERS
    assert np.any(want["y"][CAP * n:] != 0) and p["M"][CAP:].any()
    for k in ("x", "z", "y", "lam"):
        t = CAP * (S if k == "lam" else n)
        whole, tail = rel(got[k], want[k]), rel(got[k][t:], want[k][t:])
        print("long-K rel", k, "whole", whole, "knots >= 8192", tail)
        assert whole <= 1e-6 and tail <= 1e-6, (k, whole, tail)


# ---- 6. inputs and outputs -----------------------------------------------------------------------------------------------------
def test_unaligned_arrays_and_unwritten_inputs():
    """Every array the new kernel and the two prepare stages read or write - G, M, C, g, lo, hi in, x, z, y, lambda out - one
    element off the 16-byte grid gives the bits of the aligned call (c goes to the whole solve and the re-solve as it always
    did and stays where it is); the caller's G, M, C, g, c, lo and hi are not written."""
    S, C, K = 14, 7, 9
    p = XR.problem(S, C, K, 9, True, "full")
    sol = solver(S, C, K, np.float64)
    inp, Mb = inputs(sol, [p])
    kw = dict(SYN, max_admm_iters=40)
    want = cross_run(sol, inp, Mb, **kw)

    def off(t):
        u = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:]
        u.copy_(t)
        assert u.data_ptr() % 16 == 8 and u.is_contiguous()
        return u
    uin, uM = tuple(t if i == 3 else off(t) for i, t in enumerate(inp)), off(Mb)
    outs = {k: off(v) for k, v in sentinels(sol).items()}
    got = cross_run(sol, uin, uM, **kw, **outs)
    assert bits(got) == bits(want) and got.x.data_ptr() == outs["x"].data_ptr()
    for u, t in zip(uin + (uM,), inp + (Mb,)):
        assert u.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()
    fresh, fM = inputs(sol, [p])
    for t, f in zip(inp + (Mb,), fresh + (fM,)):
        assert t.cpu().numpy().tobytes() == f.cpu().numpy().tobytes()


# ---- 7. warm start -------------------------------------------------------------------------------------------------------------
def test_warm_start():
    key = (4, 2, 9, 0, False, "controls")
    p = XR.problem(*key)
    sol = solver(4, 2, 9, np.float64)
    inp, Mb = inputs(sol, [p])
    kw = dict(SYN, eps_abs=1e-7, eps_rel=1e-7)
    cold = cross_run(sol, inp, Mb, **kw)
    assert int(cold.status[0]) == _lib.QP_CONVERGED and int(cold.iters[0]) > 10
    warm = cross_run(sol, inp, Mb, z=cold.z.clone(), y=cold.y.clone(), lam=cold.lam.clone(), warm=True, **kw)
    print("cold", int(cold.iters[0]), "warm", int(warm.iters[0]))
    assert int(warm.status[0]) == _lib.QP_CONVERGED and int(warm.iters[0]) < int(cold.iters[0])
    check_converged(sol, warm, 0, p, 1e-7)


# ---- 8. frozen systems ---------------------------------------------------------------------------------------------------------
def test_frozen_systems_are_not_written_again():
    """A batch whose systems freeze at different iterations - the first has a zero right-hand side and freezes after one - while
    the last keeps the loop running: each system's outputs are those of a call on it alone, whose loop ends at its freeze (a
    system written after its freeze would hold a later iterate), and every output entry was written (no sentinel is left)."""
    S, C, K = 4, 2, 9
    ps = [XR.problem(S, C, K, seed, False, "controls") for seed in (34, 0, 17)]
    s0 = ps[0]["s"]
    zero = dict(ps[0], s=synth.KKTSystem(S, C, K, s0.G_row, s0.G_col, s0.G_val, s0.C_row, s0.C_col, s0.C_val, np.zeros_like(s0.g),
                                         np.zeros_like(s0.c), s0.rho))
    ps = [zero] + ps[1:]
    sol = solver(S, C, K, np.float64, batch=3)
    inp, Mb = inputs(sol, ps)
    r = cross_run(sol, inp, Mb, check_every=1, **SYN, **sentinels(sol))
    its = r.iters.tolist()
    print("iters", its, "status", r.status.tolist())
    assert r.status.tolist() == [_lib.QP_CONVERGED] * 3 and its[0] == 1 and its[0] < its[1] < its[2]
    for t in (r.x, r.z, r.y, r.lam):
        assert not (t == SENTINEL).any()
    assert not r.x.view(3, -1)[0].any() and not r.lam.view(3, -1)[0].any()
    for b in (0, 1, 2):
        one = solver(S, C, K, np.float64)
        oin, oM = inputs(one, [ps[b]])
        solo = cross_run(one, oin, oM, check_every=1, **SYN, **sentinels(one))
        assert system_bits(r, b, sol) == system_bits(solo, 0, one), b


# ---- 9. solver state -----------------------------------------------------------------------------------------------------------
def test_solver_state_and_refusals():
    S, C, K = 14, 7, 9
    p = XR.problem(S, C, K, 4, False, "controls")
    sol = solver(S, C, K, np.float64)
    inp, Mb = inputs(sol, [p])
    gen = sol.get_option("assembly_gen")
    r = cross_run(sol, inp, Mb, max_admm_iters=30, **SYN)
    assert int(r.iters[0]) > 1
    assert sol.get_option("assembly_valid") == 1 and sol.get_option("assembly_gen") == gen + 1
    assert sol.box_qp_pcg_iters()[0] > 0
    with pytest.raises(_lib.GatoError, match="not that of a cross solve"):      # no cross assembly is recorded
        sol.solve_rhs_cross(inp[2], inp[3], 1e-10, 300)
    gen = sol.get_option("assembly_gen")
    sol.solve_rhs(inp[2], inp[3], 1e-10, 300)                                # the transformed x-step matrix: a plain re-solve runs
    torch.cuda.synchronize()
    assert sol.get_option("assembly_gen") == gen
    # a NULL M with K > 1: GATO_EINVAL, a text, nothing enqueued
    x = sol.new(sol.N).fill_(7.0)
    others = [sol.new(sol.N) for _ in range(2)] + [sol.new(sol.sizes["sk"]), sol.new(1, torch.int32), sol.new(1, torch.int32),
                                                   sol.new(2, torch.float64)]
    torch.cuda.synchronize()
    L = _lib.lib()
    prm = _lib.BoxQpParams()
    L.gato_box_qp_default_params(prm)
    ptr = lambda t: ct.c_void_p(t.data_ptr())
    rc = L.gato_box_qp_solve_cross(sol._h, ptr(inp[0]), None, *(ptr(t) for t in inp[1:]), ct.byref(prm), ptr(x),
                                   *(ptr(t) for t in others), sol._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"d_M_blocks is required" in L.gato_last_error()
    assert float(x.min()) == 7.0 and float(x.max()) == 7.0 and sol.get_option("assembly_gen") == gen
    with pytest.raises(ValueError, match="Mb must be a contiguous"):
        sol.box_qp_cross(inp[0], Mb[:-1], *inp[1:], rho=RHO, exit_tol=1e-10, max_iters=100)
    with pytest.raises(_lib.GatoError):                                       # the parameter checks of gato_box_qp_solve
        sol.box_qp_cross(inp[0], Mb, *inp[1:], rho=RHO, exit_tol=1e-10, max_iters=100, alpha=2.0, x=x)
    torch.cuda.synchronize()
    assert float(x.min()) == 7.0 and float(x.max()) == 7.0


# ---- 10. the math-shaped entry -------------------------------------------------------------------------------------------------
def test_math_shaped_entry_equals_the_raw_call():
    import gato_python_amd
    S, C, K = 4, 2, 9
    keys = [(S, C, K, 0, False, "controls"), (S, C, K, 17, False, "controls")]
    ps = [XR.problem(*k) for k in keys]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")

    def math_args(p):
        xl, ul = P.split_states_controls(p["lo"], S, C, K)
        xh, uh = P.split_states_controls(p["hi"], S, C, K)
        return [t(b) for b in p["blocks"]] + [t(xl), t(xh), t(ul), t(uh)], t(p["M"])
    kw = dict(rho=RHO, exit_tol=1e-16, max_iters=500, eps_abs=1e-7, eps_rel=1e-7, **SYN)
    sol = solver(S, C, K, np.float64, batch=2)
    inp, Mb = inputs(sol, ps)
    raw = cross_run(sol, inp, Mb, eps_abs=1e-7, eps_rel=1e-7, **SYN)
    assert raw.status.tolist() == [_lib.QP_CONVERGED] * 2
    args, Ms = zip(*(math_args(p) for p in ps))
    res = gato_python_amd.box_qp(*(torch.stack(a) for a in zip(*args)), M=torch.stack(Ms), **kw)
    assert res.x.shape == (2, sol.N) and res.x.grad_fn is None
    assert bits(res) == bits(raw)
    one = gato_python_amd.box_qp(*args[1], M=Ms[1].requires_grad_(True), **kw)
    assert one.x.shape == (sol.N,) and one.lam.shape == (S * K,) and not one.x.requires_grad
    solo = solver(S, C, K, np.float64)
    sin, sM = inputs(solo, [ps[1]])
    raw1 = cross_run(solo, sin, sM, eps_abs=1e-7, eps_rel=1e-7, **SYN)
    assert bits(one) == bits(raw1)
    plain = gato_python_amd.box_qp(*args[1], **kw)                            # without M: another problem
    assert int(plain.status) == _lib.QP_CONVERGED and not torch.equal(plain.x, one.x)
    again = gato_python_amd.box_qp(*args[1], M=Ms[1], warm=one, **kw)
    assert int(again.status) == _lib.QP_CONVERGED and int(again.iters) < int(one.iters)
