"""What the box-QP GPU tests share: the solver and its stacked device inputs, the calls of Solver.box_qp / box_qp_polish /
box_qp_pdas and of the three C entries of the active-set iteration, the outputs as bytes and behind sentinels, and the checks
of a polished and of a converged point against the numpy references (box_qp_polish_ref, box_qp_active_ref).  Bars: fp64 parity
1e-6 in the infinity norm, KKT residuals <= 1e-7.  A plain module: every test file keeps its own fixtures."""
import ctypes as ct

import numpy as np
import torch

import box_qp_active_ref as AS
import box_qp_polish_ref as P
import box_qp_ref as ref
import kkt_grad_ref as kgr
from gato_python_amd import _lib
from oracle import gato_oracle as o

F64 = dict(exit_tol=1e-20, max_iters=1000)
PARITY = dict(eps_abs=0.0, eps_rel=0.0, max_admm_iters=25, exit_tol=1e-22, max_iters=500)
CAP = 8192                                        # knot_grid(): workgroups per system; knots >= CAP run in a second pass
SENTINEL = -7.25


def solver(S, C, K, dt, batch=1):
    from gato_python_amd.solver import Solver
    return Solver(S, C, K, dt, batch=batch)


def dev_inputs(sol, systems, bounds):
    """Stacked device inputs of the systems (G without rho, C raw, g, c, lo, hi) in the solver's dtype."""
    dt = sol.np_dtype
    Gs, Cs = zip(*(o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, s.S, s.C, s.K, 0.0) for s in systems))
    cat = lambda arrs: sol.to_device(np.concatenate([np.asarray(a, np.float64) for a in arrs]).astype(dt))
    return (cat(Gs), cat(Cs), cat([s.g for s in systems]), cat([s.c for s in systems]),
            cat([b[0] for b in bounds]), cat([b[1] for b in bounds]))


def dev_w(sol, ws):
    """Weights or caps, one vector or number per system, stacked in the solver's dtype."""
    return sol.to_device(np.concatenate([np.broadcast_to(np.asarray(w, np.float64), (sol.N,)) for w in ws]).astype(sol.np_dtype))


def g_and_c(s):
    """(G, C) of a system as scipy.sparse CSR matrices, rho not added: the kernel reads G's rows at rho 0 (a_A = 0)."""
    from scipy import sparse
    return (sparse.csr_matrix((s.G_val, s.G_col, s.G_row), shape=(s.N, s.N)),
            sparse.csr_matrix((s.C_val, s.C_col, s.C_row), shape=(s.S * s.K, s.N)))


def math_inputs(p, requires_grad=False):
    """Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi of problem p as box_qp takes them, then x_soft, u_soft where p has "w" and
    x_soft_max, u_soft_max where it has "m": eleven, thirteen or fifteen device tensors."""
    s = p["s"]
    xl, ul = P.split_states_controls(p["lo"], s.S, s.C, s.K)
    xh, uh = P.split_states_controls(p["hi"], s.S, s.C, s.K)
    arrs = list(kgr.blocks_of(s)) + [xl, xh, ul, uh]
    for k in ("w", "m"):
        if k in p:
            arrs += P.split_states_controls(p[k], s.S, s.C, s.K)
    return [torch.from_numpy(np.ascontiguousarray(t)).cuda().requires_grad_(requires_grad) for t in arrs]


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def _pcg_defaults(sol, kw):
    kw.setdefault("exit_tol", F64["exit_tol"] if sol.np_dtype == np.float64 else 1e-8)
    kw.setdefault("max_iters", F64["max_iters"])


def admm_run(sol, inputs, rho, **kw):
    """Solver.box_qp at the ADMM tests' PCG settings (exit_tol 1e-16 in fp64, 500 iterations)."""
    kw.setdefault("exit_tol", 1e-16 if sol.np_dtype == np.float64 else 1e-8)
    kw.setdefault("max_iters", 500)
    r = sol.box_qp(*inputs, rho=rho, **kw)
    torch.cuda.synchronize()
    return r


def admm(sol, inp, rho, **kw):
    """Solver.box_qp at the polish tests' PCG settings (F64)."""
    _pcg_defaults(sol, kw)
    r = sol.box_qp(*inp, rho=rho, **kw)
    torch.cuda.synchronize()
    return r


def polish(sol, inp, act, r, rho, eps=1e-6, **kw):
    _pcg_defaults(sol, kw)
    act_d = act if isinstance(act, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(act, np.int8)).cuda()
    codes = sol.box_qp_polish(*inp, act_d.reshape(-1), r, rho=rho, eps_abs=eps, eps_rel=eps, **kw)
    torch.cuda.synchronize()
    return codes.cpu().numpy()


def pdas(sol, inp, rho, eps=1e-6, act=None, outs=None, soft_weight=None, soft_cap=None, **kw):
    """Solver.box_qp_pdas; soft_weight, soft_cap: device tensors (dev_w) or None.  The fp32 default of the PCG exit tolerance
    is the hard fp32 seed rule's, 1e-8."""
    _pcg_defaults(sol, kw)
    if act is not None:
        act = torch.from_numpy(np.ascontiguousarray(act, np.int8).reshape(-1)).cuda()
    r = sol.box_qp_pdas(*inp, rho=rho, eps_abs=eps, eps_rel=eps, act=act, soft_weight=soft_weight, soft_cap=soft_cap, **(outs or {}), **kw)
    torch.cuda.synchronize()
    return r


def raw_pdas(sol, inp, w, m, entry, rho, act0=None, max_pdas_iters=30):
    """One of the C entries itself - "gato_box_qp_pdas" (w, m not passed), "gato_box_qp_pdas_soft" (m not passed) or
    "gato_box_qp_pdas_huber"; w, m None: NULL pointers -> (return code, the outputs' bytes in point_bits's order)."""
    B, N, sk = sol.batch, sol.N, sol.sizes["sk"]
    L = _lib.lib()
    prm = _lib.BoxQpParams()
    L.gato_box_qp_default_params(prm)
    prm.rho, prm.exit_tol, prm.max_iters = rho, F64["exit_tol"], F64["max_iters"]
    x, z, y, lam = (torch.zeros(n, dtype=sol.dtype, device="cuda") for n in (B * N, B * N, B * N, B * sk))
    act = torch.zeros(B * N, dtype=torch.int8, device="cuda")
    if act0 is not None:
        act.copy_(torch.from_numpy(np.ascontiguousarray(act0, np.int8).reshape(-1)))
    iters, status = torch.zeros(B, dtype=torch.int32, device="cuda"), sol.new(B, torch.int32)
    res = torch.zeros(2 * B, dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else ct.c_void_p(t.data_ptr())
    wm = {"gato_box_qp_pdas": (), "gato_box_qp_pdas_soft": (w,), "gato_box_qp_pdas_huber": (w, m)}[entry]
    rc = getattr(L, entry)(sol._h, *(ptr(t) for t in inp + wm), ptr(act), ct.byref(prm), max_pdas_iters, ptr(x), ptr(z), ptr(y),
                           ptr(lam), ptr(iters), ptr(status), ptr(res), sol._stream())
    torch.cuda.synchronize()
    res = res.view(B, 2)
    return rc, [t.cpu().numpy().tobytes() for t in (x, z, y, lam, iters, status, res[:, 0].contiguous(), res[:, 1].contiguous(), act)]


# ---- the outputs -------------------------------------------------------------------------------------------------------------
def host(t, B, n):
    return t.cpu().numpy().astype(np.float64).reshape(B, n)


def admm_host(r, b, sol):
    """System b of an ADMM result as a dict of fp64 arrays and Python numbers."""
    N, sk = sol.N, sol.sizes["sk"]
    g = lambda t, n: t.cpu().numpy().astype(np.float64).reshape(-1, n)[b]
    return dict(x=g(r.x, N), z=g(r.z, N), y=g(r.y, N), lam=g(r.lam, sk), iters=int(r.iters[b]), status=int(r.status[b]),
                res_prim=float(r.res_prim[b]), res_dual=float(r.res_dual[b]))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1.0))


def bits(r):
    return [t.cpu().numpy().tobytes() for t in (r.x, r.z, r.y, r.lam, r.iters, r.status, r.res_prim, r.res_dual)]


def point_bits(r, b, sol):
    B = sol.batch
    return [t.cpu().numpy().reshape(B, -1)[b].tobytes() for t in (r.x, r.z, r.y, r.lam, r.iters, r.status, r.res_prim, r.res_dual, r.act)]


def sentinels(sol):
    B, N, sk = sol.batch, sol.N, sol.sizes["sk"]
    return dict(x=sol.new(B * N).fill_(SENTINEL), z=sol.new(B * N).fill_(SENTINEL), y=sol.new(B * N).fill_(SENTINEL),
                lam=sol.new(B * sk).fill_(SENTINEL))


def untouched(r, b, sol):
    B = sol.batch
    return all((t.cpu().numpy().reshape(B, -1)[b] == SENTINEL).all() for t in (r.x, r.z, r.y, r.lam))


# ---- the checks --------------------------------------------------------------------------------------------------------------
def check_polished(sol, r, b, name_or_parts, act):
    """Polished system b against the dense reduced solve: x, lam within 1e-6 (inf norm), qp_kkt_residuals <= 1e-7, x on the
    active set equal to the bounds bit for bit."""
    _, H, Cm, g, c, lo, hi = name_or_parts
    xr, yr, lr = P.reduced_solve(H, Cm, g, c, lo, hi, act)
    B = sol.batch
    x, y, lam = host(r.x, B, sol.N)[b], host(r.y, B, sol.N)[b], host(r.lam, B, sol.sizes["sk"])[b]
    ex, el = np.abs(x - xr).max(), np.abs(lam - lr).max()
    kk = ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam)
    print("x err", ex, "lam err", el, "kkt", kk)
    assert ex < 1e-6 and el < 1e-6, (ex, el)
    assert max(kk.values()) <= 1e-7, kk
    A = act != 0
    assert np.array_equal(x[A], P.bound_values(act, lo, hi)[A])
    assert int(r.status[b]) == _lib.QP_CONVERGED


def check_point(sol, r, b, p, run):
    """System b of an active-set result against problem p's reference run: CONVERGED and ACCEPTED after the reference's solves on
    the reference's act, +-2 included; x, lam within 1e-6 of the reference; the residuals of the (penalised) KKT system <= 1e-7;
    x on the hard-active set equal to the bounds and, with caps, y on the saturated set equal to +-m, bit for bit; z = x on the
    soft-active set and clip(x) elsewhere."""
    H, Cm, g, c, lo, hi = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi"))
    w, m = p.get("w"), p.get("m")
    B = sol.batch
    print("iters", int(r.iters[b]), "want", run["iters"], "status", int(r.status[b]))
    assert int(r.status[b]) == _lib.QP_CONVERGED and int(r.polished[b]) == _lib.POLISH_ACCEPTED
    assert int(r.iters[b]) == run["iters"]
    act = r.act.cpu().numpy().reshape(B, -1)[b]
    assert np.array_equal(act, run["act"]), np.flatnonzero(act != run["act"])[:5]
    x, z, y, lam = host(r.x, B, sol.N)[b], host(r.z, B, sol.N)[b], host(r.y, B, sol.N)[b], host(r.lam, B, sol.sizes["sk"])[b]
    ex, el = np.abs(x - run["x"]).max(), np.abs(lam - run["lam"]).max()
    kk = AS.kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam, w, m)
    print("x err", ex, "lam err", el, "kkt", kk)
    assert ex < 1e-6 and el < 1e-6, (ex, el)
    assert max(kk.values()) <= 1e-7, kk
    sa, hard = P.soft_set(act, w), P.hard_set(act, w)
    assert np.array_equal(x[hard], P.bound_values(act, lo, hi)[hard])
    assert np.array_equal(z[sa], x[sa]) and np.array_equal(z[~sa], np.clip(x, lo, hi)[~sa])
    if m is not None:
        sat = P.sat_set(act)
        assert np.array_equal(y[sat], np.sign(act)[sat] * m[sat])


def cold_case(p):
    """A cold fp64 run of problem p (with its weights "w" and caps "m" where it has them), twice: one assembly per reference
    solve and a valid one left, check_point, and the same bits again."""
    s, run = p["s"], p["run"]
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    wm = {k: dev_w(sol, [p[v]]) for k, v in (("soft_weight", "w"), ("soft_cap", "m")) if v in p}
    gen = sol.get_option("assembly_gen")
    r = pdas(sol, inp, s.rho, **wm)
    assert sol.get_option("assembly_gen") == gen + run["iters"] and sol.get_option("assembly_valid") == 1
    check_point(sol, r, 0, p, run)
    again = pdas(sol, inp, s.rho, **wm)
    assert point_bits(again, 0, sol) == point_bits(r, 0, sol)
