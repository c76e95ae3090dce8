"""What the box-QP GPU tests share: the solver and its stacked device inputs, the calls of Solver.box_qp / box_qp_polish /
box_qp_pdas and of the three C entries of the active-set iteration, the outputs as bytes and behind sentinels, and the checks
of a polished and of a converged point against the numpy references (box_qp_polish_ref, box_qp_active_ref), and the bodies that
more than one suite runs on problems of its own (the cold run, the fp32 run, the line search alone and end to end, the layer's
gradients, the ALM cold run): each takes its problems.  Bars: fp64 parity 1e-6 in the infinity norm, KKT residuals <= 1e-7.  A
plain module: every test file keeps its own fixtures."""
import ctypes as ct

import numpy as np
import torch

import box_qp_active_ref as AS
import box_qp_alm_ref as A
import box_qp_linesearch_ref as L
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
    soft-active set and clip(x) elsewhere.  -> dict x, lam (the parity errors) and kkt (the largest residual)."""
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
    return dict(x=float(ex), lam=float(el), kkt=float(max(kk.values())))


def cold_case(p):
    """A cold fp64 run of problem p (with its weights "w" and caps "m" where it has them), twice: one assembly per reference
    solve and a valid one left, check_point, and the same bits again.  -> check_point's figures."""
    s, run = p["s"], p["run"]
    sol = solver(s.S, s.C, s.K, np.float64)
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    wm = {k: dev_w(sol, [p[v]]) for k, v in (("soft_weight", "w"), ("soft_cap", "m")) if v in p}
    gen = sol.get_option("assembly_gen")
    r = pdas(sol, inp, s.rho, **wm)
    assert sol.get_option("assembly_gen") == gen + run["iters"] and sol.get_option("assembly_valid") == 1
    figures = check_point(sol, r, 0, p, run)
    again = pdas(sol, inp, s.rho, **wm)
    assert point_bits(again, 0, sol) == point_bits(r, 0, sol)
    return figures


def fp32_case(p, iters=True):
    """An fp32 run of the walked problem p rounded to fp32, at eps = F32_EPS and the form's PCG exit tolerance (HARD_F32_EXIT_TOL
    without weights, F32_EXIT_TOL with): CONVERGED on the reference's final act (iters: after the reference's solves), the
    hard-active x the rounded bounds and, with caps, y = +-m on the saturated set, bit for bit."""
    q = P.rounded(p)
    s = q["s"]
    sol = solver(s.S, s.C, s.K, np.float32)
    wm = {k: dev_w(sol, [q[v]]) for k, v in (("soft_weight", "w"), ("soft_cap", "m")) if v in q}
    r = pdas(sol, dev_inputs(sol, [s], [(q["lo"], q["hi"])]), s.rho, eps=P.F32_EPS, exit_tol=AS.F32_EXIT_TOL if "w" in q else AS.HARD_F32_EXIT_TOL,
             max_iters=1000, **wm)
    print("seed", p["seed"], "solves", int(r.iters[0]), "reference", p["run"]["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED and (not iters or int(r.iters[0]) == p["run"]["iters"])
    act = p["run"]["act"]
    assert np.array_equal(r.act.cpu().numpy(), act)
    hard = P.hard_set(act, p.get("w"))
    assert np.array_equal(r.x.cpu().numpy()[hard], P.bound_values(act, q["lo"], q["hi"])[hard].astype(np.float32))
    if "m" in q:
        sat = P.sat_set(act)
        assert np.array_equal(r.y.cpu().numpy()[sat], (np.sign(act)[sat] * q["m"][sat]).astype(np.float32))


# ---- the line search -----------------------------------------------------------------------------------------------------------
def caps_of(p):
    return p["m"] if "m" in p else np.full(p["s"].N, np.inf)


def weights_and_caps(sol, ps):
    """soft_weight and soft_cap of Solver.box_qp_pdas for the problems ps (a cap of +inf where a problem has none)."""
    return dict(soft_weight=dev_w(sol, [p["w"] for p in ps]), soft_cap=dev_w(sol, [caps_of(p) for p in ps]))


def ls_run(sol, ps, **kw):
    inp = dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps])
    return pdas(sol, inp, ps[0]["s"].rho, line_search=True, **weights_and_caps(sol, ps), **kw)


def ls_bits(r, b, sol):
    return point_bits(r, b, sol) + [r.alpha[b].cpu().numpy().tobytes()]


def check_search(sol, cases, dt, with_caps=True):
    """Solver.box_qp_line_search on the systems `cases` (box_qp_linesearch_ref.kernel_inputs' tuples), the stepped point behind
    a sentinel at an unaligned address.  -> the largest |phi'(alpha)| / (N eps scale) over the damped systems."""
    B, N = len(cases), cases[0][0]["s"].N
    eps = float(np.finfo(dt).eps)
    ps = [c[0] for c in cases]
    inp = dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps])
    dev = lambda vs: sol.to_device(np.concatenate(vs).astype(dt))
    wd = dev_w(sol, [p["w"] for p in ps])
    md = dev_w(sol, [caps_of(p) for p in ps]) if with_caps else None
    buf = sol.new(B * N + 1).fill_(SENTINEL)
    rho = float(np.float32(ps[0]["s"].rho)) if dt == np.float32 else ps[0]["s"].rho
    alpha, slope, x = sol.box_qp_line_search(inp[0], inp[2], inp[4], inp[5], wd, md, dev([c[1] for c in cases]),
                                             dev([c[2] for c in cases]), rho=rho, x=buf[1:])
    torch.cuda.synchronize()
    alpha, slope, x = alpha.cpu().numpy(), slope.cpu().numpy(), x.cpu().numpy().reshape(B, N)
    assert float(buf[0]) == SENTINEL
    worst = 0.0
    for b, (p, xc, xp, e) in enumerate(cases):
        q = P.rounded(p) if dt == np.float32 else p
        H, g, lo, hi, m, w = q["H"], q["g"], q["lo"], q["hi"], q.get("m"), L.off_x0(q["w"], p["s"].S)
        d = xp - xc
        for j, a in enumerate((0.0, 1.0)):
            bar = L.SLACK * N * eps * L.slope_scale(H, g, lo, hi, w, m, xc, d, a)
            assert abs(slope[b, j] - (e["s0"], e["s1"])[j]) <= bar, (b, j, slope[b, j], e)
        if e["alpha"] == 1.0:
            assert alpha[b] == 1.0 and x[b].tobytes() == xp.astype(dt).tobytes(), (b, alpha[b])
            continue
        got = L.slope(H, g, lo, hi, w, m, xc, d, alpha[b])
        unit = N * eps * L.slope_scale(H, g, lo, hi, w, m, xc, d, alpha[b])
        print("system", b, "seed", p["seed"], "alpha", alpha[b], "reference", e["alpha"], "piece", e["piece"], "slope / (N eps scale)", abs(got) / unit)
        assert e["piece"][0] <= alpha[b] <= e["piece"][1], (alpha[b], e["piece"])
        assert abs(got) <= L.SLACK * unit, (got, unit)
        assert np.abs(x[b] - (xc + alpha[b] * d)).max() <= 4 * eps * max(1.0, np.abs(xc).max(), np.abs(xp).max())
        worst = max(worst, abs(got) / unit)
    return worst


def check_alphas(alpha, run):
    want = np.array(run["alpha"])
    got = alpha[:len(want)]
    print("alpha", got.tolist(), "reference", want.tolist())
    for a, t in zip(got, want):
        assert (a == t) if t in (0.0, 1.0) else (0.0 < a < 1.0), (got, want)
    assert not alpha[len(want):].any()


def ls_converges_case(p):
    """The line search end to end on the walked problem p, fp64: the reference's number of solves over the reference's act
    sequence (the act of solve j is that of a run stopped after j solves), alpha exactly 1 where the reference's is and inside
    (0, 1) elsewhere, check_point, the same bits again; without the option MAX_ITERS and nothing written.  -> check_point's
    figures."""
    s, run = p["s"], p["run"]
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run))
    sol = solver(s.S, s.C, s.K, np.float64)
    r = ls_run(sol, [p])
    figures = check_point(sol, r, 0, p, run)
    check_alphas(r.alpha[0].cpu().numpy(), run)
    assert ls_bits(ls_run(sol, [p]), 0, sol) == ls_bits(r, 0, sol)
    for j in range(1, run["iters"]):
        part = ls_run(sol, [p], max_pdas_iters=j)
        assert int(part.status[0]) == _lib.QP_MAX_ITERS and np.array_equal(part.act.cpu().numpy(), run["trace"][j - 1]["act"]), j
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    und = pdas(sol, inp, s.rho, outs=sentinels(sol), **weights_and_caps(sol, [p]))
    assert int(und.status[0]) == _lib.QP_MAX_ITERS and untouched(und, 0, sol) and und.alpha is None
    return figures


def ls_fp32_case(p):
    """The line search in fp32 on the walked problem p rounded to fp32, at eps = F32_EPS and the PCG exit tolerance F32_EXIT_TOL:
    the reference's solves, final act and full steps."""
    q = P.rounded(p)
    s = q["s"]
    sol = solver(s.S, s.C, s.K, np.float32)
    r = ls_run(sol, [q], eps=P.F32_EPS, exit_tol=AS.F32_EXIT_TOL, max_iters=1000)
    print("seed", p["seed"], "solves", int(r.iters[0]), "reference", p["run"]["iters"])
    assert int(r.status[0]) == _lib.QP_CONVERGED and int(r.iters[0]) == p["run"]["iters"]
    assert np.array_equal(r.act.cpu().numpy(), p["run"]["act"])
    check_alphas(r.alpha[0].cpu().numpy(), p["run"])


def ls_layer_gradients_case(p, stale, other):
    """box_qp_layer(method="pdas", line_search=True) on the walked line-search problem p: all fifteen gradients against the
    reference through the final act, err < 1e-6 max(1, |want|).  stale: a kkt_solve of the problem `other` (same shape) on the
    cached solver between the passes; the backward pass rebuilds its assembly with one solve on the saved act.  -> the largest
    err / max(1, |want|)."""
    import gato_python_amd
    from box_qp_huber_ref import HUBER_KEYS
    s, run = p["s"], p["run"]
    S, C, K = s.S, s.C, s.K
    ts = math_inputs(p, requires_grad=True)
    x, lam, info = gato_python_amd.box_qp_layer(*ts[:11], rho=s.rho, method="pdas", x_soft=ts[11], u_soft=ts[12], x_soft_max=ts[13],
                                                u_soft_max=ts[14], line_search=True, **F64)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and int(info.iters) == run["iters"]
    assert np.array_equal(info.act.cpu().numpy(), run["act"])
    if stale:
        from gato_python_amd import autograd
        sol = autograd._SOLVERS[(S, C, K, 1, torch.float64, torch.cuda.current_device())]     # the layer's cached solver
        gato_python_amd.kkt_solve(*math_inputs(other)[:7], rho=other["s"].rho, **F64)    # replaces the layer's assembly
        gen = sol.get_option("assembly_gen")
    rng = np.random.default_rng(7)
    xbar, lbar = rng.standard_normal(s.N), rng.standard_normal(S * K)
    ((x * torch.from_numpy(xbar).cuda()).sum() + (lam * torch.from_numpy(lbar).cuda()).sum()).backward()
    if stale:
        assert sol.get_option("assembly_gen") == gen + 1 and sol.get_option("assembly_valid") == 1
    want = P.grads(p["H"], p["Cm"], run["act"], x.detach().cpu().numpy(), lam.detach().cpu().numpy(), xbar, lbar, S, C, K,
                   w=p["w"], m=p["m"], lo=p["lo"], hi=p["hi"])
    worst = 0.0
    for k, t in zip(HUBER_KEYS, ts):
        err = np.abs(t.grad.cpu().numpy() - want[k]).max()
        print(k, err, np.abs(want[k]).max())
        assert err < 1e-6 * max(1.0, np.abs(want[k]).max()), (k, err)
        worst = max(worst, err / max(1.0, np.abs(want[k]).max()))
    return worst


# ---- the augmented-Lagrangian outer loop ---------------------------------------------------------------------------------------
def alm_run(sol, ps, eps=1e-6, act=None, mu=None, outs=None, **kw):
    """Solver.box_qp_alm on the problems ps (their weights "w" and caps "m" where the first one has them)."""
    inp = dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps])
    kw.setdefault("exit_tol", F64["exit_tol"] if sol.np_dtype == np.float64 else AS.F32_EXIT_TOL)
    kw.setdefault("max_iters", 1000)
    wm = {k: dev_w(sol, [p[v] for p in ps]) for k, v in (("soft_weight", "w"), ("soft_cap", "m")) if v in ps[0]}
    if act is not None:
        act = torch.from_numpy(np.ascontiguousarray(act, np.int8).reshape(-1)).cuda()
    if mu is not None:
        mu = sol.to_device(np.asarray(mu, np.float64).reshape(-1))
    r = sol.box_qp_alm(*inp, rho=ps[0]["s"].rho, eps_abs=eps, eps_rel=eps, act=act, mu=mu, **wm, **(outs or {}), **kw)
    torch.cuda.synchronize()
    return r


def alm_bits(r, b, sol):
    B = sol.batch
    return [t.cpu().numpy().reshape(B, -1)[b].tobytes() for t in (r.x, r.z, r.y, r.lam, r.iters, r.status, r.res_prim, r.res_dual, r.act,
                                                                   r.outer, r.weight)]


def alm_point(r, b, sol):
    B = sol.batch
    return host(r.x, B, sol.N)[b], host(r.z, B, sol.N)[b], host(r.y, B, sol.N)[b], host(r.lam, B, sol.sizes["sk"])[b]


def check_alm_run(sol, p, r, b=0):
    """System b against problem p's reference run and x*: CONVERGED with the reference's outer steps, solves and last weight; the
    hard QP's stationarity and equality <= 1e-7 (fp64) and its bound violation within the acceptance bar; |x - x*|_inf within ten
    times the reference's own distance at the same eps."""
    run, xs, eps = p["run"], p["exact"], p["eps"]
    x, z, y, lam = alm_point(r, b, sol)
    print("seed", p["seed"], p["form"], "outer", int(r.outer[b]), run["outer"], "iters", int(r.iters[b]), run["iters"], "weight", float(r.weight[b]), run["weight"])
    assert int(r.status[b]) == _lib.QP_CONVERGED
    assert (int(r.outer[b]), int(r.iters[b]), float(r.weight[b])) == (run["outer"], run["iters"], run["weight"])
    assert np.array_equal(r.act.cpu().numpy().reshape(sol.batch, -1)[b], run["act"])
    lo, hi = A.hard_box(p)
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], lo, hi, x, y, lam)
    bar = eps + eps * float(np.abs(x).max())
    dist, own = float(np.abs(x - xs["x"]).max()), float(np.abs(run["x"] - xs["x"]).max())
    print("kkt", kk, "bar", bar, "|x - x*|", dist, "reference's own", own)
    if sol.np_dtype == np.float64:
        assert kk["stat"] <= 1e-7 and kk["eq"] <= 1e-7, kk
    assert kk["bound"] <= bar and float(r.res_prim[b]) <= bar
    assert dist <= 10 * own, (dist, own)
    av = A.alm_set(p["lo"], p["hi"], p["s"].S, p.get("w"))
    assert np.array_equal(z[av], np.clip(x, p["lo"], p["hi"])[av])
    return dist, own


def check_alm_steps(sol, p, **kw):
    """The reference's weight sequence and per-step solves: a run stopped after j outer steps is MAX_ITERS with the solves of the
    first j steps, step j's weight and step j's violation."""
    run = p["run"]
    for j in range(1, run["outer"]):
        part = alm_run(sol, [p], eps=p["eps"], max_alm_iters=j, outs=sentinels(sol), **kw)
        st = run["steps"][j - 1]
        assert int(part.status[0]) == _lib.QP_MAX_ITERS and untouched(part, 0, sol), j
        assert (int(part.iters[0]), float(part.weight[0])) == (sum(t["solves"] for t in run["steps"][:j]), st["w"]), j
        assert abs(float(part.res_prim[0]) - st["v"]) <= 1e-3 * st["v"] + (0 if sol.np_dtype == np.float64 else p["eps"]), (j, float(part.res_prim[0]), st["v"])


def alm_cold_case(p):
    """A cold fp64 ALM run of the pinned problem p: check_alm_run, check_alm_steps and the same bits on a repeat.  -> check_alm_run's
    (distance to x*, the reference's own)."""
    s = p["s"]
    sol = solver(s.S, s.C, s.K, np.float64)
    r = alm_run(sol, [p])
    out = check_alm_run(sol, p, r)
    check_alm_steps(sol, p)
    assert alm_bits(alm_run(sol, [p]), 0, sol) == alm_bits(r, 0, sol)
    return out
