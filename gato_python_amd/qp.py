"""Box-constrained QP solves from math-shaped blocks.

    box_qp(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, *, rho, exit_tol, max_iters, ...) -> BoxQPResult

solves  min 1/2 x^T (G + rho I) x - g^T x  s.t.  C x = c,  lo <= x <= hi  - the KKT system of autograd.kkt_solve plus bounds on
the states and controls - by ADMM over the device re-solve (Solver.box_qp, gato_box_qp_solve), optionally polished on the ADMM
result's active set (polish=True), or by the primal-dual active-set iteration alone (method="pdas",
Solver.box_qp_pdas; x_soft / u_soft turn bounds into quadratic penalties, section 3.10, and x_soft_max /
u_soft_max cap their forces, section 3.11).  It is NOT differentiable: the inputs are read detached and the outputs carry no
grad_fn.

    box_qp_layer(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, *, rho, exit_tol, max_iters, **admm) -> (x, lam, info)

is the differentiable form: ADMM, the active set, the polish (or method="pdas": the active-set iteration alone); the backward
pass is one re-solve of the polish assembly (the reduced KKT system) plus the gradient launches; forward mode (dual tensors of
torch.autograd.forward_ad, or box_qp_layer_tangents for R directions in one call) is the same re-solve
behind one launch for the tangent right-hand sides.  Only device tensors are taken; there is no CPU fallback.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .autograd import _adjoint, _check_blocks, _check_cross, _common, _dots, _dz_layout, _fresh, _pack, _pack_tangents, _solver, _tangent_dims
from .solver import BoxQPResult, hard_active, zero_rhs


def _bound(v, shape, name, ref, what):
    """A bound of the entry `what` as a tensor of `shape` (a Python number or a tensor that broadcasts to it), in ref's dtype
    and device.  A tensor keeps its autograd history (expand sums the gradient of a broadcast bound); box_qp calls this under
    torch.no_grad()."""
    if not isinstance(v, torch.Tensor):
        return torch.full(shape, float(v), dtype=ref.dtype, device=ref.device)
    if v.device != ref.device or v.dtype != ref.dtype:
        raise ValueError(f"{what}: {name} must be a {ref.dtype} tensor on {ref.device}, got {v.dtype} on {v.device}")
    try:
        return v.expand(shape)
    except RuntimeError:
        raise ValueError(f"{what}: {name} of shape {tuple(v.shape)} does not broadcast to {shape}") from None


def _prepare(what, blocks, x_lo, x_hi, u_lo, u_hi, x_soft, u_soft, x_soft_max=None, u_soft_max=None):
    """Everything of box_qp and box_qp_layer (`what`) up to the solver call: the checks of the blocks (Q, R, A, B, q, r, c) and
    the bounds, then (Gb, Cb, g, c) packed, lo, hi, the soft weights w (None unless x_soft or u_soft is given) and the caps m
    (None unless x_soft_max or u_soft_max is given; +inf where only the other is) in the dz layout [Bt, N], and Bt, batched
    and the cached solver.  In torch ops, which torch differentiates."""
    args = dict(zip("Q R A B q r c".split(), blocks))
    batched, lead, K, S, C = _check_blocks(args, what, qp=True)
    device, dtype = _common(args, what)
    q, xs, us = args["q"], lead + (K, S), lead + (K - 1, C)
    lift = (lambda t: t) if batched else (lambda t: t.unsqueeze(0))
    xl, xh = (lift(_bound(v, xs, n, q, what)) for v, n in ((x_lo, "x_lo"), (x_hi, "x_hi")))
    ul, uh = (lift(_bound(v, us, n, q, what)) for v, n in ((u_lo, "u_lo"), (u_hi, "u_hi")))
    Gb, Cb, g, cc = _pack(*(lift(t) for t in blocks))
    lo, hi = _dz_layout(xl, ul), _dz_layout(xh, uh)
    Bt = g.shape[0]
    sol = _solver(S, C, K, Bt, dtype, device)
    w = None
    if x_soft is not None or u_soft is not None:
        xw = lift(_bound(0.0 if x_soft is None else x_soft, xs, "x_soft", q, what))
        uw = lift(_bound(0.0 if u_soft is None else u_soft, us, "u_soft", q, what))
        w = _dz_layout(xw, uw)
    m = None
    if x_soft_max is not None or u_soft_max is not None:
        xm = lift(_bound(float("inf") if x_soft_max is None else x_soft_max, xs, "x_soft_max", q, what))
        um = lift(_bound(float("inf") if u_soft_max is None else u_soft_max, us, "u_soft_max", q, what))
        m = _dz_layout(xm, um)
    return Gb, Cb, g, cc, lo, hi, w, m, Bt, batched, sol


def _check_caps(what, method, polish, soft, capped):
    """The refusals of x_soft_max / u_soft_max: they need the active-set iteration and a weight to cap."""
    if not capped:
        return
    if method != "pdas" or polish:
        raise ValueError(f"{what}: x_soft_max and u_soft_max need method='pdas' without polish (ADMM and the polish have no soft bounds)")
    if not soft:
        raise ValueError(f"{what}: x_soft_max and u_soft_max cap the force of a soft bound: give x_soft or u_soft too")


def _check_line_search(what, method, polish, soft, line_search):
    """The refusals of line_search=True that need no look at the bounds: it is an option of the active-set iteration on soft
    bounds (a finite bound without a weight is refused by the solver, which reads the bounds on the device)."""
    if not line_search:
        return
    if method != "pdas" or polish:
        raise ValueError(f"{what}: line_search=True needs method='pdas' without polish (it is a step of the active-set iteration)")
    if not soft:
        raise ValueError(f"{what}: line_search=True takes soft bounds only: give x_soft or u_soft, a positive weight on every "
                         "variable with a finite bound")


def _check_layer(what, method, soft, capped, line_search):
    """The refusals box_qp_layer and box_qp_layer_tangents (`what`) share: the method, then what the soft bounds, their caps and
    the line search need."""
    if method not in ("admm", "pdas"):
        raise ValueError(f"{what}: method must be 'admm' or 'pdas', got {method!r}")
    _check_caps(what, method, False, soft, capped)
    _check_line_search(what, method, False, soft, line_search)
    if soft and method != "pdas":
        raise ValueError(f"{what}: x_soft and u_soft need method='pdas' (ADMM and the polish have no soft bounds)")


def _layer_opts(method, max_pdas_iters, line_search, rho, exit_tol, max_iters, admm_rho, sigma, alpha, eps_abs, eps_rel,
                max_admm_iters, check_every):
    """The options _layer_solve reads: those of Solver.box_qp, and for method="pdas" max_pdas_iters and the line search."""
    opts = dict(rho=float(rho), exit_tol=float(exit_tol), max_iters=int(max_iters), admm_rho=admm_rho, sigma=sigma, alpha=alpha,
                eps_abs=eps_abs, eps_rel=eps_rel, max_admm_iters=max_admm_iters, check_every=check_every)
    if method == "pdas":
        opts["max_pdas_iters"] = int(max_pdas_iters)
        if line_search:
            opts["line_search"] = True
    return opts


def _check_cross_qp(blocks, M, method, polish):
    """The refusals of box_qp(M=): the method and the polish, then M's shape, dtype and device by kkt_solve's rules - all before
    any solver is created."""
    if method != "admm" or polish:
        raise ValueError("box_qp: M needs method='admm' without polish: the polish and the active-set iteration (method='pdas', "
                         "method='alm') invert G block by block and read it in every step, with no cross term (DESIGN.md section "
                         "3.16)")
    args = dict(zip("Q R A B q r c".split(), blocks))
    _, lead, K, S, C = _check_blocks(args, "box_qp", qp=True)
    _check_cross(M, lead, K, S, C, args["Q"], "box_qp")


def _warm_act(warm, Bt, sol, device, starts):
    """warm.act of box_qp, flat, for an active-set start; `starts` ends the refusal of one that does not match the problem."""
    act = getattr(warm, "act", None)
    if not isinstance(act, torch.Tensor) or act.numel() != Bt * sol.N or act.dtype != torch.int8 or act.device != device:
        raise ValueError(f"box_qp: warm.act does not match this problem ({Bt} x {sol.N} int8 on {device}); {starts}")
    return act.reshape(-1).contiguous()


def box_qp(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, *, rho, exit_tol, max_iters, admm_rho=0.1, sigma=1e-6, alpha=1.6,
           eps_abs=1e-6, eps_rel=1e-6, max_admm_iters=4000, check_every=25, warm=None, polish=False, method="admm",
           polish_iters=1, max_pdas_iters=30, x_soft=None, u_soft=None, x_soft_max=None, u_soft_max=None, line_search=None,
           alm_weight=100.0, alm_growth=10.0, alm_weight_max=None, max_alm_iters=50, M=None):
    """Box-constrained QP from math-shaped blocks, at most one leading batch dimension:
    Q [*,K,S,S], R [*,K-1,C,C], A [*,K-1,S,S], B [*,K-1,S,C], q [*,K,S], r [*,K-1,C], c [*,K,S] as kkt_solve takes them (A, B
    the raw values stored in C: -A and -B of the dynamics), and the bounds x_lo, x_hi [*,K,S], u_lo, u_hi [*,K-1,C] - numbers
    or tensors that broadcast to those shapes, +-inf allowed.  warm: a previous BoxQPResult of the same shape (its z, y and
    lam start the iteration).  Returns a BoxQPResult with flat x, z, y [*, N], lam [*, S K] (dz layout, as kkt_solve returns
    dz and lam) and iters, status, res_prim, res_dual [*] (scalars unbatched).  Raises ValueError for lo > hi or a NaN bound.
    polish=True: the ADMM result is then polished on its active set (Solver.box_qp_polish): where the polished point passes
    the termination test it replaces the result (status CONVERGED); result.polished [*] holds the codes (_lib.POLISH_*).
    polish_iters > 1 (with polish=True): the polish stage is the active-set iteration (Solver.box_qp_pdas) started from the
    ADMM result's active set, at most polish_iters reduced solves; result.act [*, N] is its final active set.
    method="pdas": no ADMM - the active-set iteration from a cold start (nothing active), or from warm.act when warm is a
    previous result of method="pdas" (an MPC shift), at most max_pdas_iters reduced solves; iters counts them, and a system
    that does not end CONVERGED returns zeros.  The ADMM parameters and polish are not read.
    x_soft [*,K,S], u_soft [*,K-1,C] (method="pdas" only; numbers or tensors that broadcast like the bounds; None: 0): soft
    bounds.  A weight w > 0 replaces the bound of its variable by the penalty (w / 2) dist(x, [lo,
    hi])^2, a weight 0 keeps the hard bound.  For a soft variable outside its bounds result.y is the penalty force w (x - b)
    and result.z = x.  ValueError for method="admm" or polish=True, and for a NaN, negative or infinite weight.
    x_soft_max [*,K,S], u_soft_max [*,K-1,C] (with x_soft / u_soft; numbers or tensors that broadcast like the weights; None: no
    cap): caps m >= 0 on the penalty forces.  The penalty becomes the Huber function - quadratic while
    w dist <= m, linear with slope m beyond - and the force clamp(w (x - clip(x)), -m, m).  A saturated variable has
    result.act = +-2 and result.y = +-m; warm.act may carry +-2.  ValueError for method="admm" or polish=True, without any
    weight, and for a NaN or negative cap.
    line_search=True (method="pdas" with x_soft / u_soft): the exact line search on the penalised
    objective, which makes the iteration converge where the undamped one cycles (large weights, caps between the regimes), at
    the price of more solves elsewhere.  Every variable with a finite bound (off x_0) must have a positive weight.
    result.alpha [*, max_pdas_iters] holds the step length of every solve (1: a full step, 0: none taken).  ValueError for
    method="admm", polish=True, without weights, and for a finite bound whose weight is 0.
    method="alm" (DESIGN.md section 3.14): hard bounds on states and controls by the method of multipliers over the line-search
    iteration - the method for hard state bounds, where ADMM needs thousands of x-steps and the hard active-set iteration
    cycles or meets a singular system.  Every variable with a finite bound and no weight gets a multiplier and the penalty weight
    w, from alm_weight; an outer step is one line-search iteration (at most max_pdas_iters solves) on the bounds shifted by
    -mu / w, then mu <- its force, and w <- alm_growth w where the violation did not fall below a quarter of the step before
    (while w < alm_weight_max; None: 1e8 in float64, 1e5 in float32), at most max_alm_iters steps.  CONVERGED: the violation
    of the hard bounds is within eps_abs + eps_rel |x|_inf, result.z is x clipped to them and result.y holds their multipliers.
    An infeasible box ends MAX_ITERS with result.res_prim the violation it stalls at.  x_soft / u_soft (and x_soft_max /
    u_soft_max) keep their variables soft bounds: hard actuator limits with soft state limits.  result.iters counts the reduced
    solves of all steps, result.outer the steps, result.weight the last w.  warm: a previous method="alm" result - its y starts
    the multipliers and its act the active set.  polish=True: the point is then polished on its active set
    (Solver.box_qp_polish) and replaced by the exact vertex where the polish is ACCEPTED (LICQ holds); no weights then.
    ValueError for an ADMM parameter or polish_iters that is not its default, for line_search (it is implied) and for
    alm_weight <= 0, alm_growth <= 1, alm_weight_max < alm_weight or max_alm_iters < 1.
    M [*,K-1,S,C] (None: no cross term, the call as it always was): the stage cost gains x_k^T M_k u_k,
    G_k = [[Q_k, M_k], [M_k^T, R_k]], as kkt_solve(M=) takes it; every G_k + rho I must be positive definite (not checked).  ADMM
    only (Solver.box_qp_cross): method="admm" without polish, warm as without M; the bounds and the result are in the original
    variables.  ValueError for polish=True, method="pdas" or method="alm" (the active-set kernels read G block by block), and
    for an M of another shape, dtype or device, before any solver is created."""
    if method not in ("admm", "pdas", "alm"):
        raise ValueError(f"box_qp: method must be 'admm', 'pdas' or 'alm', got {method!r}")
    if M is not None:
        _check_cross_qp((Q, R, A, B, q, r, c), M, method, polish)
    if method == "alm":
        return _box_qp_alm((Q, R, A, B, q, r, c), (x_lo, x_hi, u_lo, u_hi), (x_soft, u_soft, x_soft_max, u_soft_max),
                           dict(admm_rho=(admm_rho, 0.1), sigma=(sigma, 1e-6), alpha=(alpha, 1.6), max_admm_iters=(max_admm_iters, 4000),
                                check_every=(check_every, 25), polish_iters=(polish_iters, 1)), line_search, warm, polish,
                           dict(rho=rho, exit_tol=exit_tol, max_iters=max_iters, eps_abs=eps_abs, eps_rel=eps_rel),
                           dict(max_pdas_iters=max_pdas_iters, alm_weight=alm_weight, alm_growth=alm_growth,
                                alm_weight_max=alm_weight_max, max_alm_iters=max_alm_iters))
    if (alm_weight, alm_growth, alm_weight_max, max_alm_iters) != (100.0, 10.0, None, 50):
        raise ValueError("box_qp: alm_weight, alm_growth, alm_weight_max and max_alm_iters need method='alm'")
    soft = x_soft is not None or u_soft is not None
    _check_caps("box_qp", method, polish, soft, x_soft_max is not None or u_soft_max is not None)
    _check_line_search("box_qp", method, polish, soft, line_search)
    if soft and (method != "pdas" or polish):
        raise ValueError("box_qp: x_soft and u_soft need method='pdas' without polish (ADMM and the polish have no soft bounds)")
    if int(polish_iters) < 1 or int(max_pdas_iters) < 1:
        raise ValueError("box_qp: polish_iters and max_pdas_iters must be at least 1")
    with torch.no_grad():
        Gb, Cb, g, cc, lo, hi, wt, mt, Bt, batched, sol = _prepare("box_qp", (Q, R, A, B, q, r, c), x_lo, x_hi, u_lo, u_hi,
                                                                   x_soft, u_soft, x_soft_max, u_soft_max)
        if method == "pdas":
            act = None if warm is None else _warm_act(warm, Bt, sol, g.device,
                                                      "method='pdas' starts from the act of a previous method='pdas' result")
            res = sol.box_qp_pdas(Gb, Cb, g, cc, lo, hi, rho=rho, exit_tol=exit_tol, max_iters=max_iters, eps_abs=eps_abs,
                                  eps_rel=eps_rel, max_pdas_iters=max_pdas_iters, act=act, soft_weight=wt,
                                  soft_cap=None if mt is None else mt.contiguous(), line_search=bool(line_search))
            return _shaped(res, sol, Bt, batched)
        out = {}
        if warm is not None:
            for name in ("z", "y", "lam"):
                t = getattr(warm, name)
                n = sol.sizes["sk"] if name == "lam" else sol.N
                if not isinstance(t, torch.Tensor) or t.numel() != Bt * n or t.dtype != g.dtype or t.device != g.device:
                    raise ValueError(f"box_qp: warm.{name} does not match this problem ({Bt} x {n} {g.dtype} on {g.device})")
                out[name] = t.detach().reshape(Bt, n).clone()
        admm = dict(rho=rho, exit_tol=exit_tol, max_iters=max_iters, admm_rho=admm_rho, sigma=sigma, alpha=alpha, eps_abs=eps_abs,
                    eps_rel=eps_rel, max_admm_iters=max_admm_iters, check_every=check_every, warm=warm is not None, **out)
        if M is None:
            res = sol.box_qp(Gb, Cb, g, cc, lo, hi, **admm)
        else:                                                       # M_k S x C column-major per knot, as B_k lies in Cb
            Mb = M.detach().transpose(-1, -2).reshape(Bt, -1).contiguous()
            res = sol.box_qp_cross(Gb, Mb, Cb, g, cc, lo, hi, **admm)
        if polish:
            act = sol.box_qp_active_set(res.z, res.y, lo, hi)
            if int(polish_iters) == 1:
                sol.box_qp_polish(Gb, Cb, g, cc, lo, hi, act, res, rho=rho, exit_tol=exit_tol, max_iters=max_iters,
                                  eps_abs=eps_abs, eps_rel=eps_rel)
            else:
                _polish_iterated(sol, (Gb, Cb, g, cc, lo, hi), act, res, int(polish_iters), rho=rho, exit_tol=exit_tol,
                                 max_iters=max_iters, eps_abs=eps_abs, eps_rel=eps_rel)
    return _shaped(res, sol, Bt, batched)


def _polish_iterated(sol, inp, act, res, polish_iters, **pol):
    """The polish stage as the active-set iteration from act: where it converges, its point replaces the ADMM result in place
    (x, z, y, lam are written by the device only there), status becomes CONVERGED and the residuals the point's; elsewhere
    the ADMM result stays.  iters stays the count of ADMM x-steps."""
    pd = sol.box_qp_pdas(*inp, act=act, max_pdas_iters=polish_iters, x=res.x, z=res.z, y=res.y, lam=res.lam, **pol)
    ok = pd.status == _lib.QP_CONVERGED
    res.status.copy_(torch.where(ok, pd.status, res.status))
    res.res_prim.copy_(torch.where(ok, pd.res_prim, res.res_prim))
    res.res_dual.copy_(torch.where(ok, pd.res_dual, res.res_dual))
    res.polished, res.act = pd.polished, pd.act


def _shaped(res, sol, Bt, batched):
    N, sk = sol.N, sol.sizes["sk"]
    shp = lambda t, n: t.view(Bt, n) if batched else t.view(n)
    first = (lambda t: t) if batched else (lambda t: t[0])
    return BoxQPResult(shp(res.x, N), shp(res.z, N), shp(res.y, N), shp(res.lam, sk), first(res.iters), first(res.status),
                       first(res.res_prim), first(res.res_dual), None if res.polished is None else first(res.polished),
                       None if res.act is None else shp(res.act, N),
                       None if res.alpha is None else (res.alpha if batched else res.alpha[0]),
                       None if res.outer is None else first(res.outer), None if res.weight is None else first(res.weight))


def _box_qp_alm(blocks, bounds, soft, admm_only, line_search, warm, polish, pol, alm):
    """box_qp(method="alm"): the refusals, Solver.box_qp_alm and - polish - the active set of its point and one polish on it."""
    given = [name for name, (v, default) in admm_only.items() if v != default]
    if given:
        raise ValueError(f"box_qp: {', '.join(given)} {'is' if len(given) == 1 else 'are'} not read by method='alm' (ADMM and "
                         "its polish stage only)")
    if line_search is not None:
        raise ValueError("box_qp: line_search is implied by method='alm' (every inner iteration is the line-search one): leave it out")
    weight, growth, weight_max = float(alm["alm_weight"]), float(alm["alm_growth"]), alm["alm_weight_max"]
    if not (0 < weight < float("inf")) or not growth > 1 or (weight_max is not None and not float(weight_max) >= weight):
        raise ValueError("box_qp: method='alm' needs a finite alm_weight > 0, alm_growth > 1 and alm_weight_max >= alm_weight")
    if int(alm["max_alm_iters"]) < 1 or int(alm["max_pdas_iters"]) < 1:
        raise ValueError("box_qp: max_alm_iters and max_pdas_iters must be at least 1")
    x_soft, u_soft, x_soft_max, u_soft_max = soft
    is_soft = x_soft is not None or u_soft is not None
    _check_caps("box_qp", "pdas", False, is_soft, x_soft_max is not None or u_soft_max is not None)   # the inner iteration takes caps
    if polish and is_soft:
        raise ValueError("box_qp: polish=True with method='alm' takes hard bounds only (the polish has no soft bounds)")
    with torch.no_grad():
        Gb, Cb, g, cc, lo, hi, wt, mt, Bt, batched, sol = _prepare("box_qp", blocks, *bounds, *soft)
        act = mu = None
        if warm is not None:
            act = _warm_act(warm, Bt, sol, g.device, "method='alm' starts from the act and the y of a previous method='alm' result")
            mu = getattr(warm, "y", None)
            if not isinstance(mu, torch.Tensor) or mu.numel() != Bt * sol.N or mu.dtype != g.dtype or mu.device != g.device:
                raise ValueError(f"box_qp: warm.y does not match this problem ({Bt} x {sol.N} {g.dtype} on {g.device})")
            mu = mu.detach().reshape(-1).contiguous()
        res = sol.box_qp_alm(Gb, Cb, g, cc, lo, hi, act=act, mu=mu, soft_weight=None if wt is None else wt.contiguous(),
                             soft_cap=None if mt is None else mt.contiguous(), **pol, **alm)
        if polish:
            act = res.act
            pact = sol.box_qp_active_set(res.z, res.y, lo, hi)
            sol.box_qp_polish(Gb, Cb, g, cc, lo, hi, pact, res, **pol)
            res.act = torch.where((res.polished == _lib.POLISH_ACCEPTED).repeat_interleave(sol.N), pact, act)
    return _shaped(res, sol, Bt, batched)


# ---- the differentiable layer -----------------------------------------------------------------------------------------
class _BoxQPLayer(torch.autograd.Function):
    """(G_blocks [B, G_dense], C_blocks [B, C_dense], g [B, N], c [B, S K], lo, hi [B, N], w [B, N] or None, m [B, N] or None)
    -> (x [B, N], lam [B, S K]) of the polished solution; box[0] receives the BoxQPResult.  w: the soft-bound weights, which
    make the forward pass the active-set iteration; None: hard bounds, by ADMM and the polish or (opts has max_pdas_iters) by
    the active-set iteration.  m (with w): the caps of the penalty forces.  The backward pass is one re-solve of the last
    assembly (the reduced system; with w, the weights of the soft-active variables that are not saturated on its diagonal) plus
    the gradient launches."""

    @staticmethod
    def forward(ctx, Gb, Cb, g, c, lo, hi, w, m, sol, opts, box):
        res, act, pol = _layer_solve(sol, Gb, Cb, g, c, lo, hi, w, m, opts)
        box.append(res)
        ctx.sol, ctx.pol, ctx.gen = sol, pol, sol.get_option("assembly_gen")
        ctx.codes = res.polished.cpu()
        x, lam = res.x.view(sol.batch, sol.N), res.lam.view(sol.batch, sol.sizes["sk"])
        ctx.save_for_backward(Gb, Cb, g, c, lo, hi, w, m, act, x, lam)
        ctx.save_for_forward(Gb, Cb, lo, hi, w, m, act, x, lam)
        ctx.set_materialize_grads(False)
        return x.clone(), lam.clone()

    @staticmethod
    def jvp(ctx, Gb_dot, Cb_dot, g_dot, c_dot, lo_dot, hi_dot, w_dot, m_dot, *_):
        """Forward mode, one direction.  It runs straight after its forward, so the assembly is the
        reduced system of the returned act; a stale one raises."""
        Gb, Cb, lo, hi, w, m, act, x, lam = ctx.saved_tensors
        _fresh(ctx.sol, ctx.gen, "box_qp_layer")
        dots = dict(G_dot=Gb_dot, C_dot=Cb_dot, g_dot=g_dot, c_dot=c_dot, lo_dot=lo_dot, hi_dot=hi_dot, w_dot=w_dot, m_dot=m_dot)
        x_dot, lam_dot = _layer_tangents(ctx.sol, 1, ctx.codes, ctx.pol, Gb, Cb, lo, hi, w, m, act, x, lam, _dots(dots, x.dtype))
        return x_dot[:, 0], lam_dot[:, 0]

    @staticmethod
    @once_differentiable
    def backward(ctx, x_bar, lam_bar):
        Gb, Cb, g, c, lo, hi, w, m, act, x, lam = ctx.saved_tensors
        sol, pol, need = ctx.sol, ctx.pol, ctx.needs_input_grad
        if x_bar is None and lam_bar is None:
            return (None,) * 11
        xb = torch.zeros_like(x) if x_bar is None else x_bar.to(x.dtype).contiguous()
        lb = torch.zeros_like(lam) if lam_bar is None else lam_bar.to(lam.dtype).contiguous()
        live = (~zero_rhs(xb, lb)).cpu()
        unpolished = live & (ctx.codes != _lib.POLISH_ACCEPTED)
        if unpolished.any():
            bad = unpolished.nonzero().flatten().tolist()
            raise RuntimeError(f"box_qp_layer: systems {bad} have a nonzero upstream gradient but their polish was not accepted "
                               f"(codes {ctx.codes[bad].tolist()}, _lib.POLISH_*): their x and lam are ADMM iterates (zeros "
                               "after method='pdas'), which have no gradient here")
        if not live.any():                   # every system's gradient is exactly zero: no re-solve (its PCG would form 0/0)
            return tuple(torch.zeros_like(t) if need[i] else None for i, t in enumerate((Gb, Cb, g, c, lo, hi, w, m))) + (None,) * 3
        if sol.get_option("assembly_gen") != ctx.gen or sol.get_option("assembly_valid") == 0:
            _rebuild_assembly(sol, Gb, Cb, g, c, lo, hi, w, m, act, x, lam, pol)   # another forward replaced the assembly
        # the reduced system reads x_bar off the hard-active set only (Ginv' has zero rows there; a soft-active variable is in
        # the system): with those masked, a system whose upstream gradient lives on its hard-active set alone has a zero
        # right-hand side, and _adjoint's zero test gives it a = beta = 0 instead of the PCG's 0/0
        hard = hard_active(act.view_as(xb), None if w is None else w.view_as(xb))
        xf = torch.where(hard, torch.zeros((), dtype=xb.dtype, device=xb.device), xb)
        a, beta = _adjoint(sol, lam, x, lb, xf, pol["exit_tol"], pol["max_iters"])
        Gbar = torch.empty_like(Gb) if need[0] else None
        Cbar = torch.empty_like(Cb) if need[1] else None
        if Gbar is not None or Cbar is not None:
            sol.kkt_grad_blocks(x, lam, a, beta, Gbar, Cbar)
        lo_bar = hi_bar = w_bar = m_bar = None
        if need[4] or need[5] or need[6] or need[7]:
            if w is None:
                lo_bar, hi_bar = sol.box_qp_bound_grad(Gb, Cb, act, xb, a, beta)
            elif m is not None:
                lo_bar, hi_bar, w_bar, m_bar = sol.box_qp_huber_grad(Gb, Cb, act, w.contiguous(), m.contiguous(), lo, hi,
                                                                     x.contiguous(), xb, a.contiguous(), beta.contiguous())
            else:
                lo_bar, hi_bar, w_bar = sol.box_qp_soft_grad(Gb, Cb, act, w.contiguous(), lo, hi, x.contiguous(), xb,
                                                             a.contiguous(), beta.contiguous())
        keep = live.to(x.device)[:, None]
        mask = lambda i, t: None if t is None or not need[i] else torch.where(keep, t.view(sol.batch, -1),
                                                                              torch.zeros((), dtype=t.dtype, device=t.device))
        return tuple(mask(i, t) for i, t in enumerate((Gbar, Cbar, a, beta, lo_bar, hi_bar, w_bar, m_bar))) + (None,) * 3


def _layer_solve(sol, Gb, Cb, g, c, lo, hi, w, m, opts):
    """The forward pass of the layer on packed inputs -> (BoxQPResult, act, the options of the polish); the solver's assembly is
    the reduced system of act afterwards."""
    opts = dict(opts)
    pdas_iters = opts.pop("max_pdas_iters", None)      # set: the active-set iteration alone (method="pdas")
    line_search = opts.pop("line_search", False)        # the forward pass only: the rebuild of a stale assembly is one solve
    pol = {k: opts[k] for k in ("rho", "exit_tol", "max_iters", "eps_abs", "eps_rel")}
    if w is not None or pdas_iters is not None:
        res = sol.box_qp_pdas(Gb, Cb, g, c, lo, hi, max_pdas_iters=pdas_iters, soft_weight=w, soft_cap=m,
                              line_search=line_search, **pol)
        act = res.act
    else:
        res = sol.box_qp(Gb, Cb, g, c, lo, hi, **opts)
        act = sol.box_qp_active_set(res.z, res.y, lo, hi)
        sol.box_qp_polish(Gb, Cb, g, c, lo, hi, act, res, **pol)
    return res, act, pol


def _layer_tangents(sol, R, codes, pol, Gb, Cb, lo, hi, w, m, act, x, lam, dots):
    """(x_dot [B, R, N], lam_dot [B, R, S K]) of the layer's point on the solver's current assembly (the reduced system of act)
    for the tangents dots (Solver.kkt_tangent_rhs's names, [B, R, ...]).  A system whose polish was not accepted raises
    RuntimeError if any of its tangents is nonzero, as the backward pass does for a nonzero upstream gradient, and gets zeros
    otherwise."""
    B = sol.batch
    live = torch.zeros(B, dtype=torch.bool, device=x.device)
    for t in dots.values():
        live |= t.view(B, -1).ne(0).any(1)
    live = live.cpu()
    unpolished = live & (codes != _lib.POLISH_ACCEPTED)
    if unpolished.any():
        bad = unpolished.nonzero().flatten().tolist()
        raise RuntimeError(f"box_qp_layer: systems {bad} have a nonzero input tangent but their polish was not accepted "
                           f"(codes {codes[bad].tolist()}, _lib.POLISH_*): their x and lam are ADMM iterates (zeros after "
                           "method='pdas'), which have no tangent here")
    if not live.any():                       # every tangent is exactly zero: no re-solve (its PCG would form 0/0)
        return (torch.zeros(B, R, sol.N, dtype=x.dtype, device=x.device),
                torch.zeros(B, R, sol.sizes["sk"], dtype=x.dtype, device=x.device))
    cont = lambda t: None if t is None else t.contiguous()
    lam_dot, x_dot = sol.tangents(R, x.contiguous(), lam.contiguous(), pol["exit_tol"], pol["max_iters"], Gb=Gb, Cb=Cb,
                                  act=act.reshape(-1), soft_weight=cont(w), soft_cap=cont(m), lo=lo.contiguous(),
                                  hi=hi.contiguous(), **dots)
    keep = (codes == _lib.POLISH_ACCEPTED).to(x.device)[:, None, None]
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    return torch.where(keep, x_dot, zero), torch.where(keep, lam_dot, zero)


def _rebuild_assembly(sol, Gb, Cb, g, c, lo, hi, w, m, act, x, lam, pol):
    """The assembly a backward pass re-solves, from the saved active set (it is a function of the inputs, the weights and act
    alone).  Hard bounds: the polish on act, its point into scratch copies; with weights w (and caps m: act may hold +-2): one
    solve of the active-set iteration from act, its point into tensors of its own."""
    if w is not None:
        sol.box_qp_pdas(Gb, Cb, g, c, lo, hi, max_pdas_iters=1, act=act, soft_weight=w, soft_cap=m, **pol)
        return
    res2 = torch.empty(sol.batch, 2, dtype=torch.float64, device=x.device)
    scratch = BoxQPResult(x.clone(), x.clone(), x.clone(), lam.clone(), None,
                          torch.empty(sol.batch, dtype=torch.int32, device=x.device), res2[:, 0], res2[:, 1])
    sol.box_qp_polish(Gb, Cb, g, c, lo, hi, act, scratch, **pol)


def box_qp_layer(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, *, rho, exit_tol, max_iters, admm_rho=0.1, sigma=1e-6,
                 alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_admm_iters=4000, check_every=25, method="admm", max_pdas_iters=30,
                 x_soft=None, u_soft=None, x_soft_max=None, u_soft_max=None, line_search=False):
    """Differentiable box-constrained QP: the inputs of box_qp; returns (x [*, N], lam [*, S K], info) with x and lam those
    of the polished solution, differentiable with respect to every tensor input (the bounds included; Q and R as symmetric,
    DESIGN.md section 3.6), and info a detached BoxQPResult (info.polished: the polish codes).  A system whose polish was not
    accepted returns its ADMM iterate; a backward pass through it with a nonzero upstream gradient raises RuntimeError.
    method="pdas": the forward pass is the active-set iteration alone (Solver.box_qp_pdas, cold start, at most max_pdas_iters
    reduced solves; the ADMM parameters are not read; a system that does not converge returns zeros); the backward pass is the
    same.  x_soft, u_soft (method="pdas" only): the soft-bound weights of box_qp; the layer is
    differentiable with respect to them too.  x_soft_max, u_soft_max (with x_soft / u_soft): the caps of box_qp (DESIGN.md section
    3.11); differentiable with respect to them as well (a cap's gradient is nonzero only on a saturated variable).
    line_search=True: box_qp's line search in the forward pass; the backward pass is unchanged - a
    converged point is the KKT point of its act.  rho is not differentiated and double backward is not supported."""
    _check_layer("box_qp_layer", method, x_soft is not None or u_soft is not None,
                 x_soft_max is not None or u_soft_max is not None, line_search)
    Gb, Cb, g, cc, lo, hi, wt, mt, Bt, batched, sol = _prepare("box_qp_layer", (Q, R, A, B, q, r, c), x_lo, x_hi, u_lo, u_hi,
                                                               x_soft, u_soft, x_soft_max, u_soft_max)
    if mt is not None:
        mt = mt.contiguous()
    opts = _layer_opts(method, max_pdas_iters, line_search, rho, exit_tol, max_iters, admm_rho, sigma, alpha, eps_abs, eps_rel,
                       max_admm_iters, check_every)
    box = []
    x, lam = _BoxQPLayer.apply(Gb, Cb, g, cc, lo, hi, wt, mt, sol, opts, box)
    info = _shaped(box[0], sol, Bt, batched)
    info = BoxQPResult(*(t.detach().clone() for t in (info.x, info.z, info.y, info.lam, info.iters, info.status, info.res_prim,
                                                      info.res_dual, info.polished)),
                       act=None if info.act is None else info.act.clone(), alpha=None if info.alpha is None else info.alpha.clone())
    return (x, lam, info) if batched else (x[0], lam[0], info)


def box_qp_layer_tangents(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, tangents, *, rho, exit_tol, max_iters, admm_rho=0.1,
                          sigma=1e-6, alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_admm_iters=4000, check_every=25, method="admm",
                          max_pdas_iters=30, x_soft=None, u_soft=None, x_soft_max=None, u_soft_max=None, line_search=False):
    """box_qp_layer and its forward-mode sensitivities along R directions in one call: the inputs of
    box_qp_layer and tangents, a dict from input name (Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, x_soft, u_soft, x_soft_max,
    u_soft_max) to a tensor of that input's full shape with one extra dimension R after the batch dimension (a bound's, weight's
    or cap's tangent may also be a number or a tensor that broadcasts to that shape); the given ones share R, a missing name is
    a zero tangent.  Returns (x [*, N], lam [*, S K], info, x_dot [*, R, N], lam_dot [*, R, S K]); nothing carries a grad_fn.
    The tangents are those of the returned act: the solution is piecewise smooth in its inputs.  A system whose polish was not
    accepted raises RuntimeError if one of its tangents is nonzero and gets zeros otherwise."""
    what = "box_qp_layer_tangents"
    soft = x_soft is not None or u_soft is not None
    capped = x_soft_max is not None or u_soft_max is not None
    _check_layer(what, method, soft, capped, line_search)
    with torch.no_grad():
        Gb, Cb, g, cc, lo, hi, wt, mt, Bt, batched, sol = _prepare(what, (Q, R, A, B, q, r, c), x_lo, x_hi, u_lo, u_hi, x_soft,
                                                                   u_soft, x_soft_max, u_soft_max)
        K, S, C = sol.K, sol.S, sol.C
        lead = (Bt,) if batched else ()
        shapes = dict(Q=(K, S, S), R=(K - 1, C, C), A=(K - 1, S, S), B=(K - 1, S, C), q=(K, S), r=(K - 1, C), c=(K, S))
        pairs = dict(lo=("x_lo", "u_lo"), hi=("x_hi", "u_hi"), w=("x_soft", "u_soft"), m=("x_soft_max", "u_soft_max"))
        vec = {n: (K, S) if n.startswith("x") else (K - 1, C) for p in pairs.values() for n in p}
        if not isinstance(tangents, dict):
            raise ValueError(f"{what}: tangents must be a non-empty dict of input name -> tensor")
        for name, have in (("x_soft", soft), ("u_soft", soft), ("x_soft_max", capped), ("u_soft_max", capped)):
            if name in tangents and not have:
                raise ValueError(f"{what}: a tangent of {name} needs the input itself")
        for name in shapes:
            if name in tangents and not isinstance(tangents[name], torch.Tensor):
                raise ValueError(f"{what}: the tangent of {name} must be a torch.Tensor")
        full = {n: t for n, t in tangents.items() if not (n in vec and (not isinstance(t, torch.Tensor) or t.dim() != len(lead) + 3))}
        Rn = _tangent_dims(full, dict(shapes, **vec), lead, what)
        dots = _pack_tangents({n: t for n, t in tangents.items() if n in shapes}, shapes, Bt, Rn, q)
        for key, (xn, un) in pairs.items():
            if xn in tangents or un in tangents:
                xv, uv = (_bound(tangents.get(n, 0.0), lead + (Rn,) + vec[n], n + " tangent", q, what).reshape((Bt * Rn,) + vec[n])
                          for n in (xn, un))
                dots[key + "_dot"] = _dz_layout(xv, uv)
        if mt is not None:
            mt = mt.contiguous()
        opts = _layer_opts(method, max_pdas_iters, line_search, rho, exit_tol, max_iters, admm_rho, sigma, alpha, eps_abs, eps_rel,
                           max_admm_iters, check_every)
        res, act, pol = _layer_solve(sol, Gb, Cb, g, cc, lo, hi, wt, mt, opts)
        x, lam = res.x.view(Bt, sol.N).clone(), res.lam.view(Bt, sol.sizes["sk"]).clone()
        x_dot, lam_dot = _layer_tangents(sol, Rn, res.polished.cpu(), pol, Gb, Cb, lo, hi, wt, mt, act, x, lam, _dots(dots, x.dtype))
        info = _shaped(res, sol, Bt, batched)
    return (x, lam, info, x_dot, lam_dot) if batched else (x[0], lam[0], info, x_dot[0], lam_dot[0])


STATUS = {_lib.QP_CONVERGED: "CONVERGED", _lib.QP_MAX_ITERS: "MAX_ITERS", _lib.QP_NONFINITE: "NONFINITE",
          _lib.QP_BAD_BOUNDS: "BAD_BOUNDS"}
