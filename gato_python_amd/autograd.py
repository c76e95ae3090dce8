"""torch autograd through the KKT solve.

    kkt_solve(Q, R, A, B, q, r, c, *, M=None, rho, exit_tol, max_iters) -> (lam, dz)
    kkt_solve_csr(G_row, G_col, G_val, C_row, C_col, C_val, g, c, *, cross=False, rho, exit_tol, max_iters) -> (lam, dz)
    kkt_solve_tangents(Q, R, A, B, q, r, c, tangents, *, M=None, rho, exit_tol, max_iters) -> (lam, dz, lam_dot, dz_dot)

The forward is the device solve (Solver.linsys_blocks / linsys / linsys_batched).  The backward is one re-solve of the same
assembly with the incoming gradients as right-hand side (the KKT matrix is symmetric, so the adjoint system has the forward's
matrix: Solver.solve_rhs), then one launch that forms the matrix gradients from dz, lambda and the adjoint (gato_grad.hip).
Forward mode: the tangent system has the same matrix, so a tangent is one launch for its right-hand side
(gato_tangent.hip) and the same re-solve - through torch.autograd.forward_ad dual tensors (the jvp of the Function, one direction)
or kkt_solve_tangents (R directions in one call).
One Function, _KktSolve, serves the four input forms (blocks, blocks with a cross term, CSR, CSR with cross entries); a _Form
record names what differs between them: the forward call, the gradient call and whether the re-solve is the cross one.
A cross term M goes through Solver.linsys_blocks_cross / solve_rhs_cross / kkt_grad_cross (reverse
mode); its forward mode is kkt_solve_tangents(..., M=M) over Solver.tangents_cross (section 3.17), not forward_ad dual tensors.
kkt_solve_csr(..., cross=True) reads the cross term from the CSR itself - G entries of state rows in
control columns - through Solver.linsys_cross and kkt_grad_csr_cross; cross=False is the path it was, which drops such entries.
Only device tensors are taken; there is no CPU fallback.  rho is not differentiated, and double backward is not supported.
"""
from __future__ import annotations

import ctypes as ct
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .solver import Solver, zero_rhs

_NP = {torch.float32: np.float32, torch.float64: np.float64}
_SOLVERS = {}


def _solver(S, C, K, B, dtype, device):
    """The cached Solver of one (S, C, K, B, dtype, device): every call of one shape shares its workspace."""
    key = (S, C, K, B, dtype, device)
    sol = _SOLVERS.get(key)
    if sol is None:
        sol = _SOLVERS[key] = Solver(S, C, K, _NP[dtype], device=device, batch=B)
    return sol


def _common(tensors, what):
    """device index and dtype shared by all value tensors; ValueError before any library call otherwise."""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} is on {t.device}: the solve runs on the GPU only (there is no CPU fallback)")
    devs = {t.device for t in tensors.values()}
    if len(devs) != 1:
        raise ValueError(f"{what}: the tensors are on different devices: {sorted(str(d) for d in devs)}")
    dts = {t.dtype for t in tensors.values()}
    if len(dts) != 1 or next(iter(dts)) not in _NP:
        raise ValueError(f"{what}: the values must share one dtype, float32 or float64; got {sorted(str(d) for d in dts)}")
    return next(iter(devs)).index, next(iter(dts))


def _check_blocks(args, what, qp=False):
    """The seven math-shaped blocks of `what` (a dict by name): all tensors, Q [*, K, S, S] with at most one leading batch
    dimension, R at least 2-D, every block of the shape that (K, S, C) and the batch set.  -> (batched, lead, K, S, C);
    ValueError before any library call otherwise.  qp: the entry is a box QP (K >= 2, and its messages name Q and R together
    and do not repeat the sizes; kkt_solve takes K = 1 and checks the sizes itself)."""
    for name, t in args.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    Q, R = args["Q"], args["R"]
    batched = Q.dim() == 4
    bad_Q = Q.dim() not in (3, 4) or Q.shape[-1] != Q.shape[-2]
    if qp and (bad_Q or R.dim() < 2):
        raise ValueError(f"{what}: Q must be [*, K, S, S] and R [*, K-1, C, C], got {tuple(Q.shape)} and {tuple(R.shape)}")
    if bad_Q:
        raise ValueError(f"{what}: Q must be [*, K, S, S], got {tuple(Q.shape)}")
    if R.dim() < 2:
        raise ValueError(f"{what}: R must be [*, K-1, C, C], got {tuple(R.shape)}")
    K, S, C = Q.shape[-3], Q.shape[-1], R.shape[-1]
    if qp and K < 2:
        raise ValueError(f"{what}: K = {K}: at least two knots")
    lead = (Q.shape[0],) if batched else ()
    sizes = "" if qp else f" (S = {S}, C = {C}, K = {K}{', batch %d' % lead[0] if lead else ''})"
    want = dict(Q=(K, S, S), R=(K - 1, C, C), A=(K - 1, S, S), B=(K - 1, S, C), q=(K, S), r=(K - 1, C), c=(K, S))
    for name, shp in want.items():
        if tuple(args[name].shape) != lead + shp:
            raise ValueError(f"{what}: {name} has shape {tuple(args[name].shape)}, want {lead + shp}{sizes}")
    return batched, lead, K, S, C


def _opts(rho, exit_tol, max_iters):
    return float(rho), float(exit_tol), int(max_iters)


# ---- the one Function and its four input forms ----------------------------------------------------------------------------
class _Form(NamedTuple):
    """What one input form of the KKT solve gives _KktSolve.  vals: the form's matrix tensors, in the order of apply; idx: the
    CSR forms' (G_row, G_col, C_row, C_col), None for blocks; opts: (rho, exit_tol, max_iters)."""
    forward: Callable       # (sol, idx, vals, g, c, opts, lam, dz): the whole solve and check_status; lam = dz = None: into the solver's own
    grad: Callable          # (sol, idx, vals, dz, lam, a, beta, need) -> the bars of vals, None where need (one flag per val) is False
    cross: bool             # the assembly is a cross solve's: the adjoint re-solve is solve_rhs_cross
    no_jvp: Optional[str]   # why forward_ad raises NotImplementedError; None: the tangent of the blocks form


def _blocks_forward(sol, idx, vals, g, c, opts, lam, dz):
    rho, exit_tol, max_iters = opts
    sol.linsys_blocks(*vals, g, c, exit_tol, max_iters, rho, lam, dz)      # Cb itself: a re-solve reads the caller's C blocks again
    sol.check_status()


def _blocks_cross_forward(sol, idx, vals, g, c, opts, lam, dz):
    rho, exit_tol, max_iters = opts
    sol.linsys_blocks_cross(*vals, g, c, exit_tol, max_iters, rho, lam, dz)
    sol.check_status()


def _csr_forward(sol, idx, vals, g, c, opts, lam, dz):
    rho, exit_tol, max_iters = opts
    G_row, G_col, C_row, C_col = idx
    G_val, C_val = vals
    if sol.batch == 1:
        sol.linsys(G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam, dz)
    else:
        sol.linsys_batched(G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam, dz)
    sol.check_status()


def _csr_cross_forward(sol, idx, vals, g, c, opts, lam, dz):
    rho, exit_tol, max_iters = opts
    G_row, G_col, C_row, C_col = idx
    G_val, C_val = vals
    sol.linsys_cross(G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam, dz)
    sol.check_status()


def _pair_grad(call, vals, need):
    """(G_bar, C_bar) like vals where need says so, filled by one call(G_bar, C_bar) unless neither is wanted."""
    Gbar, Cbar = (torch.empty_like(v) if n else None for v, n in zip(vals, need))
    if Gbar is not None or Cbar is not None:
        call(Gbar, Cbar)
    return Gbar, Cbar


def _blocks_grad(sol, idx, vals, dz, lam, a, beta, need):
    return _pair_grad(lambda Gbar, Cbar: sol.kkt_grad_blocks(dz, lam, a, beta, Gbar, Cbar), vals, need)


def _blocks_cross_grad(sol, idx, vals, dz, lam, a, beta, need):
    Gb, Mb, Cb = vals
    Gbar, Cbar = _blocks_grad(sol, idx, (Gb, Cb), dz, lam, a, beta, (need[0], need[2]))
    Mbar = torch.empty_like(Mb) if need[1] else None
    if Mbar is not None and Mbar.numel():
        sol.kkt_grad_cross(dz, a, Mbar)
    return Gbar, Mbar, Cbar


def _csr_grad(sol, idx, vals, dz, lam, a, beta, need):
    return _pair_grad(lambda Gbar, Cbar: sol.kkt_grad_csr(*idx, dz, lam, a, beta, Gbar, Cbar), vals, need)


def _csr_cross_grad(sol, idx, vals, dz, lam, a, beta, need):
    return _pair_grad(lambda Gbar, Cbar: sol.kkt_grad_csr_cross(*idx, dz, lam, a, beta, Gbar, Cbar), vals, need)


# vals: (G_blocks [B, G_dense], C_blocks [B, C_dense]); with a cross term (G_blocks, M_blocks [B, (K-1) S C], C_blocks); the CSR
# pair (G_val [B, nnz_G], C_val [B, nnz_C]) on a shared pattern
_BLOCKS = _Form(_blocks_forward, _blocks_grad, False, None)
_BLOCKS_CROSS = _Form(_blocks_cross_forward, _blocks_cross_grad, True,
                      "kkt_solve: forward mode with a cross term M is not built through torch.autograd.forward_ad "
                      "(DESIGN.md section 3.17); use kkt_solve_tangents(..., M=M) for R directions in one call, or reverse mode")
_CSR = _Form(_csr_forward, _csr_grad, False,
             "kkt_solve_csr: forward mode is not built through torch.autograd.forward_ad; use kkt_solve_tangents on blocks, or "
             "reverse mode")
_CSR_CROSS = _Form(_csr_cross_forward, _csr_cross_grad, True,
                   "kkt_solve_csr: forward mode with cross=True is not built through torch.autograd.forward_ad "
                   "(DESIGN.md sections 3.17, 3.18); use kkt_solve_tangents(..., M=M) on blocks, or reverse mode")


class _KktSolve(torch.autograd.Function):
    """(g [B, N], c [B, S K], *vals of the form) -> (lam [B, S K], dz [B, N]) of the original problem."""

    @staticmethod
    def forward(ctx, form, idx, sol, rho, exit_tol, max_iters, g, c, *vals):
        B = sol.batch
        lam = torch.empty(B, sol.sizes["sk"], dtype=g.dtype, device=g.device)
        dz = torch.empty(B, sol.N, dtype=g.dtype, device=g.device)
        opts = (rho, exit_tol, max_iters)
        form.forward(sol, idx, vals, g, c, opts, lam, dz)
        ctx.form, ctx.idx, ctx.sol, ctx.opts, ctx.gen = form, idx, sol, opts, sol.get_option("assembly_gen")
        ctx.save_for_backward(g, c, lam, dz, *vals)
        if form.no_jvp is None:
            ctx.save_for_forward(lam, dz)
        ctx.set_materialize_grads(False)
        return lam, dz

    @staticmethod
    def jvp(ctx, *dots):
        """Forward mode, one direction, the blocks form only: the tangent right-hand side and one
        re-solve.  It runs straight after its forward, so the assembly is the forward's; a stale one raises."""
        if ctx.form.no_jvp is not None:
            raise NotImplementedError(ctx.form.no_jvp)
        lam, dz = ctx.saved_tensors
        sol = ctx.sol
        _, exit_tol, max_iters = ctx.opts
        _fresh(sol, ctx.gen, "kkt_solve")
        g_dot, c_dot, Gb_dot, Cb_dot = dots[6:]
        given = dict(G_dot=Gb_dot, C_dot=Cb_dot, g_dot=g_dot, c_dot=c_dot)
        lam_dot, dz_dot = sol.tangents(1, dz, lam, exit_tol, max_iters, **_dots(given, dz.dtype))
        return lam_dot[:, 0], dz_dot[:, 0]

    @staticmethod
    @once_differentiable
    def backward(ctx, lam_bar, dz_bar):
        g, c, lam, dz, *vals = ctx.saved_tensors
        form, idx, sol = ctx.form, ctx.idx, ctx.sol
        _, exit_tol, max_iters = ctx.opts
        if lam_bar is None and dz_bar is None:
            return (None,) * (8 + len(vals))
        if sol.get_option("assembly_gen") != ctx.gen or sol.get_option("assembly_valid") == 0:
            form.forward(sol, idx, vals, g, c, ctx.opts, None, None)      # another forward replaced the assembly
        a, beta = _adjoint(sol, lam, dz, lam_bar, dz_bar, exit_tol, max_iters, cross=form.cross)
        need = ctx.needs_input_grad
        bars = form.grad(sol, idx, vals, dz, lam, a, beta, need[8:])
        return (None,) * 6 + (a if need[6] else None, beta if need[7] else None) + tuple(bars)


def _fresh(sol, gen, what):
    """RuntimeError unless the solver's assembly is still that of generation gen: a tangent re-solves it and never rebuilds it."""
    if sol.get_option("assembly_gen") != gen or sol.get_option("assembly_valid") == 0:
        raise RuntimeError(f"{what}: another solve replaced this forward pass's assembly before its tangent was taken; forward "
                           "mode re-solves the assembly of its own forward pass (take the tangent before the next solve of this shape)")


def _dots(dots, dtype):
    """The given tangents (None: zero, dropped) as contiguous tensors of dtype."""
    return {k: t.to(dtype).contiguous() for k, t in dots.items() if t is not None}


def _adjoint(sol, lam, dz, lam_bar, dz_bar, exit_tol, max_iters, cross=False):
    """[a; beta] = M^-1 [dz_bar; lam_bar]: one re-solve of the current assembly (a missing gradient is zero).  cross: the
    assembly is a cross solve's and the re-solve is solve_rhs_cross (the adjoint in the original variables)."""
    gin = torch.zeros_like(dz) if dz_bar is None else dz_bar.to(dz.dtype).contiguous()
    cin = torch.zeros_like(lam) if lam_bar is None else lam_bar.to(lam.dtype).contiguous()
    sol.reserve_rhs(1)
    beta, a, _ = (sol.solve_rhs_cross if cross else sol.solve_rhs)(gin, cin, exit_tol, max_iters)
    sol.check_status()              # a hand-off time-out (iters = -1) raises, as in the forward; running to max_iters does not
    zero = zero_rhs(gin, cin)[:, None]          # such a system has a zero adjoint; its PCG would divide 0 by 0 instead
    return torch.where(zero, 0, a.view_as(dz)), torch.where(zero, 0, beta.view_as(lam))


def _pack(Q, R, A, B, q, r, c):
    """Math-shaped blocks [Bt, ...] -> the solver's G_dense / C_dense / g / c layouts, in torch ops (torch differentiates them)."""
    Bt, K, S, _ = Q.shape
    C = R.shape[-1]
    Qf = Q.transpose(-1, -2).reshape(Bt, K, S * S)                 # column-major per knot
    Rf = R.transpose(-1, -2).reshape(Bt, K - 1, C * C)
    Gb = torch.cat([torch.cat([Qf[:, :K - 1], Rf], 2).reshape(Bt, -1), Qf[:, K - 1]], 1)
    Af = A.transpose(-1, -2).reshape(Bt, K - 1, S * S)
    Bf = B.transpose(-1, -2).reshape(Bt, K - 1, S * C)
    Cb = torch.cat([Af, Bf], 2).reshape(Bt, -1)
    return Gb.contiguous(), Cb.contiguous(), _dz_layout(q, r), c.reshape(Bt, -1).contiguous()


def _dz_layout(xv, uv):
    """Per-knot values xv [Bt, K, S] and uv [Bt, K-1, C] -> the dz layout [Bt, N]: (x_k, u_k) per knot, then x_{K-1}."""
    Bt, K = xv.shape[:2]
    return torch.cat([torch.cat([xv[:, :K - 1], uv], 2).reshape(Bt, -1), xv[:, K - 1]], 1).contiguous()


def _check_cross(M, lead, K, S, C, ref, what):
    """M [*, K-1, S, C] of ref's dtype and device; ValueError before any solver is created otherwise."""
    if not isinstance(M, torch.Tensor):
        raise ValueError(f"{what}: M must be a torch.Tensor, got {type(M).__name__}")
    if tuple(M.shape) != lead + (K - 1, S, C):
        raise ValueError(f"{what}: M has shape {tuple(M.shape)}, want {lead + (K - 1, S, C)} (S = {S}, C = {C}, K = {K})")
    if M.dtype != ref.dtype:
        raise ValueError(f"{what}: M is {M.dtype}, the other values are {ref.dtype}")
    if M.device != ref.device:
        raise ValueError(f"{what}: M is on {M.device}, the other values are on {ref.device}")


def kkt_solve(Q, R, A, B, q, r, c, *, M=None, rho, exit_tol, max_iters):
    """Differentiable KKT solve from math-shaped blocks, at most one leading batch dimension:
    Q [*,K,S,S], R [*,K-1,C,C], A [*,K-1,S,S], B [*,K-1,S,C], q [*,K,S], r [*,K-1,C], c [*,K,S] (A, B as stored in C: the
    raw values, -A and -B of the dynamics).  Returns flat lam [*, S K] and dz [*, N], as linsys_solve does.
    Q, R are taken as symmetric: their gradients are those of symmetric perturbations.
    M [*,K-1,S,C]: the stage cost gains x_k^T M_k u_k, G_k = [[Q_k, M_k], [M_k^T, R_k]]; every G_k + rho I
    must be positive definite (not checked).  Its gradient is that of M_k and M_k^T perturbed together.  Reverse mode only:
    under torch.autograd.forward_ad a given M raises NotImplementedError.  M=None is the solve without a cross term."""
    args = dict(Q=Q, R=R, A=A, B=B, q=q, r=r, c=c)
    batched, lead, K, S, C = _check_blocks(args, "kkt_solve")
    if K < 1 or S < 1 or C < 1:
        raise ValueError(f"kkt_solve: S = {S}, C = {C}, K = {K} must all be >= 1")
    if M is not None:
        _check_cross(M, lead, K, S, C, Q, "kkt_solve")
    device, dtype = _common(args, "kkt_solve")
    blocks = (Q, R, A, B, q, r, c) if batched else tuple(t.unsqueeze(0) for t in (Q, R, A, B, q, r, c))
    Bt = blocks[0].shape[0]
    rho, exit_tol, max_iters = _opts(rho, exit_tol, max_iters)
    Gb, Cb, g, cc = _pack(*blocks)
    form, vals = _BLOCKS, (Gb, Cb)
    if M is not None:                                                      # M in the layout of B: column-major per knot
        form, vals = _BLOCKS_CROSS, (Gb, M.transpose(-1, -2).reshape(Bt, (K - 1) * S * C).contiguous(), Cb)
    sol = _solver(S, C, K, Bt, dtype, device)
    lam, dz = _KktSolve.apply(form, None, sol, rho, exit_tol, max_iters, g, cc, *vals)
    return (lam, dz) if batched else (lam[0], dz[0])


def _tangent_dims(tangents, shapes, lead, what):
    """R of the explicit tangents (a dict name -> tensor of its input's shape with one extra dimension R after the batch
    dimension; all given ones share R); ValueError for an unknown name, a wrong shape or no tangent at all."""
    if not isinstance(tangents, dict) or not tangents:
        raise ValueError(f"{what}: tangents must be a non-empty dict of input name -> tensor")
    unknown = sorted(set(tangents) - set(shapes))
    if unknown:
        raise ValueError(f"{what}: tangents names {unknown}; the inputs are {sorted(shapes)}")
    R = None
    for name, t in tangents.items():
        if not isinstance(t, torch.Tensor):
            continue                                                      # a number: broadcast (bounds only, checked by the caller)
        nl = len(lead)
        if t.dim() != nl + 1 + len(shapes[name]) or tuple(t.shape[:nl]) != lead or tuple(t.shape[nl + 1:]) != shapes[name]:
            raise ValueError(f"{what}: the tangent of {name} has shape {tuple(t.shape)}, want {lead + ('R',) + shapes[name]}")
        if R is not None and t.shape[nl] != R:
            raise ValueError(f"{what}: the tangents do not share one R ({R} and {t.shape[nl]})")
        R = t.shape[nl]
    if R is None or R < 1:
        raise ValueError(f"{what}: at least one tangent must be a tensor with R >= 1 directions")
    return R


def _pack_tangents(tangents, shapes, Bt, R, ref):
    """The block tangents [Bt, R, ...] in the solver's layouts [Bt, R, G_dense] etc. by _pack on Bt R systems; a pair (Q, R),
    (A, B) or (q, r) neither of which is given stays None, c likewise."""
    def full(name):
        t = tangents.get(name)
        return torch.zeros((Bt * R,) + shapes[name], dtype=ref.dtype, device=ref.device) if t is None \
            else t.detach().to(ref.dtype).reshape((Bt * R,) + shapes[name])
    Gd, Cd, gd, cd = _pack(*(full(n) for n in "Q R A B q r c".split()))
    have = lambda *names: any(n in tangents for n in names)
    return dict(G_dot=Gd if have("Q", "R") else None, C_dot=Cd if have("A", "B") else None, g_dot=gd if have("q", "r") else None,
                c_dot=cd if have("c") else None)


def kkt_solve_tangents(Q, R, A, B, q, r, c, tangents, *, M=None, rho, exit_tol, max_iters):
    """kkt_solve and its forward-mode sensitivities along R directions in one call:
    -> (lam [*, S K], dz [*, N], lam_dot [*, R, S K], dz_dot [*, R, N]).  tangents: a dict from input name (Q, R, A, B, q, r,
    c) to a tensor of that input's shape with one extra dimension R after the batch dimension; the given ones share R, a
    missing name is a zero tangent.  Q and R tangents are used as given (symmetric perturbations).  One solve, one launch for the
    R right-hand sides, one re-solve for all of them.  Nothing returned carries a grad_fn.
    M [*, K-1, S, C]: the cross term of kkt_solve; tangents may then name "M" as well, [*, R, K-1, S, C],
    used as given (M_k and M_k^T perturbed together, the convention of kkt_solve's gradient of M).  One launch more: the map
    back to the original variables.  M=None is the call without a cross term."""
    what = "kkt_solve_tangents"
    args = dict(Q=Q, R=R, A=A, B=B, q=q, r=r, c=c)
    batched, lead, K, S, C = _check_blocks(args, what)
    if K < 1 or S < 1 or C < 1:
        raise ValueError(f"{what}: S = {S}, C = {C}, K = {K} must all be >= 1")
    shapes = dict(Q=(K, S, S), R=(K - 1, C, C), A=(K - 1, S, S), B=(K - 1, S, C), q=(K, S), r=(K - 1, C), c=(K, S))
    if M is not None:                                                      # M and its tangent: checked before any device is asked for
        _check_cross(M, lead, K, S, C, Q, what)
        shapes["M"] = (K - 1, S, C)
        _tangent_dims(tangents, shapes, lead, what)
    elif isinstance(tangents, dict) and "M" in tangents:
        raise ValueError(f"{what}: a tangent of M needs the input itself (M=...)")
    device, dtype = _common(args, what)
    Rn = _tangent_dims(tangents, shapes, lead, what)
    _common(dict(tangents, q=q), what)
    rho, exit_tol, max_iters = _opts(rho, exit_tol, max_iters)
    with torch.no_grad():
        blocks = [t if batched else t.unsqueeze(0) for t in (Q, R, A, B, q, r, c)]
        Bt = blocks[0].shape[0]
        Gb, Cb, g, cc = _pack(*blocks)
        sol = _solver(S, C, K, Bt, dtype, device)
        lam = torch.empty(Bt, sol.sizes["sk"], dtype=dtype, device=g.device)
        dz = torch.empty(Bt, sol.N, dtype=dtype, device=g.device)
        dots = _pack_tangents({n: t for n, t in tangents.items() if n != "M"}, shapes, Bt, Rn, q)
        if M is None or K == 1:                                            # K = 1 has no M at all: the plain path
            sol.linsys_blocks(Gb, Cb, g, cc, exit_tol, max_iters, rho, lam, dz)
            sol.check_status()
            lam_dot, dz_dot = sol.tangents(Rn, dz, lam, exit_tol, max_iters, **_dots(dots, dtype))
        else:
            Mb = M.detach().reshape(Bt, K - 1, S, C).transpose(-1, -2).reshape(Bt, -1).contiguous()      # column-major per knot
            sol.linsys_blocks_cross(Gb, Mb, Cb, g, cc, exit_tol, max_iters, rho, lam, dz)
            sol.check_status()
            Md = tangents.get("M")
            if Md is not None:
                dots["M_dot"] = Md.detach().reshape(Bt * Rn, K - 1, S, C).transpose(-1, -2).reshape(Bt, -1)
            lam_dot, dz_dot = sol.tangents_cross(Rn, dz, lam, exit_tol, max_iters, **_dots(dots, dtype))
    return (lam, dz, lam_dot, dz_dot) if batched else (lam[0], dz[0], lam_dot[0], dz_dot[0])


# ---- CSR form ----------------------------------------------------------------------------------------------------------
def _index(t, name, what, device):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != device:
        raise ValueError(f"{what}: {name} must be a CUDA tensor on cuda:{device} (there is no CPU fallback)")
    if t.dtype not in (torch.int32, torch.int64) or t.dim() != 1:
        raise ValueError(f"{what}: {name} must be a 1-D int32 / int64 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.to(torch.int32).contiguous()


def _check_pattern(G_row, G_col, C_row, C_col, N, host=None):
    """The scatter kernels trust the indices (as the reference does): refuse, on the host, what would send them out of range.
    host: a dict that receives the host copies made here (G_row, G_col, C_row, C_col)."""
    for name, ptr, col in (("G", G_row, G_col), ("C", C_row, C_col)):
        p, cidx = ptr.cpu().numpy(), col.cpu().numpy()
        if host is not None:
            host[name + "_row"], host[name + "_col"] = p, cidx
        if p[0] < 0 or p[-1] > cidx.size or np.any(np.diff(p) < 0):
            raise ValueError(f"kkt_solve_csr: {name}_row must rise from >= 0 to <= len({name}_col) = {cidx.size}")
        if cidx.size and (cidx.min() < 0 or cidx.max() >= N):
            raise ValueError(f"kkt_solve_csr: {name}_col holds an index outside [0, {N})")
    return C_row.cpu().numpy()


def _check_mirrors(G_row_host, G_col_host, S, C, K):
    """cross=True reads the cross term from the state rows only: a mirror entry (control row, state column) whose state-row
    partner is not stored would be dropped silently - ValueError instead.  Upper-only storage passes.  The partner is looked
    for the way the scatter addresses: the mirror entry stands for M_k[col % n, row % n - S] with k = row // n, and the partner is
    a kept entry of that slot - a state row of the same knot (control rows exist below the last knot only, so it has an M) in a
    column that folds to row % n, whichever knot that column lies in."""
    n, N = S + C, (S + C) * K - C
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(np.asarray(G_row_host, np.int64)))
    col = np.asarray(G_col_host, np.int64)[int(G_row_host[0]):int(G_row_host[0]) + row.size]
    knot, isr, isc = row // n, row % n, col % n
    mirror = (isr >= S) & (isc < S)
    if not mirror.any():
        return
    kept = (isr < S) & (isc >= S) & (knot < K - 1)
    slot = lambda a, b: (knot * n + a) * n + b              # (knot, state row, control column) of an M slot
    lone = mirror & ~np.isin(slot(isc, isr), slot(isr, isc)[kept])
    if lone.any():
        e = int(np.flatnonzero(lone)[0])
        raise ValueError(f"kkt_solve_csr: cross=True reads G's cross term from the state rows, and {int(lone.sum())} entries of "
                         f"control rows in state columns have no partner there (the first: row {int(row[e])}, column "
                         f"{int(col[e])}, no entry at row {int(knot[e] * n + isc[e])}, column {int(row[e])}); store the upper "
                         f"triangle or both")


def _infer_shape(C_row_host, len_g, len_c):
    h = np.ascontiguousarray(C_row_host, np.int32)
    S, C, K = ct.c_int(), ct.c_int(), ct.c_int()
    rc = _lib.lib().gato_infer_shape(h.ctypes.data_as(ct.c_void_p), len(h), len_g, len_c, ct.byref(S), ct.byref(C),
                                     ct.byref(K))
    if rc != 0:
        raise ValueError("kkt_solve_csr: " + _lib.lib().gato_last_error().decode())
    return S.value, C.value, K.value


def _cross_pattern(G_row, G_col, C_row, C_col, N, SK):
    """The host-side checks of kkt_solve_csr(cross=True), before any device is asked for: index tensors on any device, the
    pattern in range, (S, C, K), no mirror entry without its partner.  -> (S, C, K)."""
    what = "kkt_solve_csr"
    for name, t in (("G_row", G_row), ("G_col", G_col), ("C_row", C_row), ("C_col", C_col)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64) or t.dim() != 1:
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} must be a 1-D int32 / int64 tensor, got {got}")
    if G_row.numel() != N + 1 or C_row.numel() != SK + 1:
        raise ValueError(f"{what}: len(G_row) = {G_row.numel()} and len(C_row) = {C_row.numel()}, want N + 1 = {N + 1} and "
                         f"S K + 1 = {SK + 1}")
    host = {}
    S, C, K = _infer_shape(_check_pattern(G_row, G_col, C_row, C_col, N, host), N, SK)
    _check_mirrors(host["G_row"], host["G_col"], S, C, K)
    return S, C, K


def kkt_solve_csr(G_row, G_col, G_val, C_row, C_col, C_val, g, c, *, cross=False, rho, exit_tol, max_iters):
    """Differentiable KKT solve on CSR input (gpu_library.linsys_solve's arrays, on the device).  Differentiable in G_val,
    C_val, g and c; the indices are shared by a batch: values [B, nnz] / g [B, N] / c [B, S K], or unbatched [nnz] / [N] /
    [S K].  The gradient of a value is that of the dense slot the scatter writes it into - 0 where the scatter drops it or a
    later entry of its row overwrites it.  (S, C, K) come from the lengths and C's leading identity rows.
    cross=False: G entries between the Q and R parts (a state row with a control column and its mirror) are dropped, as the
    reference's scatter drops them.  cross=True: a G entry of a state row of knot k < K-1 in a control
    column is M_k[row % n, col % n - S] of the stage cost's cross term x_k^T M_k u_k; its gradient is that of M_k and M_k^T
    perturbed together.  The mirror entries in the control rows are not read and get a zero gradient (G is taken as symmetric;
    upper-only storage is accepted, a mirror entry without its state-row partner raises ValueError), rho is added to every
    diagonal entry of G whether the CSR stores it or not, and every G_k + rho I must be positive definite (not checked).
    Reverse mode only: under torch.autograd.forward_ad it raises NotImplementedError."""
    what = "kkt_solve_csr"
    vals = dict(G_val=G_val, C_val=C_val, g=g, c=c)
    for name, t in vals.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    batched = g.dim() == 2
    if any(t.dim() != (2 if batched else 1) for t in vals.values()):
        raise ValueError(f"{what}: G_val, C_val, g, c must all be 1-D or all [B, ...]: "
                         f"{[tuple(t.shape) for t in vals.values()]}")
    Bt = g.shape[0] if batched else 1
    if batched and any(t.shape[0] != Bt for t in vals.values()):
        raise ValueError(f"{what}: the batch sizes differ: {[tuple(t.shape) for t in vals.values()]}")
    shape = _cross_pattern(G_row, G_col, C_row, C_col, g.shape[-1], c.shape[-1]) if cross else None
    device, dtype = _common(vals, what)
    G_row, G_col, C_row, C_col = (_index(t, n, what, device) for t, n in
                                  ((G_row, "G_row"), (G_col, "G_col"), (C_row, "C_row"), (C_col, "C_col")))
    if G_val.shape[-1] != G_col.numel() or C_val.shape[-1] != C_col.numel():
        raise ValueError(f"{what}: G_val / C_val hold {G_val.shape[-1]} / {C_val.shape[-1]} values per system, G_col / C_col "
                         f"{G_col.numel()} / {C_col.numel()} indices")
    N, SK = g.shape[-1], c.shape[-1]
    if shape is None and (G_row.numel() != N + 1 or C_row.numel() != SK + 1):       # _cross_pattern has checked the lengths
        raise ValueError(f"{what}: len(G_row) = {G_row.numel()} and len(C_row) = {C_row.numel()}, want N + 1 = {N + 1} and "
                         f"S K + 1 = {SK + 1}")
    S, C, K = shape if cross else _infer_shape(_check_pattern(G_row, G_col, C_row, C_col, N), N, SK)
    rho, exit_tol, max_iters = _opts(rho, exit_tol, max_iters)
    G_val2, C_val2, g2, c2 = (t.reshape(Bt, -1).contiguous() for t in (G_val, C_val, g, c))
    sol = _solver(S, C, K, Bt, dtype, device)
    lam, dz = _KktSolve.apply(_CSR_CROSS if cross else _CSR, (G_row, G_col, C_row, C_col), sol, rho, exit_tol, max_iters, g2, c2, G_val2, C_val2)
    return (lam, dz) if batched else (lam[0], dz[0])
