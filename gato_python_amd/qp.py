"""Box-constrained QP solves from math-shaped blocks.

    box_qp(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, *, rho, exit_tol, max_iters, ...) -> BoxQPResult

solves  min 1/2 x^T (G + rho I) x - g^T x  s.t.  C x = c,  lo <= x <= hi  - the KKT system of autograd.kkt_solve plus bounds on
the states and controls - by ADMM over the device re-solve (Solver.box_qp, gato_box_qp_solve).  It is NOT differentiable: the
inputs are read detached and the outputs carry no grad_fn.  Only device tensors are taken; there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from .autograd import _common, _pack, _solver
from .solver import BoxQPResult


def _bound(v, shape, name, ref):
    """A bound as a tensor of `shape` (a Python number or a tensor that broadcasts to it), in ref's dtype and device."""
    if not isinstance(v, torch.Tensor):
        return torch.full(shape, float(v), dtype=ref.dtype, device=ref.device)
    if v.device != ref.device or v.dtype != ref.dtype:
        raise ValueError(f"box_qp: {name} must be a {ref.dtype} tensor on {ref.device}, got {v.dtype} on {v.device}")
    try:
        return v.detach().expand(shape)
    except RuntimeError:
        raise ValueError(f"box_qp: {name} of shape {tuple(v.shape)} does not broadcast to {shape}") from None


def box_qp(Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi, *, rho, exit_tol, max_iters, admm_rho=0.1, sigma=1e-6, alpha=1.6,
           eps_abs=1e-6, eps_rel=1e-6, max_admm_iters=4000, check_every=25, warm=None):
    """Box-constrained QP from math-shaped blocks, at most one leading batch dimension:
    Q [*,K,S,S], R [*,K-1,C,C], A [*,K-1,S,S], B [*,K-1,S,C], q [*,K,S], r [*,K-1,C], c [*,K,S] as kkt_solve takes them (A, B
    the raw values stored in C: -A and -B of the dynamics), and the bounds x_lo, x_hi [*,K,S], u_lo, u_hi [*,K-1,C] - numbers
    or tensors that broadcast to those shapes, +-inf allowed.  warm: a previous BoxQPResult of the same shape (its z, y and
    lam start the iteration).  Returns a BoxQPResult with flat x, z, y [*, N], lam [*, S K] (dz layout, as kkt_solve returns
    dz and lam) and iters, status, res_prim, res_dual [*] (scalars unbatched).  Raises ValueError for lo > hi or a NaN bound."""
    args = dict(Q=Q, R=R, A=A, B=B, q=q, r=r, c=c)
    for name, t in args.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"box_qp: {name} must be a torch.Tensor, got {type(t).__name__}")
    batched = Q.dim() == 4
    if Q.dim() not in (3, 4) or Q.shape[-1] != Q.shape[-2] or R.dim() < 2:
        raise ValueError(f"box_qp: Q must be [*, K, S, S] and R [*, K-1, C, C], got {tuple(Q.shape)} and {tuple(R.shape)}")
    K, S, C = Q.shape[-3], Q.shape[-1], R.shape[-1]
    if K < 2:
        raise ValueError(f"box_qp: K = {K}: at least two knots")
    lead = (Q.shape[0],) if batched else ()
    want = dict(Q=(K, S, S), R=(K - 1, C, C), A=(K - 1, S, S), B=(K - 1, S, C), q=(K, S), r=(K - 1, C), c=(K, S))
    for name, shp in want.items():
        if tuple(args[name].shape) != lead + shp:
            raise ValueError(f"box_qp: {name} has shape {tuple(args[name].shape)}, want {lead + shp}")
    _common(args, "box_qp")
    with torch.no_grad():
        xl, xh = (_bound(v, lead + (K, S), n, q) for v, n in ((x_lo, "x_lo"), (x_hi, "x_hi")))
        ul, uh = (_bound(v, lead + (K - 1, C), n, q) for v, n in ((u_lo, "u_lo"), (u_hi, "u_hi")))
        if not batched:
            Q, R, A, B, q, r, c, xl, xh, ul, uh = (t.unsqueeze(0) for t in (Q, R, A, B, q, r, c, xl, xh, ul, uh))
        Bt = Q.shape[0]
        Gb, Cb, g, cc = _pack(*(t.detach() for t in (Q, R, A, B, q, r, c)))
        # the bounds in the dz layout: the same packing as q / r into g
        lo = torch.cat([torch.cat([xl[:, :K - 1], ul], 2).reshape(Bt, -1), xl[:, K - 1]], 1).contiguous()
        hi = torch.cat([torch.cat([xh[:, :K - 1], uh], 2).reshape(Bt, -1), xh[:, K - 1]], 1).contiguous()
        sol = _solver(S, C, K, Bt, g.dtype, g.device.index)
        out = {}
        if warm is not None:
            for name in ("z", "y", "lam"):
                t = getattr(warm, name)
                n = sol.sizes["sk"] if name == "lam" else sol.N
                if not isinstance(t, torch.Tensor) or t.numel() != Bt * n or t.dtype != g.dtype or t.device != g.device:
                    raise ValueError(f"box_qp: warm.{name} does not match this problem ({Bt} x {n} {g.dtype} on {g.device})")
                out[name] = t.detach().reshape(Bt, n).clone()
        res = sol.box_qp(Gb, Cb, g, cc, lo, hi, rho=rho, exit_tol=exit_tol, max_iters=max_iters, admm_rho=admm_rho,
                         sigma=sigma, alpha=alpha, eps_abs=eps_abs, eps_rel=eps_rel, max_admm_iters=max_admm_iters,
                         check_every=check_every, warm=warm is not None, **out)
    N, sk = sol.N, sol.sizes["sk"]
    shp = lambda t, n: t.view(Bt, n) if batched else t.view(n)
    first = (lambda t: t) if batched else (lambda t: t[0])
    return BoxQPResult(shp(res.x, N), shp(res.z, N), shp(res.y, N), shp(res.lam, sk), first(res.iters), first(res.status),
                       first(res.res_prim), first(res.res_dual))


STATUS = {_lib.QP_CONVERGED: "CONVERGED", _lib.QP_MAX_ITERS: "MAX_ITERS", _lib.QP_NONFINITE: "NONFINITE",
          _lib.QP_BAD_BOUNDS: "BAD_BOUNDS"}
