"""Constrained MPC with an output cost.  The LTI plant of lqr_cross_term.py, x+ = A x + B u, is driven
from x_0 with the stage cost 1/2 |Cy x + Dy u|^2 - so Q = Cy^T Cy, R = Dy^T Dy and the cross term M = Cy^T Dy - under the
actuator limits |u| <= u_max.  box_qp(M=...) solves the horizon by ADMM; the box stays a box on u although the x-step runs in the
variables of the change of variables u = v - W x.  Prints the KKT residuals of the returned point for the QP with M, formed in
torch from the blocks, and how far the controls move when M is dropped.            python examples/box_mpc_cross.py [K] [u_max]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = int(sys.argv[1]) if len(sys.argv) > 1 else 30
U_MAX = float(sys.argv[2]) if len(sys.argv) > 2 else 0.8
S, C, RHO = 4, 2, 1e-8
dt = 0.1
# two double integrators, weakly coupled
A = np.eye(S) + dt * np.array([[0, 1, 0, 0], [0, 0, 0.2, 0], [0, 0, 0, 1], [-0.2, 0, 0, 0.0]])
B = np.array([[0.5 * dt * dt, 0], [dt, 0], [0, 0.5 * dt * dt], [0, dt]])
# the output y = Cy x + Dy u: positions, velocities that see the controls, and the controls themselves
Cy = np.vstack([np.diag([3.0, 1.0, 3.0, 1.0]), np.zeros((C, S))])
Dy = np.vstack([np.array([[0, 0], [0.3, 0], [0, 0], [0, 0.3]]), 0.5 * np.eye(C)])
Q, R, M = Cy.T @ Cy, Dy.T @ Dy, Cy.T @ Dy
QN = 10.0 * Q
x0 = np.array([1.0, 0.0, -0.5, 0.2])


def blocks():
    """The math-shaped blocks of box_qp: C holds the raw values -A, -B; row block 0 of C x = c pins x_0."""
    Qs = np.tile(Q, (K, 1, 1))
    Qs[-1] = QN
    c = np.zeros((K, S))
    c[0] = x0
    rep = lambda a: np.tile(a, (K - 1, 1, 1))
    return Qs, rep(R), rep(-A), rep(-B), np.zeros((K, S)), np.zeros((K - 1, C)), c, rep(M)


def split(v, per, last):
    """A flat [K per - (per - last)] vector of the dz layout -> (x [K, S], u [K-1, C])."""
    import torch
    body = v[:(K - 1) * per].view(K - 1, per)
    return torch.cat([body[:, :S], v[(K - 1) * per:].view(1, last)]), body[:, S:]


def kkt_residuals(b, Ms, res, u_max):
    """Stationarity H x - g + C^T lambda + y, equality C x - c, the violation of |u| <= u_max and the complementarity of y, in
    the infinity norm; H = G + rho I with M_k, M_k^T between Q_k and R_k."""
    import torch
    Qs, Rs, As, Bs, q, r, c = b
    x, u = split(res.x, S + C, S)
    yx, yu = split(res.y, S + C, S)
    lam = res.lam.view(K, S)
    mv = lambda mat, v: torch.einsum("kij,kj->ki", mat, v)
    hx = mv(Qs, x) + RHO * x
    hx[:-1] += mv(Ms, u)
    hu = mv(Ms.transpose(1, 2), x[:-1]) + mv(Rs, u) + RHO * u
    cx = lam.clone()
    cx[:-1] += mv(As.transpose(1, 2), lam[1:])
    cu = mv(Bs.transpose(1, 2), lam[1:])
    stat = max((hx - q + cx + yx).abs().max(), (hu - r + cu + yu).abs().max())
    eq = x - c
    eq[1:] += mv(As, x[:-1]) + mv(Bs, u)
    bound = (u.abs() - u_max).clamp(min=0).max()
    comp = torch.maximum(yu.clamp(min=0) * (u_max - u).abs(), (-yu).clamp(min=0) * (u + u_max).abs()).max()
    return dict(stat=float(stat), eq=float(eq.abs().max()), bound=float(bound), comp=float(max(comp, yx.abs().max())))


def main():
    import torch
    import gato_python_amd
    from gato_python_amd import _lib
    t = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
    *b, Ms = map(t, blocks())
    inf = float("inf")
    kw = dict(rho=RHO, exit_tol=1e-20, max_iters=1000, eps_abs=1e-8, eps_rel=1e-8, admm_rho=1.0)
    res = gato_python_amd.box_qp(*b, -inf, inf, -U_MAX, U_MAX, M=Ms, **kw)
    assert int(res.status) == _lib.QP_CONVERGED, res
    kk = kkt_residuals(b, Ms, res, U_MAX)
    _, u = split(res.x, S + C, S)
    at = int((split(res.z, S + C, S)[1].abs() >= U_MAX).sum())               # z is the iterate clipped to the box
    print("K = %d knots, |u| <= %g: %d ADMM iterations, %d of %d controls at a limit, u_0 = %s"
          % (K, U_MAX, int(res.iters), at, u.numel(), np.round(u[0].cpu().numpy(), 6)))
    print("KKT residuals of the QP with M: stationarity %.2e, dynamics %.2e, bounds %.2e, complementarity %.2e"
          % (kk["stat"], kk["eq"], kk["bound"], kk["comp"]))
    # without the cross term the problem is another one: its controls differ visibly
    res0 = gato_python_amd.box_qp(*b, -inf, inf, -U_MAX, U_MAX, **kw)
    _, u0 = split(res0.x, S + C, S)
    print("dropping M moves the controls by %.3g (and the point no longer solves the QP: stationarity %.2e)"
          % (float((u0 - u).abs().max()), kkt_residuals(b, Ms, res0, U_MAX)["stat"]))
    assert at > 0 and max(kk.values()) < 1e-6, kk


if __name__ == "__main__":
    main()
