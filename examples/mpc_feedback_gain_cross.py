"""The feedback gain of an MPC law whose stage cost couples states and controls, by forward-mode sensitivities (DESIGN.md
section 3.17).  The plant and the output cost 1/2 |Cy x + Dy u|^2 are those of examples/lqr_cross_term.py: Q = Cy^T Cy, R = Dy^T Dy
and the cross term M = Cy^T Dy.  The first control u_0 is a function of the measured state x_0, which enters through block 0 of
c, so the gain du_0 / dx_0 [C, S] is the tangent of the solution along the S unit directions of that block:
kkt_solve_tangents(..., M=M), one call and one re-solve for the S right-hand sides.  For this unconstrained problem the gain is
known in closed form: -K_0 of the Riccati recursion with the cross term.  The gain of the problem without M is printed beside it:
dropping the cross term is another control law.            python examples/mpc_feedback_gain_cross.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = int(sys.argv[1]) if len(sys.argv) > 1 else 30
S, C, RHO = 4, 2, 1e-8
dt = 0.1
# two double integrators, weakly coupled; the output y = Cy x + Dy u of examples/lqr_cross_term.py
A = np.eye(S) + dt * np.array([[0, 1, 0, 0], [0, 0, 0.2, 0], [0, 0, 0, 1], [-0.2, 0, 0, 0.0]])
B = np.array([[0.5 * dt * dt, 0], [dt, 0], [0, 0.5 * dt * dt], [0, dt]])
Cy = np.vstack([np.diag([3.0, 1.0, 3.0, 1.0]), np.zeros((C, S))])
Dy = np.vstack([np.array([[0, 0], [0.3, 0], [0, 0], [0, 0.3]]), 0.5 * np.eye(C)])
Q, R, M = Cy.T @ Cy, Dy.T @ Dy, Cy.T @ Dy
QN = 10.0 * Q
x0 = np.array([1.0, 0.0, -0.5, 0.2])


def riccati_gain(Mx):
    """K_0 of the backward sweep with the cross term Mx (rho on every diagonal, as the solver adds it): u_0 = -K_0 x_0."""
    P = QN + RHO * np.eye(S)
    for _ in range(K - 1):
        Hux = Mx.T + B.T @ P @ A
        Kk = np.linalg.solve(R + RHO * np.eye(C) + B.T @ P @ B, Hux)
        P = Q + RHO * np.eye(S) + A.T @ P @ A - Hux.T @ Kk
    return Kk


def main():
    import torch
    import gato_python_amd
    t = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
    rep = lambda a: np.tile(a, (K - 1, 1, 1))
    Qs = np.tile(Q, (K, 1, 1))
    Qs[-1] = QN
    c = np.zeros((K, S))
    c[0] = x0                                                              # row block 0 of C dz = c pins x_0; C holds -A, -B
    blocks = [t(v) for v in (Qs, rep(R), rep(-A), rep(-B), np.zeros((K, S)), np.zeros((K - 1, C)), c)]
    c_dot = np.zeros((S, K, S))
    c_dot[np.arange(S), 0, np.arange(S)] = 1.0                             # the direction dx_0 = e_j
    opts = dict(rho=RHO, exit_tol=1e-20, max_iters=1000)
    _, _, _, dz_dot = gato_python_amd.kkt_solve_tangents(*blocks, dict(c=t(c_dot)), M=t(rep(M)), **opts)
    gain = dz_dot[:, S:S + C].T.cpu().numpy()                              # u_0 follows x_0 in the dz layout: [C, S]
    _, _, _, dz_dot0 = gato_python_amd.kkt_solve_tangents(*blocks, dict(c=t(c_dot)), **opts)
    gain0 = dz_dot0[:, S:S + C].T.cpu().numpy()
    want = -riccati_gain(M)
    diff = np.abs(gain - want).max()
    print("K = %d knots, du_0/dx_0 from %d tangents in one call:\n%s" % (K, S, np.array2string(gain, precision=8)))
    print("-K_0 of the Riccati recursion with the cross term:\n%s" % np.array2string(want, precision=8))
    print("the gain without M:\n%s" % np.array2string(gain0, precision=8))
    print("largest difference to -K_0: %.3g   (dropping M moves the gain by %.3g)" % (diff, np.abs(gain0 - want).max()))
    assert diff < 1e-8 * np.abs(want).max(), diff
    assert np.abs(gain0 + riccati_gain(np.zeros((S, C)))).max() < 1e-8 * np.abs(want).max()


if __name__ == "__main__":
    main()
