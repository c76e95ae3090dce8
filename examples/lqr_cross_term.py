"""A finite-horizon LQR whose stage cost couples states and controls.  The plant x+ = A x + B u is
driven from x_0 with the output cost 1/2 |C x + D u|^2 per stage - a Gauss-Newton cost on y = C x + D u - so Q = C^T C,
R = D^T D and the cross term M = C^T D, which block-diagonal inputs cannot express.  kkt_solve(M=...) solves the whole horizon
at once; the same problem by the Riccati recursion with a cross term (numpy, backward sweep for the gains, forward roll-out)
gives the trajectory to compare with.  Prints the largest difference.            python examples/lqr_cross_term.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = int(sys.argv[1]) if len(sys.argv) > 1 else 30
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


def riccati():
    """The trajectory (x_k, u_k) of min sum 1/2 [x; u]^T [[Q, M], [M^T, R]] [x; u] + 1/2 x_N^T QN x_N (rho on every diagonal, as the
    solver adds it): P_N = QN, K_k = (R + B^T P B)^-1 (M^T + B^T P A), P_k = Q + A^T P A - (M^T + B^T P A)^T K_k, u = -K x."""
    P = QN + RHO * np.eye(S)
    gains = []
    for _ in range(K - 1):
        Huu = R + RHO * np.eye(C) + B.T @ P @ B
        Hux = M.T + B.T @ P @ A
        Kk = np.linalg.solve(Huu, Hux)
        P = Q + RHO * np.eye(S) + A.T @ P @ A - Hux.T @ Kk
        gains.append(Kk)
    xs, us, x = [x0], [], x0
    for Kk in reversed(gains):
        u = -Kk @ x
        x = A @ x + B @ u
        us.append(u)
        xs.append(x)
    return np.array(xs), np.array(us)


def blocks():
    """The math-shaped blocks of kkt_solve: C holds the raw values -A, -B; row block 0 of C dz = c pins x_0."""
    Qs = np.tile(Q, (K, 1, 1))
    Qs[-1] = QN
    c = np.zeros((K, S))
    c[0] = x0
    rep = lambda a: np.tile(a, (K - 1, 1, 1))
    return Qs, rep(R), rep(-A), rep(-B), np.zeros((K, S)), np.zeros((K - 1, C)), c, rep(M)


def main():
    import torch
    import gato_python_amd
    t = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
    *b, Ms = blocks()
    lam, dz = gato_python_amd.kkt_solve(*map(t, b), M=t(Ms), rho=RHO, exit_tol=1e-20, max_iters=1000)
    dz = dz.cpu().numpy()
    n = S + C
    xs = np.array([dz[k * n:k * n + S] for k in range(K)])
    us = np.array([dz[k * n + S:(k + 1) * n] for k in range(K - 1)])
    xr, ur = riccati()
    diff = max(np.abs(xs - xr).max(), np.abs(us - ur).max())
    # without the cross term the problem is another one: its controls differ visibly
    _, dz0 = gato_python_amd.kkt_solve(*map(t, b), rho=RHO, exit_tol=1e-20, max_iters=1000)
    u0 = np.array([dz0.cpu().numpy()[k * n + S:(k + 1) * n] for k in range(K - 1)])
    print("K = %d knots, u_0 = %s (Riccati %s)" % (K, np.round(us[0], 6), np.round(ur[0], 6)))
    print("largest difference to the Riccati recursion: %.3g   (dropping M moves the controls by %.3g)" % (diff, np.abs(u0 - ur).max()))
    assert diff < 1e-8 * max(np.abs(xr).max(), np.abs(ur).max()), diff


if __name__ == "__main__":
    main()
