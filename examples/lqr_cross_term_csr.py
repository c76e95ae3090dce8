"""The LQR of examples/lqr_cross_term.py from CSR arrays.  The same plant and output cost
1/2 |Cy x + Dy u|^2 per stage, so Q = Cy^T Cy, R = Dy^T Dy and the cross term M = Cy^T Dy; kkt.get_kkt(M=...) linearises the
problem into the CSR arrays gpu_library.linsys_solve takes - G then holds M and M^T between the Q and R parts - and
kkt_solve_csr(cross=True) solves it.  The numpy Riccati recursion with a cross term gives the trajectory to compare with, and one
line shows what cross=False returns for the very same arrays: the solution of the problem without M, with no error.
    python examples/lqr_cross_term_csr.py [K]
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


def controls(dz):
    n = S + C
    return np.array([dz[k * n + S:(k + 1) * n] for k in range(K - 1)])


def main():
    import torch
    from gato_python_amd import kkt, kkt_solve_csr
    # linearised around the zero trajectory with the target at the origin and the start pinned by c_0 = x_0 - xs: g = 0, c_0 = -x0,
    # so the unknowns are the negated trajectory (the sign convention of the reference's KKT producer)
    s = kkt.get_kkt(kkt.LinearPlant(A, B), np.zeros((K, S)), np.zeros((K - 1, C)), x0, np.zeros(S), dt, Q, R, QN, rho=RHO, M=M)
    n = S + C
    rows = np.repeat(np.arange(s.N), np.diff(s.G_row))
    cross = int(((rows % n < S) != (s.G_col % n < S)).sum())
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    args = (i32(s.G_row), i32(s.G_col), f64(s.G_val), i32(s.C_row), i32(s.C_col), f64(s.C_val), f64(s.g), f64(s.c))
    kw = dict(rho=RHO, exit_tol=1e-20, max_iters=1000)
    _, dz = kkt_solve_csr(*args, cross=True, **kw)
    dz = -dz.cpu().numpy()
    xs, us = np.array([dz[k * n:k * n + S] for k in range(K)]), controls(dz)
    xr, ur = riccati()
    diff = max(np.abs(xs - xr).max(), np.abs(us - ur).max())
    _, dz0 = kkt_solve_csr(*args, cross=False, **kw)          # the same arrays through the plain CSR path: the cross entries are dropped
    print("K = %d knots, G holds %d entries of which %d are cross entries; u_0 = %s (Riccati %s)"
          % (K, len(s.G_col), cross, np.round(us[0], 6), np.round(ur[0], 6)))
    print("cross=True: largest difference to the Riccati recursion %.3g" % diff)
    print("cross=False on the same arrays: controls off by %.3g, and no error" % np.abs(controls(-dz0.cpu().numpy()) - ur).max())
    assert diff < 1e-8 * max(np.abs(xr).max(), np.abs(ur).max()), diff


if __name__ == "__main__":
    main()
