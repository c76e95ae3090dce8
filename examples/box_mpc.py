"""Receding-horizon control with a force limit |u| <= U_MAX: the two double integrators of examples/lti_mpc.py, each step one
box-constrained QP (gato_python_amd.box_qp: ADMM over the device re-solve) warm-started from the previous step's (z, y,
lambda).  Per step the script prints the ADMM iterations, the largest bound violation of the applied force, and the same for
the unconstrained solve (gato_python_amd.kkt_solve), which does violate the limit.      python examples/box_mpc.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
import gato_python_amd                                 # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 30
STEPS, dt, U_MAX = 20, 0.1, 2.0
# two double integrators (planar point mass): S = 4 (position, velocity per axis), C = 2 (force per axis)
a = np.kron(np.eye(2), np.array([[1.0, dt], [0.0, 1.0]]))
b = np.kron(np.eye(2), np.array([[0.5 * dt * dt], [dt]]))
S, C = 4, 2
Qs, Rs, QF = np.diag([10.0, 1.0, 10.0, 1.0]), 0.1 * np.eye(C), np.diag([100.0, 10.0, 100.0, 10.0])
t = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
# the KKT blocks of the trajectory step around zero (C holds -A, -B); they never change, only q and c_0 do
Q = t(np.stack([Qs] * (K - 1) + [QF]))
R, A, B = t(np.stack([Rs] * (K - 1))), t(np.stack([-a] * (K - 1))), t(np.stack([-b] * (K - 1)))
r = t(np.zeros((K - 1, C)))
opts = dict(rho=1e-6, exit_tol=1e-14, max_iters=500)


def rhs(x0, goal):
    """q_k = -Q_k goal, c_0 = -x0: the solution dz is the negated trajectory, so the force to apply is -dz_u,0"""
    q = -np.einsum("kij,j->ki", np.stack([Qs] * (K - 1) + [QF]), goal)
    c = np.zeros((K, S))
    c[0] = -x0
    return t(q), t(c)


x = np.array([1.0, 0.0, -0.5, 0.2])
goal = np.zeros(S)
prev = None
worst_box, worst_free = 0.0, 0.0
for step in range(STEPS):
    if step == 10:
        goal = np.array([3.0, 0.0, 3.0, 0.0])                          # a far goal: the limit becomes active
    q, c = rhs(x, goal)
    res = gato_python_amd.box_qp(Q, R, A, B, q, r, c, -np.inf, np.inf, -U_MAX, U_MAX, warm=prev, **opts)
    _, dz_free = gato_python_amd.kkt_solve(Q, R, A, B, q, r, c, **opts)
    assert int(res.status) == 0, res
    prev = res
    u = -res.z[S:S + C].cpu().numpy()                                 # z: the iterate inside the box
    u_free = -dz_free[S:S + C].detach().cpu().numpy()
    v_box = float(np.maximum(np.abs(u) - U_MAX, 0.0).max())
    v_free = float(np.maximum(np.abs(u_free) - U_MAX, 0.0).max())
    worst_box, worst_free = max(worst_box, v_box), max(worst_free, v_free)
    x = a @ x + b @ u
    print("step %2d  ADMM iters %4d  |u| %.3f  violation %.2e  unconstrained |u| %.3f  violation %.2e  |x - goal| %.4f"
          % (step, int(res.iters), np.abs(u).max(), v_box, np.abs(u_free).max(), v_free, np.linalg.norm(x - goal)))
print("largest violation: box QP %.3e, unconstrained %.3e" % (worst_box, worst_free))
