"""Receding-horizon control with a force limit |u| <= U_MAX, the problem of examples/box_mpc.py, by the primal-dual active-set
iteration (gato_python_amd.box_qp(method="pdas")): bounds on the controls alone, so every reduced
system is regular, there is no penalty to choose, and each step starts from the previous step's active set.  Per step the
script prints the reduced solves it took beside the ADMM x-steps of the same QP (warm-started as box_mpc.py does), the
difference of the two forces, and the largest bound violation of the applied force.      python examples/box_mpc_pdas.py [K]
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
prev, prev_admm = None, None
worst_box, worst_gap = 0.0, 0.0
for step in range(STEPS):
    if step == 10:
        goal = np.array([3.0, 0.0, 3.0, 0.0])                          # a far goal: the limit becomes active
    q, c = rhs(x, goal)
    res = gato_python_amd.box_qp(Q, R, A, B, q, r, c, -np.inf, np.inf, -U_MAX, U_MAX, method="pdas", warm=prev, **opts)
    adm = gato_python_amd.box_qp(Q, R, A, B, q, r, c, -np.inf, np.inf, -U_MAX, U_MAX, warm=prev_admm, **opts)
    assert int(res.status) == 0 and int(adm.status) == 0, (res, adm)
    prev, prev_admm = res, adm
    u = -res.x[S:S + C].cpu().numpy()                                 # x of a converged active-set solve lies in the box
    gap = float(np.abs(u + adm.z[S:S + C].cpu().numpy()).max())
    v_box = float(np.maximum(np.abs(u) - U_MAX, 0.0).max())
    worst_box, worst_gap = max(worst_box, v_box), max(worst_gap, gap)
    x = a @ x + b @ u
    print("step %2d  reduced solves %2d  active %2d  ADMM iters %4d  |u| %.3f  violation %.2e  |u - u_admm| %.2e  |x - goal| %.4f"
          % (step, int(res.iters), int((res.act != 0).sum()), int(adm.iters), np.abs(u).max(), v_box, gap, np.linalg.norm(x - goal)))
print("largest violation %.3e, largest difference to ADMM %.3e" % (worst_box, worst_gap))
