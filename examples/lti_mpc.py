"""Receding-horizon control of a linear plant: the KKT matrices of a linear plant with a quadratic cost are the same at
every control step, only c_0 = x_0 - xs (and g, when the goal moves) change.  The system is assembled ONCE; every step
then writes the new right-hand side and calls Solver.solve_rhs (no re-assembly).  The same loop also runs a full solve per
step, and the script prints the largest relative difference between the two.      python examples/lti_mpc.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
from gato_python_amd import kkt                        # noqa: E402
from gato_python_amd.solver import Solver             # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 30
STEPS, dt = 20, 0.1
# two double integrators (planar point mass): S = 4 (position, velocity per axis), C = 2 (force per axis)
a = np.array([[1.0, dt], [0.0, 1.0]])
b = np.array([[0.5 * dt * dt], [dt]])
plant = kkt.LinearPlant(np.kron(np.eye(2), a), np.kron(np.eye(2), b))
S, C = plant.S, plant.C
Q, R, QF = np.diag([10.0, 1.0, 10.0, 1.0]), 0.1 * np.eye(C), np.diag([100.0, 10.0, 100.0, 10.0])
tol, mi = 1e-12, 500


def problem(x0, goal):
    """KKT system linearised around the zero trajectory: G and C never change, c_0 = 0 - x0, g = Q (0 - goal)."""
    return kkt.get_kkt(plant, np.zeros((K, S)), np.zeros((K - 1, C)), x0, goal, dt, Q, R, QF, rho=1e-6)


x = np.array([1.0, 0.0, -0.5, 0.2])
goal = np.zeros(S)
p = problem(x, goal)
re, full = Solver(S, C, K, np.float64), Solver(S, C, K, np.float64)
lam, dz = re.new(S * K), re.new(re.N)
re.linsys(*re.upload_system(p), tol, mi, p.rho, lam, dz)                 # the one assembly
g, c = re.to_device(p.g), re.to_device(p.c)
lam_f, dz_f = full.new(S * K), full.new(full.N)
worst = 0.0
for step in range(STEPS):
    if step == 10:
        goal = np.array([0.5, 0.0, 0.5, 0.0])                           # the goal moves: g changes too
    q = problem(x, goal)
    assert np.array_equal(q.G_val, p.G_val) and np.array_equal(q.C_val, p.C_val)
    g.copy_(torch.from_numpy(q.g)); c.copy_(torch.from_numpy(q.c))
    lam_r, dz_r, it = re.solve_rhs(g, c, tol, mi)
    full.linsys(*full.upload_system(q), tol, mi, q.rho, lam_f, dz_f)
    torch.cuda.synchronize()
    dr, df = dz_r.cpu().numpy(), dz_f.cpu().numpy()
    lr, lf = lam_r.cpu().numpy(), lam_f.cpu().numpy()
    diff = max(np.abs(dr - df).max() / np.abs(df).max(), np.abs(lr - lf).max() / np.abs(lf).max())
    worst = max(worst, diff)
    u = -dr[S:S + C]                                                    # the KKT solution is the negative Newton step
    x = plant.step(x, u, dt)
    print("step %2d  iters %3d  |x - goal| %.4f  difference %.2e" % (step, int(it.cpu()[0]), np.linalg.norm(x - goal), diff))
print("largest difference %.3e" % worst)
