"""A double integrator driven to rest with a force limit |u| <= 0.5 and a velocity limit |v| <= 0.57, the problem of DESIGN.md
sections 3.9 and 3.10.  With both limits hard the active-set iteration (box_qp(method="pdas")) eliminates so many velocities
that its second reduced system is singular, and it ends without an answer.  With the velocity limit soft - x_soft: a
quadratic penalty of weight W on the violation, the force limit still hard - the same call converges: a violating velocity
stays in the reduced system and only gains W on its diagonal.  The script prints both outcomes, the largest velocity
violation per weight, and the penalty forces the result carries in y.                 python examples/box_mpc_soft.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
import gato_python_amd                                 # noqa: E402
from gato_python_amd.qp import STATUS                  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dt, U_MAX, V_MAX = 0.1, 0.5, 0.57
S, C = 2, 1
a = np.array([[1.0, dt], [0.0, 1.0]])
b = np.array([[0.5 * dt * dt], [dt]])
t = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
Q = np.tile(np.diag([10.0, 1.0]), (K, 1, 1))
Q[-1] = np.diag([100.0, 10.0])
c = np.zeros((K, S))
c[0] = -np.array([1.0, 0.0])                                           # x_0 = (1, 0); C holds -A, -B
blocks = [t(Q), t(np.tile(0.1 * np.eye(C), (K - 1, 1, 1))), t(np.tile(-a, (K - 1, 1, 1))), t(np.tile(-b, (K - 1, 1, 1))),
          t(np.zeros((K, S))), t(np.zeros((K - 1, C))), t(c)]
x_hi = t(np.tile([np.inf, V_MAX], (K, 1)))                             # the position is free, the velocity limited
opts = dict(rho=1e-6, exit_tol=1e-14, max_iters=500, method="pdas")

hard = gato_python_amd.box_qp(*blocks, -x_hi, x_hi, -U_MAX, U_MAX, **opts)
print("hard velocity limit:  %s after %d reduced solves (no answer is written)" % (STATUS.get(int(hard.status), "?"), int(hard.iters)))
assert int(hard.status) != 0

n = S + C
for W in (1.0, 10.0, 100.0):
    x_soft = t(np.tile([0.0, W], (K, 1)))                              # weight W on every velocity bound
    res = gato_python_amd.box_qp(*blocks, -x_hi, x_hi, -U_MAX, U_MAX, x_soft=x_soft, **opts)
    assert int(res.status) == 0, res
    x = res.x.cpu().numpy()
    vel = np.array([x[k * n + 1] for k in range(K)])
    frc = np.array([x[k * n + S] for k in range(K - 1)])
    soft_active = (res.act.cpu().numpy() != 0)[[k * n + 1 for k in range(K)]]
    print("soft, weight %5.0f:   CONVERGED after %2d reduced solves, %2d velocities beyond the limit by at most %.2e, "
          "largest penalty force |y| %.3f, |u| <= %.3f" % (W, int(res.iters), int(soft_active.sum()),
          float(np.maximum(np.abs(vel) - V_MAX, 0.0).max()), float(np.abs(res.y.cpu().numpy()[[k * n + 1 for k in range(K)]]).max()),
          float(np.abs(frc).max())))
    assert np.abs(frc).max() <= U_MAX                                  # the hard bound holds exactly
