"""A double integrator driven to rest with a force limit |u| <= 0.5 and a soft velocity limit |v| <= 0.57, the problem of
examples/box_mpc_soft.py, with a cap on the penalty force.  The quadratic penalty of weight 100 pulls a
violating velocity back with a force w (v - 0.57) that grows with the violation (3.9 here); a weight of 1e6 without a cap is
where the undamped iteration cycles and ends without an answer.  With the cap m the penalty is the Huber function: the force is
clamp(w (v - 0.57), -m, m), a velocity whose force would pass the cap is saturated (act = +-2, y = +-m), and however large
the weight no term pulls harder than m.  With m below the force the limit would need, the limit gives way by a bounded amount
and the call converges at weight 1e6.  The script prints the three outcomes.          python examples/box_mpc_huber.py [K]
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

n = S + C
vix = [k * n + 1 for k in range(K)]


def report(name, res):
    if int(res.status) != 0:
        print("%-28s %s after %d reduced solves (no answer is written)" % (name, STATUS.get(int(res.status), "?"), int(res.iters)))
        return
    x, y, act = res.x.cpu().numpy(), res.y.cpu().numpy(), res.act.cpu().numpy()
    frc = np.array([x[k * n + S] for k in range(K - 1)])
    print("%-28s CONVERGED after %2d reduced solves, %d velocities quadratic-active, %d saturated, limit exceeded by at most "
          "%.2e, largest penalty force |y| %.3f, |u| <= %.3f" % (name, int(res.iters), int((np.abs(act[vix]) == 1).sum()),
          int((np.abs(act[vix]) == 2).sum()), float(np.maximum(np.abs(x[vix]) - V_MAX, 0.0).max()), float(np.abs(y[vix]).max()),
          float(np.abs(frc).max())))
    assert np.abs(frc).max() <= U_MAX                                  # the hard bound holds exactly


soft = lambda W: t(np.tile([0.0, W], (K, 1)))                          # weight W on every velocity bound
box = (-x_hi, x_hi, -U_MAX, U_MAX)
quad = gato_python_amd.box_qp(*blocks, *box, x_soft=soft(100.0), **opts)
report("weight 100, no cap:", quad)
assert int(quad.status) == 0
stiff = gato_python_amd.box_qp(*blocks, *box, x_soft=soft(1e6), **opts)
report("weight 1e6, no cap:", stiff)
CAP = 0.3
huber = gato_python_amd.box_qp(*blocks, *box, x_soft=soft(1e6), x_soft_max=CAP, **opts)
report("weight 1e6, cap %.1f:" % CAP, huber)
assert int(huber.status) == 0
assert np.abs(huber.y.cpu().numpy()[vix]).max() <= CAP                 # no velocity is pulled harder than the cap
