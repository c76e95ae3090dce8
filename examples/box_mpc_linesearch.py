"""A double integrator driven to rest with a soft force limit |u| <= 0.5 and a soft velocity limit |v| <= 0.57, both with the
stiff weight 1e6 and the cap 1 on the penalty force (DESIGN.md sections 3.11, 3.12): a cap "between the regimes", where the
undamped active-set iteration cycles and ends MAX_ITERS without an answer.  With every bound soft the problem is the
minimisation of a strongly convex piecewise-quadratic function on C x = c, each reduced solve is a Newton step of it, and
line_search=True takes the exact minimiser along that step instead of the whole step: the iteration then converges, in more
solves than a problem the undamped iteration can do would need.  The script prints both outcomes and the step lengths.
                                                                               python examples/box_mpc_linesearch.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
import gato_python_amd                                 # noqa: E402
from gato_python_amd.qp import STATUS                  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dt, U_MAX, V_MAX, WEIGHT, CAP = 0.1, 0.5, 0.57, 1e6, 1.0
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
opts = dict(rho=1e-6, exit_tol=1e-14, max_iters=500, method="pdas", x_soft=WEIGHT, u_soft=WEIGHT, x_soft_max=CAP, u_soft_max=CAP)

n = S + C
vix = [k * n + 1 for k in range(K)]
uix = [k * n + S for k in range(K - 1)]


def report(name, res):
    if int(res.status) != 0:
        print("%-12s %s after %d reduced solves (no answer is written)" % (name, STATUS.get(int(res.status), "?"), int(res.iters)))
        return
    x, y, act = res.x.cpu().numpy(), res.y.cpu().numpy(), res.act.cpu().numpy()
    print("%-12s CONVERGED after %2d reduced solves, %d bounds saturated, %d quadratic-active, velocity limit exceeded by at most "
          "%.2e, force limit by %.2e, largest penalty force |y| %.3f" % (
              name, int(res.iters), int((np.abs(act) == 2).sum()), int((np.abs(act) == 1).sum()),
              float(np.maximum(np.abs(x[vix]) - V_MAX, 0.0).max()), float(np.maximum(np.abs(x[uix]) - U_MAX, 0.0).max()),
              float(np.abs(y).max())))


box = (-x_hi, x_hi, -U_MAX, U_MAX)
undamped = gato_python_amd.box_qp(*blocks, *box, max_pdas_iters=30, **opts)
report("undamped:", undamped)
damped = gato_python_amd.box_qp(*blocks, *box, max_pdas_iters=60, line_search=True, **opts)
report("line search:", damped)
print("step lengths:", " ".join("%.3f" % v for v in damped.alpha[:int(damped.iters)].tolist()))
assert int(undamped.status) == 1 and int(damped.status) == 0
assert np.abs(damped.y.cpu().numpy()).max() <= CAP                      # no bound pulls harder than the cap
