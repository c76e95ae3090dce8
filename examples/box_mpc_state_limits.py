"""A double integrator driven to rest with a HARD force limit |u| <= 0.5 and a HARD velocity limit |v| <= 0.57 (DESIGN.md section
3.14).  Hard state bounds are where the other methods struggle: ADMM has one fixed penalty and takes thousands of x-steps, the
hard active-set iteration eliminates the active states and meets a singular reduced system, and soft bounds answer another
question.  method="alm" runs the method of multipliers over the line-search iteration: a few dozen reduced solves in a handful
of outer steps, and the bound holds to the solver's tolerance.  The script prints it beside ADMM (polished).
                                                                               python examples/box_mpc_state_limits.py [K]
"""
import os
import sys
import time

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
box = (-x_hi, x_hi, -U_MAX, U_MAX)
opts = dict(rho=1e-6, exit_tol=1e-14, max_iters=500)

n = S + C
vix = [k * n + 1 for k in range(1, K)]                                  # the velocities after x_0
uix = [k * n + S for k in range(K - 1)]


def timed(**kw):
    gato_python_amd.box_qp(*blocks, *box, **opts, **kw)                # the first call sizes the work areas
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = gato_python_amd.box_qp(*blocks, *box, **opts, **kw)
    torch.cuda.synchronize()
    return res, 1e3 * (time.perf_counter() - t0)


def report(name, res, ms, what):
    x = res.x.cpu().numpy()
    print("%-6s %-10s %5d %-14s %7.2f ms   velocity limit exceeded by %.1e, force limit by %.1e, objective %.9f" % (
        name, STATUS.get(int(res.status), "?"), int(res.iters), what, ms, float(np.maximum(np.abs(x[vix]) - V_MAX, 0.0).max()),
        float(np.maximum(np.abs(x[uix]) - U_MAX, 0.0).max()),
        float(0.5 * (x[[k * n + i for k in range(K) for i in range(S)]].reshape(K, S) ** 2 * np.diagonal(Q, axis1=1, axis2=2)).sum()
              + 0.05 * (x[uix] ** 2).sum())))


alm, alm_ms = timed(method="alm")
report("alm:", alm, alm_ms, "reduced solves")
print("       %d outer steps, last weight %g, %d velocity and %d force bounds active" % (
    int(alm.outer), float(alm.weight), int((alm.y.cpu().numpy()[vix] != 0).sum()), int((alm.y.cpu().numpy()[uix] != 0).sum())))
admm, admm_ms = timed(polish=True)
report("admm:", admm, admm_ms, "x-steps")
assert int(alm.status) == 0 and int(admm.status) == 0
assert float((alm.x - admm.x).abs().max()) < 1e-4                       # the same point
