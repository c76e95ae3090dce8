"""The feedback gain of a constrained MPC law by forward-mode sensitivities.  A double integrator is
driven to rest under a force limit |u| <= 0.5; the first control u_0 is a function of the measured state x_0, and the gain
du_0 / dx_0 [C, S] is what a tracking loop around the MPC law needs between two solves.  x_0 enters through block 0 of c, so the
gain is the tangent of the solution along the S unit directions of that block: one call, one re-solve for the S right-hand
sides.  The same matrix by reverse mode takes one backward pass per control, C of them.  Where u_0 sits on its limit the law is
locally constant: that row of the gain is exactly zero.            python examples/mpc_feedback_gain.py [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
import gato_python_amd                                 # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dt, U_MAX = 0.1, 0.5
S, C = 2, 1
a = np.array([[1.0, dt], [0.0, 1.0]])
b = np.array([[0.5 * dt * dt], [dt]])
t = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")
Q = np.tile(np.diag([10.0, 1.0]), (K, 1, 1))
Q[-1] = np.diag([100.0, 10.0])
opts = dict(rho=1e-6, exit_tol=1e-14, max_iters=500, method="pdas")
inf = float("inf")


def problem(x0):
    c = np.zeros((K, S))
    c[0] = -np.asarray(x0)                                             # row block 0 of C x = c pins x_0; C holds -A, -B
    return [t(Q), t(np.tile(0.1 * np.eye(C), (K - 1, 1, 1))), t(np.tile(-a, (K - 1, 1, 1))), t(np.tile(-b, (K - 1, 1, 1))),
            t(np.zeros((K, S))), t(np.zeros((K - 1, C))), t(c)]


def gains(x0):
    blocks = problem(x0)
    box = (-inf, inf, -U_MAX, U_MAX)
    # forward mode: c_0 = -x_0, so the direction dx_0 = e_j is the tangent -e_j of c's block 0
    c_dot = np.zeros((S, K, S))
    c_dot[np.arange(S), 0, np.arange(S)] = -1.0
    x, lam, info, x_dot, lam_dot = gato_python_amd.box_qp_layer_tangents(*blocks, *box, dict(c=t(c_dot)), **opts)
    assert int(info.polished) == 0
    fwd = x_dot[:, S:S + C].T.cpu().numpy()                            # u_0 follows x_0 in the dz layout: [C, S]
    # reverse mode: one backward pass per control
    blocks[6].requires_grad_()
    xr, _, _ = gato_python_amd.box_qp_layer(*blocks, *box, **opts)
    rev = np.stack([-torch.autograd.grad(xr[S + i], blocks[6], retain_graph=True)[0][0].cpu().numpy() for i in range(C)])
    return x[S:S + C].cpu().numpy(), info.act[S:S + C].cpu().numpy(), fwd, rev


for x0 in ((0.005, 0.0), (1.0, 0.0)):                                 # a small offset: u_0 inside its limits; a large one: on its limit
    u0, act, fwd, rev = gains(x0)
    print("x_0 = %s: u_0 = %s, %s" % (x0, np.round(u0, 6), "on its limit" if act.any() else "inside its limits"))
    print("  du_0/dx_0 from %d tangents in one call : %s" % (S, np.array2string(fwd, precision=8)))
    print("  du_0/dx_0 from %d backward pass(es)     : %s" % (C, np.array2string(rev, precision=8)))
    assert np.abs(fwd - rev).max() <= 1e-8 * max(1.0, np.abs(rev).max())
    for i in range(C):
        if act[i]:
            assert not fwd[i].any()                                    # a saturated control does not move with x_0
        else:
            assert np.abs(fwd[i]).max() > 0
