"""Learn the state-cost weights of a linear-quadratic controller from an expert trajectory, by gradient descent through the
KKT solve (gato_python_amd.kkt_solve, torch autograd: the backward is one adjoint re-solve plus one gradient kernel).

The plant is two double integrators (S = 4, C = 2).  The expert drives it from rest to a goal with the diagonal state weights
W_TRUE; the learner starts from unit weights and fits log-weights with Adam so that its planned trajectory matches the
expert's.  The loss falls and the weights approach W_TRUE.      python examples/learn_cost_weights.py [steps]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
from gato_python_amd import kkt_solve                  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 150
K, dt, S, C = 20, 0.1, 4, 2
dev, f64 = "cuda:0", torch.float64
a = np.array([[1.0, dt], [0.0, 1.0]])
b = np.array([[0.5 * dt * dt], [dt]])
A_dyn, B_dyn = np.kron(np.eye(2), a), np.kron(np.eye(2), b)
W_TRUE = torch.tensor([5.0, 0.5, 2.0, 0.2], dtype=f64, device=dev)
goal = torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=f64, device=dev)
x0 = torch.zeros(S, dtype=f64, device=dev)
opts = dict(rho=1e-8, exit_tol=1e-20, max_iters=500)

# the constraint rows x_k+1 - A x_k - B u_k = 0 store -A and -B; x_0 = c_0
A = -torch.tensor(A_dyn, dtype=f64, device=dev).expand(K - 1, S, S)
B = -torch.tensor(B_dyn, dtype=f64, device=dev).expand(K - 1, S, C)
R = 0.1 * torch.eye(C, dtype=f64, device=dev).expand(K - 1, C, C)
r = torch.zeros(K - 1, C, dtype=f64, device=dev)
c = torch.zeros(K, S, dtype=f64, device=dev)
c[0] = x0


def plan(w):
    """min sum_k 1/2 (x_k - goal)^T diag(w) (x_k - goal) + 1/2 u_k^T R u_k: G dz + C^T lam = g with q_k = diag(w) goal."""
    Q = torch.diag_embed(w).expand(K, S, S)
    q = (w * goal).expand(K, S)
    lam, dz = kkt_solve(Q, R, A, B, q, r, c, **opts)
    return dz


with torch.no_grad():
    expert = plan(W_TRUE)
log_w = torch.zeros(S, dtype=f64, device=dev, requires_grad=True)
opt = torch.optim.Adam([log_w], lr=0.1)
first = None
for step in range(STEPS + 1):
    opt.zero_grad()
    loss = ((plan(log_w.exp()) - expert) ** 2).mean()
    loss.backward()
    first = first if first is not None else loss.item()
    if step % (STEPS // 10 or 1) == 0:
        print(f"step {step:4d}  loss {loss.item():.3e}  weights {np.round(log_w.exp().detach().cpu().numpy(), 3)}")
    opt.step()
print(f"loss {first:.3e} -> {loss.item():.3e}; true weights {W_TRUE.cpu().numpy()}")
assert loss.item() < 0.05 * first, "the loss did not fall"
