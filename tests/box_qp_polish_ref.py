"""numpy reference of the box-QP polish and of the gradients through a polished solution, fp64.

The problem is that of box_qp_ref:  min 1/2 x^T H x - g^T x  s.t.  C x = c,  lo <= x <= hi,  H = G + rho I  (dz layout).
active_set() is OSQP's rule on (z, y) of an ADMM result; reduced_solve() is the exact KKT solution with the active variables
fixed at their bounds, [[H_FF, C_F^T], [C_F, 0]] [x_F; lam] = [g_F - H_FA b_A; c - C_A b_A]; polish() adds the device's
acceptance test; grads() is the backward pass of DESIGN.md section 3.6 applied to the reduced system."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_ref as ref                          # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
from gato_python_amd import synth                 # noqa: E402

ACCEPTED, REJECTED, NONFINITE, BAD_ACTIVE = 0, 1, 2, 3


def active_set(z, y, lo, hi, S):
    """act [N] int8: +1 upper where hi - z < y, -1 lower where z - lo < -y, -1 wherever lo == hi, 0 otherwise, and 0 on the
    S coordinates of x_0 (row block 0 of C pins them).  An infinite bound is never active by the rule itself."""
    z, y, lo, hi = (np.asarray(v) for v in (z, y, lo, hi))
    act = np.zeros(z.shape, np.int8)
    with np.errstate(invalid="ignore"):
        act[hi - z < y] = 1
        act[z - lo < -y] = -1
    act[lo == hi] = -1
    act[..., :S] = 0
    return act


def bound_values(act, lo, hi):
    """b: hi where act = +1, lo where act = -1, 0 on free coordinates."""
    return np.where(act > 0, hi, np.where(act < 0, lo, 0.0))


def _reduced_matrix(H, Cm, act):
    F = act == 0
    m = Cm.shape[0]
    return np.block([[H[np.ix_(F, F)], Cm[:, F].T], [Cm[:, F], np.zeros((m, m))]]), F


def reduced_solve(H, Cm, g, c, lo, hi, act):
    """(x, y, lam) of the reduced KKT system: x_A = b_A exactly, y_A = (g - H x - C^T lam)_A, y_F = 0.  A singular reduced
    system (LICQ fails) gives NaN."""
    act = np.asarray(act)
    A = act != 0
    b = bound_values(act, lo, hi)
    M, F = _reduced_matrix(H, Cm, act)
    rhs = np.concatenate([g[F] - H[np.ix_(F, A)] @ b[A], c - Cm[:, A] @ b[A]])
    try:
        sol = np.linalg.solve(M, rhs)
    except np.linalg.LinAlgError:
        sol = np.full(M.shape[0], np.nan)
    x = np.zeros(len(g))
    x[A] = b[A]
    x[F] = sol[:F.sum()]
    lam = sol[F.sum():]
    y = np.zeros(len(g))
    y[A] = (g - H @ x - Cm.T @ lam)[A]
    return x, y, lam


def polish(H, Cm, g, c, lo, hi, z, y, S, eps_abs=1e-6, eps_rel=1e-6, act=None):
    """The device's polish of one ADMM result (z, y): dict decision, act, x, z, y, lam, res_prim, res_dual (of the polished
    point; the caller keeps its ADMM point unless decision == ACCEPTED)."""
    act = active_set(z, y, lo, hi, S) if act is None else np.asarray(act)
    x, yp, lam = reduced_solve(H, Cm, g, c, lo, hi, act)
    zp = np.clip(x, lo, hi)
    with np.errstate(invalid="ignore"):
        rp, rd, sp, sd = ref.residuals(H, Cm, g, c, x, zp, yp, lam)
    out = dict(act=act, x=x, z=zp, y=yp, lam=lam, res_prim=rp, res_dual=rd)
    if not all(np.isfinite(v).all() for v in (x, zp, yp, lam)) or not (np.isfinite(rp) and np.isfinite(rd)):
        out["decision"] = NONFINITE
        return out
    tol_d = eps_abs + eps_rel * sd
    eq = lo == hi
    sign_ok = np.all(yp[(act > 0) & ~eq] >= -tol_d) and np.all(yp[(act < 0) & ~eq] <= tol_d)
    ok = rp <= eps_abs + eps_rel * sp and rd <= tol_d and sign_ok
    out["decision"] = ACCEPTED if ok else REJECTED
    return out


def adjoint(H, Cm, act, xbar, lambar):
    """[a; beta] of the reduced system for upstream gradients (xbar, lambar): a_A = 0."""
    M, F = _reduced_matrix(H, Cm, np.asarray(act))
    sol = np.linalg.solve(M, np.concatenate([np.asarray(xbar, np.float64)[F], np.asarray(lambar, np.float64)]))
    a = np.zeros(H.shape[0])
    a[F] = sol[:F.sum()]
    return a, sol[F.sum():]


def bound_grads(H, Cm, act, xbar, a, beta):
    """(lo_bar, hi_bar) [N]: on A, xbar - (H a + C^T beta) goes to hi for act = +1 and to lo for act = -1 (lo == hi: to lo,
    hi gets 0); free coordinates get 0 in both."""
    act = np.asarray(act)
    bb = np.where(act != 0, np.asarray(xbar, np.float64) - (H @ a + Cm.T @ beta), 0.0)
    return np.where(act < 0, bb, 0.0), np.where(act > 0, bb, 0.0)


def grads(H, Cm, act, x, lam, xbar, lambar, S, C, K):
    """Gradients of L = xbar . x + lambar . lam through the polished solution with respect to all eleven inputs of
    box_qp_layer: dict Q, R, A, B, q, r, c (kkt_grad_ref.grads_math on the reduced adjoint) and x_lo, x_hi [K, S], u_lo,
    u_hi [K-1, C]; also a, beta, lo, hi (dz layout)."""
    a, beta = adjoint(H, Cm, act, xbar, lambar)
    out = kgr.grads_math(x, lam, a, beta, S, C, K)
    lo_bar, hi_bar = bound_grads(H, Cm, act, xbar, a, beta)
    out["x_lo"], out["u_lo"] = split_states_controls(lo_bar, S, C, K)
    out["x_hi"], out["u_hi"] = split_states_controls(hi_bar, S, C, K)
    out.update(a=a, beta=beta, lo=lo_bar, hi=hi_bar)
    return out


def split_states_controls(v, S, C, K):
    """dz-layout vector -> (per-knot states [K, S], controls [K-1, C]); the inverse of box_qp_ref.dz_layout."""
    n = S + C
    v = np.asarray(v, np.float64)
    xs = np.stack([v[k * n: k * n + S] for k in range(K)])
    us = np.stack([v[k * n + S: (k + 1) * n] for k in range(K - 1)]) if K > 1 else np.zeros((0, C))
    return xs, us


def dense_from_blocks(Q, R, A, B, q, r, c, rho):
    """(H, C, g, c) of math-shaped blocks as box_qp takes them (A, B the raw values stored in C; C's identity blocks
    explicit), H with rho added: the dense problem finite differences perturb."""
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    n, N = S + C, (S + C) * K - C
    H = np.zeros((N, N))
    Cm = np.zeros((S * K, N))
    for k in range(K):
        H[k * n: k * n + S, k * n: k * n + S] = Q[k]
        Cm[k * S: (k + 1) * S, k * n: k * n + S] = np.eye(S)
        if k < K - 1:
            H[k * n + S: (k + 1) * n, k * n + S: (k + 1) * n] = R[k]
            Cm[(k + 1) * S: (k + 2) * S, k * n: k * n + S] = A[k]
            Cm[(k + 1) * S: (k + 2) * S, k * n + S: (k + 1) * n] = B[k]
    H += rho * np.eye(N)
    return H, Cm, ref.dz_layout(q, r, S, C, K), np.asarray(c, np.float64).reshape(-1).copy()


# ---- the problems of DESIGN.md section 3.8 ------------------------------------------------------------------------------
def boxes(s, seed, eq=True, states=True):
    """The box of tests/test_gpu_box_qp.py's boxes(): controls and every other state bounded around half their unconstrained
    value, x_0 free, one control fixed (lo == hi) when eq.  states=False: the states are all free (a control-only box)."""
    rng = np.random.default_rng(seed)
    dz, _ = synth.dense_kkt_solve(s)
    n, N = s.S + s.C, s.N
    w = 0.5 * np.abs(dz) + 0.05 * rng.uniform(0.5, 1.5, N)
    lo, hi = -w, w.copy()
    idx = np.arange(N)
    state = (idx % n) < s.S
    free = (idx < s.S) | (state & ((idx % 2 == 1) | (not states)))
    lo[free], hi[free] = -np.inf, np.inf
    if eq:
        j = s.S + n * (s.K // 2)
        lo[j] = hi[j] = 0.25 * dz[j]
    return lo, hi


def problem(name):
    """(KKTSystem, lo, hi, admm_rho) of one problem of the table."""
    if name == "pendulum":
        s, lo, hi = ref.pendulum_box(0.2)
        return s, lo, hi, 0.1
    if name == "double_integrator":
        s, lo, hi, _ = ref.double_integrator(K=20, u_max=0.5, v_max=0.57)
        return s, lo, hi, 0.1
    if name == "6_3_20":
        s = synth.make_system(6, 3, 20, seed=2)
        lo, hi = boxes(s, 3)
        return s, lo, hi, 10.0
    if name == "14_7_50":
        s = synth.make_system(14, 7, 50, seed=0)
        lo, hi = boxes(s, 3, eq=False, states=False)
        return s, lo, hi, 1.0
    raise KeyError(name)


PROBLEMS = ("pendulum", "double_integrator", "6_3_20", "14_7_50")
# ADMM iterations (eps_abs = eps_rel = 0) after which the rule gives the exact active set, with margin over the first one
EXACT_FROM = dict(pendulum=50, double_integrator=2000, **{"6_3_20": 2000, "14_7_50": 100})


def exact_active(name):
    """(act, H, C, g, c, lo, hi) of a problem: the active set of its ADMM iterate after EXACT_FROM iterations."""
    s, lo, hi, arho = problem(name)
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, admm_rho=arho, eps_abs=0.0, eps_rel=0.0, max_admm_iters=EXACT_FROM[name])
    return active_set(out["z"], out["y"], lo, hi, s.S), H, Cm, g, c, lo, hi
