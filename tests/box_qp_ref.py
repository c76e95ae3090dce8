"""numpy reference of the box-constrained QP solve, fp64, for the tests.

The problem, per system:  min 1/2 x^T H x - g^T x  s.t.  C x = c,  lo <= x <= hi,  H = G + rho I  (the solver's KKT system
M [dz; lambda] = [g; c] plus a box in the dz layout).  admm() restates the device iteration with dense solves of the x-step
matrix; qp_kkt_residuals() is an algorithm-free optimality check of a returned point.  H and C may be scipy.sparse matrices
(sparse_parts): the solves then go through scipy.sparse.linalg.splu, which reaches horizons the dense path cannot hold
(the KKT matrix of 2/1/8197 would take 13 GB)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gato_python_amd import synth                 # noqa: E402

CONVERGED, MAX_ITERS, NONFINITE, BAD_BOUNDS = 0, 1, 2, 3


def parts(s):
    """(H, C, g, c) of a KKTSystem in fp64, H with the solver's rho added (synth.dense_kkt)."""
    M, rhs = synth.dense_kkt(s)
    N = s.N
    return M[:N, :N].copy(), M[N:, :N].copy(), rhs[:N].copy(), rhs[N:].copy()


def sparse_parts(s):
    """parts(s) as scipy.sparse CSR matrices, straight from the system's CSR arrays: the same entries, bit for bit."""
    from scipy import sparse
    N, SK = s.N, s.S * s.K
    G = sparse.csr_matrix((np.asarray(s.G_val, np.float64), s.G_col, s.G_row), shape=(N, N))
    Cm = sparse.csr_matrix((np.asarray(s.C_val, np.float64), s.C_col, s.C_row), shape=(SK, N))
    H = (G + s.rho * sparse.identity(N, format="csr")).tocsr()
    return H, Cm, np.asarray(s.g, np.float64).copy(), np.asarray(s.c, np.float64).copy()


def is_sparse(M):
    from scipy import sparse
    return sparse.issparse(M)


def kkt_solver(H, Cm, diag=None):
    """solve(rhs) of [[H + diag(diag), C^T], [C, 0]]: an LU factorisation, dense (scipy.linalg.lu_factor) or sparse (splu)
    as H is."""
    N, m = H.shape[0], Cm.shape[0]
    if is_sparse(H):
        from scipy import sparse
        from scipy.sparse.linalg import splu
        Hd = H if diag is None else H + sparse.diags(np.broadcast_to(diag, (N,)))
        lu = splu(sparse.bmat([[Hd, Cm.T], [Cm, None]], format="csc"))
        return lu.solve
    from scipy.linalg import lu_factor, lu_solve
    Hd = H if diag is None else H + np.diag(np.broadcast_to(diag, (N,)))
    lu = lu_factor(np.block([[Hd, Cm.T], [Cm, np.zeros((m, m))]]))
    return lambda rhs: lu_solve(lu, rhs)


def dz_layout(xv, uv, S, C, K):
    """Per-knot state values xv [K, S] and control values uv [K-1, C] -> one vector in the dz layout (x_k then u_k)."""
    xv, uv = np.broadcast_to(xv, (K, S)), np.broadcast_to(uv, (K - 1, C))
    return np.concatenate([np.concatenate([xv[:K - 1], uv], 1).reshape(-1), xv[K - 1]])


def penalties(lo, hi, admm_rho):
    """rho_i: 0 free (both bounds infinite), 1e3 admm_rho where lo == hi, admm_rho otherwise."""
    free = np.isneginf(lo) & np.isposinf(hi)
    return np.where(free, 0.0, np.where(lo == hi, 1e3 * admm_rho, admm_rho))


def residuals(H, Cm, g, c, x, z, y, lam):
    """(r_prim, r_dual, primal scale, dual scale) of the device's termination test."""
    Hx, Ctl = H @ x, Cm.T @ lam
    nrm = lambda v: float(np.abs(v).max()) if v.size else 0.0
    r_prim = max(nrm(x - z), nrm(Cm @ x - c))
    r_dual = nrm(Hx - g + Ctl + y)
    return r_prim, r_dual, max(nrm(x), nrm(z), nrm(c)), max(nrm(Hx), nrm(Ctl), nrm(y), nrm(g))


def admm(H, Cm, g, c, lo, hi, *, admm_rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_admm_iters=4000,
         z0=None, y0=None):
    """The device iteration with exact (LU) x-steps.  Returns dict x, z, y, lam, iters, status, res_prim, res_dual - the iterate
    after `iters` x-steps, where the test first passed (or the last one: MAX_ITERS)."""
    N, m = H.shape[0], Cm.shape[0]
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rho = penalties(lo, hi, admm_rho)
    free = rho == 0
    solve = kkt_solver(H, Cm, sigma + rho)
    z = np.clip(np.zeros(N) if z0 is None else np.asarray(z0, np.float64), lo, hi)
    x = z.copy()
    y = np.where(free, 0.0, np.zeros(N) if y0 is None else np.asarray(y0, np.float64))
    lam = np.zeros(m)
    for it in range(1, max_admm_iters + 1):
        gt = g + sigma * x + rho * z - y
        sol = solve(np.concatenate([gt, c]))
        xt, lam = sol[:N], sol[N:]
        xh = alpha * xt + (1 - alpha) * z
        x = alpha * xt + (1 - alpha) * x
        with np.errstate(divide="ignore", invalid="ignore"):
            zn = np.where(free, xh, np.clip(xh + y / np.where(free, 1.0, rho), lo, hi))
        y = np.where(free, 0.0, y + rho * (xh - zn))
        z = zn
        rp, rd, sp, sd = residuals(H, Cm, g, c, x, z, y, lam)
        if not (np.isfinite(rp) and np.isfinite(rd)):
            status = NONFINITE
            break
        if rp <= eps_abs + eps_rel * sp and rd <= eps_abs + eps_rel * sd:
            status = CONVERGED
            break
    else:
        status = MAX_ITERS
    return dict(x=x, z=z, y=y, lam=lam, iters=it, status=status, res_prim=rp, res_dual=rd)


def qp_kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam):
    """Optimality of (x, y, lam) for the QP, independent of the algorithm (infinity norms):
    stationarity H x - g + C^T lam + y, equality C x - c, bound violation of x, and complementarity - y_i > 0 only where
    x_i = hi_i, y_i < 0 only where x_i = lo_i (measured as |y_i| times the distance to the bound its sign names; a sign
    that names an infinite bound counts |y_i|)."""
    x, y, lam = (np.asarray(v, np.float64) for v in (x, y, lam))
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    up = np.maximum(y, 0.0) * np.where(np.isposinf(hi), 1.0, np.abs(hi - x))
    dn = np.maximum(-y, 0.0) * np.where(np.isneginf(lo), 1.0, np.abs(x - lo))
    viol = np.maximum(np.maximum(lo - x, x - hi), 0.0)
    return dict(stat=float(np.abs(H @ x - g + Cm.T @ lam + y).max()), eq=float(np.abs(Cm @ x - c).max()),
                bound=float(viol.max()), comp=float(np.maximum(up, dn).max()))


def objective(H, g, x):
    return float(0.5 * x @ H @ x - g @ x)


def double_integrator(K=20, dt=0.1, x0=(1.0, 0.0), u_max=0.5, v_max=None, rho=1e-6):
    """A double integrator (S = 2: position, velocity; C = 1: force) driven to 0 from x0 with |u| <= u_max (and
    |velocity| <= v_max): (KKTSystem, lo, hi).  Blocks as kkt_solve takes them: C holds -A, -B; c_0 = -x0 pins x_0."""
    S, C = 2, 1
    a = np.array([[1.0, dt], [0.0, 1.0]])
    b = np.array([[0.5 * dt * dt], [dt]])
    Q = np.tile(np.diag([10.0, 1.0]), (K, 1, 1))
    Q[-1] = np.diag([100.0, 10.0])
    R = np.tile(0.1 * np.eye(C), (K - 1, 1, 1))
    A = np.tile(-a, (K - 1, 1, 1))
    B = np.tile(-b, (K - 1, 1, 1))
    q, r = np.zeros((K, S)), np.zeros((K - 1, C))
    c = np.zeros((K, S))
    c[0] = -np.asarray(x0, np.float64)
    s = synth.blocks_to_csr(Q, R, A, B, q, r, c, rho=rho)
    vm = np.inf if v_max is None else v_max
    lo = dz_layout(np.array([-np.inf, -vm]), -u_max, S, C, K)
    hi = dz_layout(np.array([np.inf, vm]), u_max, S, C, K)
    return s, lo, hi, (Q, R, A, B, q, r, c)


def pendulum_box(u_max=0.2):
    """The reference's pendulum system (synth.pendulum_system) with |u| <= u_max: (KKTSystem, lo, hi)."""
    s = synth.pendulum_system()
    lo = dz_layout(np.full(s.S, -np.inf), -u_max, s.S, s.C, s.K)
    hi = dz_layout(np.full(s.S, np.inf), u_max, s.S, s.C, s.K)
    return s, lo, hi
