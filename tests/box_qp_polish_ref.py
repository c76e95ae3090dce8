"""numpy reference of the box-QP polish and of the gradients through a polished solution, fp64.

The problem is that of box_qp_ref:  min 1/2 x^T H x - g^T x  s.t.  C x = c,  lo <= x <= hi,  H = G + rho I  (dz layout).
active_set() is OSQP's rule on (z, y) of an ADMM result; reduced_solve() is the exact KKT solution with the active variables
fixed at their bounds, [[H_FF, C_F^T], [C_F, 0]] [x_F; lam] = [g_F - H_FA b_A; c - C_A b_A]; polish() adds the device's
acceptance test; grads() is the backward pass of DESIGN.md section 3.6 applied to the reduced system.  The reduced system is
also that of the active-set iteration (box_qp_active_ref), whose bounds may be soft (a weight vector
w >= 0, w_i > 0 penalises the bound of variable i by (w_i / 2) dist^2; a soft-active variable stays in the system, its
diagonal entry gains w_i, g gains w_i b_i, and its multiplier is the force y_i = w_i (x_i - b_i)) and capped (section 3.11: a
cap m_i on that force; act = +-2 names a saturated variable, free in the system with g_i - s m_i and y_i = s m_i).  w=None
means all hard, m=None no caps; every function here is one implementation for the three forms.  H and C may be
scipy.sparse matrices (box_qp_ref.sparse_parts).  constructed_problem() builds QPs with a known active set (active states
included) at any shape, constructed() walks its seeds by a rule on the reference alone, and reduced_stage_solve() restates
the device's route to the reduced solution on the oracle's stages in a given dtype."""
import dataclasses
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


def _cols(M, idx):
    return M[:, idx]


def _sub(M, rows, cols):
    return M[rows][:, cols] if ref.is_sparse(M) else M[np.ix_(rows, cols)]


def soft_set(act, w=None):
    """The soft-active variables: active with a positive weight (the saturated ones included)."""
    act = np.asarray(act)
    return (act != 0) & (np.asarray(w) > 0) if w is not None else np.zeros(act.shape, bool)


def sat_set(act):
    """The saturated variables: act = +-2."""
    return np.abs(np.asarray(act, np.int64)) == 2


def hard_set(act, w=None):
    """The hard-active variables: active, not soft, eliminated from the reduced system."""
    return (np.asarray(act) != 0) & ~soft_set(act, w)


def unsaturated(act):
    """act with the saturated variables free: the act whose quadratic reduced system the saturated one shares."""
    act = np.asarray(act, np.int8)
    return np.where(sat_set(act), 0, act).astype(np.int8)


def _reduced_solver(H, Cm, act, w=None):
    """(solve, F) of the reduced matrix [[H_FF + diag(w) on the soft-active, C_F^T], [C_F, 0]]; F the indices of the variables
    that are not hard-active.  solve(rhs) gives NaN where the matrix is singular (LICQ fails).  Dense: np.linalg.solve;
    sparse: one splu factorisation."""
    act = unsaturated(act)
    soft = soft_set(act, w)
    F = np.flatnonzero(~hard_set(act, w))
    if not ref.is_sparse(H):
        M = reduced_matrix(H, Cm, act, w)

        def solve(rhs):
            try:
                return np.linalg.solve(M, rhs)
            except np.linalg.LinAlgError:
                return np.full(len(rhs), np.nan)
        return solve, F
    try:
        solve = ref.kkt_solver(_sub(H, F, F), _cols(Cm, F), diag=np.where(soft, w, 0.0)[F] if soft.any() else None)
    except RuntimeError:                                  # splu: "Factor is exactly singular"
        solve = lambda rhs: np.full(len(rhs), np.nan)
    return solve, F


def reduced_matrix(H, Cm, act, w=None):
    """The dense reduced matrix [[H_FF, C_F^T], [C_F, 0]], w_i on the diagonal of the soft-active (for its condition number;
    dense sizes only)."""
    act = unsaturated(act)
    soft = soft_set(act, w)
    F = np.flatnonzero(~hard_set(act, w))
    m = Cm.shape[0]
    dense = lambda M: M.toarray() if ref.is_sparse(M) else M
    M = np.block([[dense(_sub(H, F, F)), dense(_cols(Cm, F)).T], [dense(_cols(Cm, F)), np.zeros((m, m))]])
    if soft.any():
        M[np.arange(len(F)), np.arange(len(F))] += np.where(soft, w, 0.0)[F]
    return M


def reduced_solve(H, Cm, g, c, lo, hi, act, w=None, m=None):
    """(x, y, lam) of the reduced KKT system: x_i = b_i exactly and y_i = (g - H x - C^T lam)_i on the hard-active set, y_i =
    w_i (x_i - b_i) on the soft-active one, y_i = s m_i on the saturated one, y = 0 elsewhere.  A singular reduced system (LICQ
    fails) gives NaN.  H, Cm dense or scipy.sparse."""
    act = np.asarray(act)
    sat = sat_set(act)
    if sat.any():
        push = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), 0.0)
        g, act = g - push, unsaturated(act)
    soft = soft_set(act, w)
    A = np.flatnonzero(hard_set(act, w))
    b = bound_values(act, lo, hi)
    solve, F = _reduced_solver(H, Cm, act, w)
    top = g[F] + (np.where(soft, w, 0.0) * b)[F] if soft.any() else g[F]
    sol = solve(np.concatenate([top - _sub(H, F, A) @ b[A], c - _cols(Cm, A) @ b[A]]))
    x = np.zeros(len(g))
    x[A] = b[A]
    x[F] = sol[:len(F)]
    lam = sol[len(F):]
    y = np.zeros(len(g))
    y[A] = (g - H @ x - Cm.T @ lam)[A]
    if soft.any():
        y[soft] = (w * (x - b))[soft]
    if sat.any():
        y = np.where(sat, push, y)
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


def adjoint(H, Cm, act, xbar, lambar, w=None):
    """[a; beta] of the reduced system for upstream gradients (xbar, lambar): a = 0 on the hard-active set."""
    solve, F = _reduced_solver(H, Cm, act, w)
    sol = solve(np.concatenate([np.asarray(xbar, np.float64)[F], np.asarray(lambar, np.float64)]))
    a = np.zeros(H.shape[0])
    a[F] = sol[:len(F)]
    return a, sol[len(F):]


def bound_grads(H, Cm, act, xbar, a, beta, w=None, lo=None, hi=None, x=None):
    """(lo_bar, hi_bar) [N], and with weights (lo_bar, hi_bar, w_bar): b_bar is xbar_i - (H a + C^T beta)_i on a hard-active i
    and w_i a_i on a soft-active one, and goes to hi for act = +1 and to lo for act = -1 (lo == hi: to lo, hi gets 0); w_bar_i =
    a_i (b_i - x_i) on the soft-active; 0 elsewhere."""
    act = np.asarray(act)
    soft = soft_set(act, w)
    bb = np.where(hard_set(act, w), np.asarray(xbar, np.float64) - (H @ a + Cm.T @ beta), 0.0)
    if w is None:
        return np.where(act < 0, bb, 0.0), np.where(act > 0, bb, 0.0)
    bb = np.where(soft, w * a, bb)
    return np.where(act < 0, bb, 0.0), np.where(act > 0, bb, 0.0), np.where(soft, a * (bound_values(act, lo, hi) - x), 0.0)


def grads(H, Cm, act, x, lam, xbar, lambar, S, C, K, w=None, m=None, lo=None, hi=None):
    """Gradients of L = xbar . x + lambar . lam through a converged point with respect to the inputs of box_qp_layer: dict Q, R,
    A, B, q, r, c (kkt_grad_ref.grads_math on the reduced adjoint) and x_lo, x_hi [K, S], u_lo, u_hi [K-1, C]; with w (and lo,
    hi) also x_soft, u_soft; with m also x_soft_max, u_soft_max - the saturated variables are free, get 0 in lo, hi and w, and
    m_bar_i = -s a_i.  Eleven, thirteen or fifteen inputs; also a, beta, lo, hi (and w, m) in the dz layout."""
    sat, sign = sat_set(act), np.sign(np.asarray(act, np.int8))
    act = unsaturated(act)
    a, beta = adjoint(H, Cm, act, xbar, lambar, w)
    out = kgr.grads_math(x, lam, a, beta, S, C, K)
    bars = dict(zip(("lo", "hi", "w"), bound_grads(H, Cm, act, xbar, a, beta, w, lo, hi, x)))
    if m is not None:
        bars["m"] = np.where(sat, -sign * a, 0.0)
    for k, name in (("lo", "lo"), ("hi", "hi"), ("w", "soft"), ("m", "soft_max")):
        if k in bars:
            out["x_" + name], out["u_" + name] = split_states_controls(bars[k], S, C, K)
    out.update(a=a, beta=beta, **bars)
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
def boxes(s, seed, eq=True, states=True, dz=None):
    """The box of tests/test_gpu_box_qp.py's boxes(): controls and every other state bounded around half their unconstrained
    value, x_0 free, one control fixed (lo == hi) when eq.  states=False: the states are all free (a control-only box).
    dz: the unconstrained solution, where the dense solve that finds it otherwise is out of reach."""
    rng = np.random.default_rng(seed)
    if dz is None:
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


# ---- constructed problems: a known active set with active states, without running ADMM -----------------------------------
def constructed_system(S, C, K, seed):
    """synth's seeded system with dense Q_k and R_k (synth.make_blocks(dense_q=True) plus a dense positive semidefinite
    part on R_k): with diagonal blocks a wrong mask, a transposed index or a missed shift through H_:A would change
    nothing."""
    Q, R, A, B, q, r, c = synth.make_blocks(S, C, K, seed, dense_q=True)
    M = 0.1 * np.random.default_rng([seed, 11]).standard_normal((K - 1, C, C))
    return synth.blocks_to_csr(Q, R + M @ M.transpose(0, 2, 1), A, B, q, r, c)


def constructed_problem(S, C, K, seed, sparse=False, scale=1.0, release=0.0):
    """A box QP on constructed_system(S, C, K, seed) whose exact solution has a known active set, built backwards:
      1. the active index set A: per knot k < K-1 about half the controls (at least one where C >= 2; with C = 1 the
         control, or nothing where a state of the next knot must be active), per knot k >= 1 a random number of states
         between 0 and min(free controls of knot k-1, S-1) - so that LICQ holds generically - with at least one state of
         knot 1 and one of the last knot when K >= 3, and never a state of x_0;
      2. bound values b_A = 0.5 dz_A + 0.05 N(0, 1), dz the unconstrained solution;
      3. one reduced solve with every active variable an upper bound gives y_A;
      4. act = sign(y_A) (+1 where y >= 0) and b on that side; every other active variable gets a finite opposite bound
         at distance 1 + |b|, the rest an infinite one;
      5. every third free variable gets a loose finite box around x, and one active control lo == hi when K >= 3, C >= 2.
    Long horizons (thousands of active variables, states that drift over thousands of knots) cannot meet the seed rule
    as built above - the smallest of 6000 multipliers is below 1e-3 and |x| reaches 1e2 on every seed - so two knobs of
    the construction, not of the rule, exist for them: scale multiplies g, c and the noise of b (and with them x, y, lam), after
    step 3 the active variables with |y| < release are set free and the solve repeated until none is left.
    The reduced point is then the QP's optimum by construction.  Returns a dict: s, H, Cm, g, c (dense, or scipy.sparse
    with sparse=True), lo, hi, act, x, y, lam, seed."""
    s = constructed_system(S, C, K, seed)
    s.g, s.c = s.g * scale, s.c * scale
    H, Cm, g, c = ref.sparse_parts(s) if sparse else ref.parts(s)
    rng = np.random.default_rng([seed, S, C, K])
    n, N = S + C, s.N
    inf = np.full(N, np.inf)
    dz, _, _ = reduced_solve(H, Cm, g, c, -inf, inf, np.zeros(N, np.int8))
    A = np.zeros(N, bool)
    free_prev = 0
    for k in range(K):
        if k >= 1:
            most = min(free_prev, S - 1)
            ns = int(rng.integers(0, most + 1))
            if K >= 3 and k in (1, K - 1):
                ns = max(ns, 1)
            A[k * n + rng.permutation(S)[:ns]] = True
        if k < K - 1:
            must_leave = K >= 3 and k in (0, K - 2)                 # a state of knot k+1 must be active: keep a control free
            if C >= 2:
                nc = int(np.clip(C // 2 + rng.integers(-1, 2), 1, C - 1))
            else:
                nc = 0 if must_leave else (1 if K == 2 else int(rng.integers(0, 2)))
            A[k * n + S + rng.permutation(C)[:nc]] = True
            free_prev = C - nc
    b = np.where(A, 0.5 * dz + 0.05 * scale * rng.standard_normal(N), 0.0)
    _, y0, _ = reduced_solve(H, Cm, g, c, -inf, np.where(A, b, np.inf), A.astype(np.int8))
    while release > 0 and np.any(np.abs(y0[A]) < release):
        A &= np.abs(y0) >= release
        b = np.where(A, b, 0.0)
        _, y0, _ = reduced_solve(H, Cm, g, c, -inf, np.where(A, b, np.inf), A.astype(np.int8))
    act = np.where(A, np.where(y0 >= 0, 1, -1), 0).astype(np.int8)
    lo, hi = -inf, inf.copy()
    lo[act < 0], hi[act > 0] = b[act < 0], b[act > 0]
    other = np.zeros(N, bool)
    other[np.flatnonzero(A)[::2]] = True
    lo[other & (act > 0)] = (b - (1 + np.abs(b)))[other & (act > 0)]
    hi[other & (act < 0)] = (b + (1 + np.abs(b)))[other & (act < 0)]
    if K >= 3 and C >= 2:
        j = (K // 2) * n + S + np.flatnonzero(A[(K // 2) * n + S: (K // 2 + 1) * n])[0]
        lo[j] = hi[j] = b[j]
        act[j] = -1
    x, y, lam = reduced_solve(H, Cm, g, c, lo, hi, act)
    loose = np.flatnonzero(~A)[::3]
    w = (1 + np.abs(x[loose])) * rng.uniform(0.5, 1.5, len(loose))
    lo[loose], hi[loose] = x[loose] - w, x[loose] + w
    return dict(s=s, H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, act=act, x=x, y=y, lam=lam, seed=seed)


COND_CAP = 1e8
# the cases of tests/test_gpu_qp_kernel_sweep.py (the CPU suite checks that the seed rule finds a seed for each)
SWEEP_SHAPES = [(2, 1), (4, 2), (6, 3), (12, 6), (14, 7), (32, 16)]
SWEEP_SHORT_K = (2, 3, 9)
SWEEP_F32 = [(S, C, 9) for S, C in SWEEP_SHAPES] + [(14, 7, 3), (32, 16, 3)]
SWEEP_BATCH = (14, 7, 9, 5)                       # S, C, K, systems of the batch test
SWEEP_LONG = (2, 1, 8197)
F32_EPS = 1e-4                                    # eps_abs = eps_rel of the fp32 polishes


def meets_seed_rule(p, cond=True):
    """The conditions a constructed problem must meet, from the reference alone: its polish ACCEPTED, cond(M_reduced) <=
    1e8 (dense sizes), |x| <= 10, every non-equality active multiplier at least 1e-3 from 0 and every bounded free
    variable at least 1e-3 inside its box.  -> (ok, dict of the measured figures)."""
    H, Cm, g, c, lo, hi, act, x, y = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi", "act", "x", "y"))
    N = len(g)
    dec = polish(H, Cm, g, c, lo, hi, np.zeros(N), np.zeros(N), p["s"].S, act=act)
    on, eq = act != 0, lo == hi
    fig = dict(decision=dec["decision"], res_prim=dec["res_prim"], res_dual=dec["res_dual"])
    if dec["decision"] != ACCEPTED:
        return False, fig
    fig["xmax"] = float(np.abs(x).max())
    fig["ymin"] = float(np.abs(y[on & ~eq]).min()) if (on & ~eq).any() else np.inf
    with np.errstate(invalid="ignore"):
        fig["inside"] = float(np.min(np.minimum(x - lo, hi - x)[~on]))
    fig["cond"] = float(np.linalg.cond(reduced_matrix(H, Cm, act))) if cond and not ref.is_sparse(H) else None
    ok = fig["xmax"] <= 10 and fig["ymin"] >= 1e-3 and fig["inside"] >= 1e-3 and (fig["cond"] is None or fig["cond"] <= COND_CAP)
    return bool(ok), fig


def rounded(p):
    """The problem with every input rounded to fp32 (values held in fp64; rho rounded too, and the weights "w" and caps "m" where
    it has them) and the fp64 reduced solution on its act: the truth an fp32 run is judged against."""
    s = p["s"].astype(np.float32).astype(np.float64)
    s.rho = float(np.float32(p["s"].rho))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    H, Cm, g, c = ref.parts(s)
    lo, hi = f32(p["lo"]), f32(p["hi"])
    wm = {k: f32(p[k]) for k in ("w", "m") if k in p}
    x, y, lam = reduced_solve(H, Cm, g, c, lo, hi, p["act"], **wm)
    return dict(p, s=s, H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, x=x, y=y, lam=lam, **wm)


def restatement_accepted(p, dtype, eps, max_iters=1000):
    """(accepted, pcg iterations): the acceptance test of polish() on the point reduced_stage_solve gives in `dtype`
    (residuals evaluated in fp64)."""
    H, Cm, g, c, lo, hi, act = (p[k] for k in ("H", "Cm", "g", "c", "lo", "hi", "act"))
    x, lam, iters = reduced_stage_solve(p["s"], lo, hi, act, dtype, max_iters=max_iters)
    x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
    if not (np.isfinite(x).all() and np.isfinite(lam).all()):
        return False, iters
    on, eq = act != 0, lo == hi
    y = np.where(on, g - H @ x - Cm.T @ lam, 0.0)
    rp, rd, sp, sd = ref.residuals(H, Cm, g, c, x, np.clip(x, lo, hi), y, lam)
    tol_d = eps + eps * sd
    sign_ok = np.all(y[(act > 0) & ~eq] >= -tol_d) and np.all(y[(act < 0) & ~eq] <= tol_d)
    return bool(rp <= eps + eps * sp and rd <= tol_d and sign_ok), iters


def f32_ok(p):
    """The further seed condition of the fp32 cases: the fp32 restatement of the rounded problem passes the acceptance
    test, and passes it with its PCG stopped one iteration sooner too.  In fp32 the PCG of these systems ends within a
    few iterations of the test's threshold (14/7/3 seed 0: |C x - c| 3.6e-4 one iteration before the exit, 8.4e-5 at it,
    the bar 2.1e-4), and another summation order leaves the loop an iteration sooner or later: a seed whose decision hangs
    on that last iteration decides nothing about a kernel."""
    q = rounded(p)
    ok, iters = restatement_accepted(q, np.float32, F32_EPS)
    return ok and iters >= 1 and restatement_accepted(q, np.float32, F32_EPS, max_iters=iters)[0]


_CONSTRUCTED = {}


LONG_KNOBS = dict(sparse=True, scale=1.0 / 64, release=2e-3)       # constructed_problem's knobs at SWEEP_LONG


def constructed(S, C, K, count=1, sparse=False, extra=None, tag=None, limit=20, **knobs):
    """The first `count` constructed problems of seeds 0, 1, 2, ... < limit that meet the seed rule (and extra(p), a further
    condition on the reference alone, cached under tag), as a list; fewer than count if the walk runs out."""
    key = (S, C, K, sparse, tag, tuple(sorted(knobs.items())))
    got = _CONSTRUCTED.setdefault(key, dict(next=0, found=[]))
    while len(got["found"]) < count and got["next"] < limit:
        p = constructed_problem(S, C, K, got["next"], sparse=sparse, **knobs)
        got["next"] += 1
        ok, fig = meets_seed_rule(p, cond=not sparse)
        if ok and (extra is None or extra(p)):
            p["figures"] = fig
            got["found"].append(p)
    return got["found"][:count]


def wrong_sign(p):
    """(act, index) of the constructed problem with the sign of one active non-equality control flipped (the first one whose
    opposite bound is finite, so that the flipped act names a finite bound)."""
    S, n = p["s"].S, p["s"].S + p["s"].C
    act, lo, hi = p["act"], p["lo"], p["hi"]
    idx = np.arange(len(act))
    cand = np.flatnonzero((act != 0) & (lo != hi) & (idx % n >= S) & np.isfinite(lo) & np.isfinite(hi))
    j = int(cand[0])
    flipped = act.copy()
    flipped[j] = -act[j]
    return flipped, j


# ---- the reduced stage path restated in a given dtype ----------------------------------------------------------------------
def reduced_stage_solve(s, lo, hi, act, dtype, exit_tol=1e-8, max_iters=1000, w=None, m=None):
    """What the device's reduced solve computes, restated in `dtype` on the oracle's stages: Q_k and R_k (rho added) with the
    hard-active rows and columns replaced by the identity, the oracle's Gauss-Jordan inverse, the hard-active entries zeroed;
    g' = g - H_:A b_A (0 on A), c' = c - C_:A b_A (C's identity blocks included); form_schur with those inverses, form_ss, pcg,
    compute_dz; x = b on A, dz elsewhere.  With weights the diagonal of Q_k, R_k gains w_i and g' gains w_i b_i on the
    soft-active set (0 elsewhere: the terms are added whenever w is given, as the device adds them); with caps a saturated
    variable is free, its g_i - s m_i formed in `dtype`.  -> (x, lam, pcg iterations)."""
    from oracle import gato_oracle as o
    dt = np.dtype(dtype).type
    act = np.asarray(act, np.int8)
    sat = sat_set(act)
    if sat.any():
        push = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), 0.0).astype(dt)
        s, act = dataclasses.replace(s, g=(np.asarray(s.g, dt) - push).astype(dt)), unsaturated(act)
    S, C, K, n = s.S, s.C, s.K, s.S + s.C
    Q, R, A, B, q, r, c = (np.asarray(t, dt) for t in kgr.blocks_of(s))
    rho = dt(s.rho)
    Q = Q + rho * np.eye(S, dtype=dt)
    R = R + rho * np.eye(C, dtype=dt)
    soft, on = soft_set(act, w), hard_set(act, w)
    ball = bound_values(act, np.asarray(lo, dt), np.asarray(hi, dt)).astype(dt)
    b = np.where(on, ball, dt(0)).astype(dt)
    xs, us = (np.arange(K)[:, None] * n + np.arange(S)), (np.arange(K - 1)[:, None] * n + S + np.arange(C))
    onx, onu, bx, bu = on[xs], on[us], b[xs], b[us]
    eye = lambda k: np.eye(k, dtype=dt)[None]
    mx, mu = onx[:, :, None] | onx[:, None, :], onu[:, :, None] | onu[:, None, :]
    Qw, Rw = Q, R
    if w is not None:
        d = np.where(soft, np.asarray(w, dt), dt(0)).astype(dt)
        db = (d * np.where(soft, ball, dt(0))).astype(dt)
        Qw = Q + d[xs][:, :, None] * np.eye(S, dtype=dt)
        Rw = R + d[us][:, :, None] * np.eye(C, dtype=dt)
        q, r = q + db[xs], r + db[us]
    Qi = np.where(mx, dt(0), o.gauss_jordan_inverse(np.where(mx, eye(S), Qw)))
    Ri = np.where(mu, dt(0), o.gauss_jordan_inverse(np.where(mu, eye(C), Rw)))
    # g' and c': the kernel's fma chains are sums of a few products; numpy's matrix products in dt stand for them
    qp = np.where(onx, dt(0), q - np.einsum("kij,kj->ki", Q, bx))
    rp = np.where(onu, dt(0), r - np.einsum("kij,kj->ki", R, bu))
    cp = c - bx
    cp[1:] -= np.einsum("kij,kj->ki", A, bx[:-1]) + np.einsum("kij,kj->ki", B, bu)
    gp = ref.dz_layout(qp, rp, S, C, K).astype(dt)
    Gd, Cd = o.pack_G(Q, R), kgr.pack_C(A, B).astype(dt)
    S_bd, P_bd, gam, Ginv = o.form_schur(Gd, Cd, gp, cp.reshape(-1), S, C, K, inverses=(Qi, Ri))
    P_bd = o.form_ss(S_bd, P_bd, S, K)
    lam, iters = o.pcg(S_bd, P_bd, gam, S, K, exit_tol, max_iters)
    dz = o.compute_dz(Ginv, Cd, gp, lam, S, C, K)
    return np.where(on, b, dz), lam, iters


PROBLEMS = ("pendulum", "double_integrator", "6_3_20", "14_7_50")
# ADMM iterations (eps_abs = eps_rel = 0) after which the rule gives the exact active set, with margin over the first one
EXACT_FROM = dict(pendulum=50, double_integrator=2000, **{"6_3_20": 2000, "14_7_50": 100})


def exact_active(name):
    """(act, H, C, g, c, lo, hi) of a problem: the active set of its ADMM iterate after EXACT_FROM iterations."""
    s, lo, hi, arho = problem(name)
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, admm_rho=arho, eps_abs=0.0, eps_rel=0.0, max_admm_iters=EXACT_FROM[name])
    return active_set(out["z"], out["y"], lo, hi, s.S), H, Cm, g, c, lo, hi
