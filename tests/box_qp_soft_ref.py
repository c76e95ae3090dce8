"""numpy reference of the active-set iteration with soft bounds, fp64.

The problem, per system, with H = G + rho I and a weight vector w >= 0 in the dz layout:

    min 1/2 x^T H x - g^T x + sum_i (w_i / 2) dist(x_i, [lo_i, hi_i])^2   s.t.  C x = c,  lo_i <= x_i <= hi_i wherever w_i = 0.

w_i = 0 is the hard bound of box_qp_pdas_ref; w_i > 0 penalises the bound of variable i instead.  A soft variable outside its
bounds is active but stays in the reduced system: its diagonal entry gains w_i, g gains w_i b_i, and its multiplier is the
penalty force y_i = w_i (x_i - b_i).  pdas_soft() is the iteration of gato_box_qp_pdas_soft with exact reduced solves and
records per solve the act, the count of changed entries and the decision margin; with w = 0 it is box_qp_pdas_ref.pdas,
operation for operation.  soft_grads() is the backward pass; soft_stage() restates the iteration on the oracle's stages in a
given dtype (how an fp32 device run is predicted); the seed walks keep only problems whose every decision has a margin no
rounding on the device can cross.  H and C may be dense or scipy.sparse."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
from gato_python_amd import synth                 # noqa: E402

CONVERGED, MAX_ITERS, NONFINITE = ref.CONVERGED, ref.MAX_ITERS, ref.NONFINITE
WEIGHT = 100.0                                    # the weight of the walked problems' soft state bounds
# The PCG exit tolerance of the fp32 cases, restatement and device alike.  The PCG stops on eta = r . Pinv r, a squared norm, so
# the tolerance that matches the acceptance test's eps = F32_EPS = 1e-4 is eta = 1e-8: a PCG stopped there leaves |C x - c| at
# the test's own bar and the decision to the summation order (14/7/9 seed 0 on the device: 3.8e-4 against a bar of 3.0e-4 on the
# reference's final act, where the restatement has 2.4e-5, and 1.7e-4 one iteration sooner).  One decade in the residual, two
# in eta, takes the solve's error out of the decision, which is what a case about the soft kernels must do.
F32_EXIT_TOL = 1e-10


def soft_set(act, w):
    """The soft-active variables: active with a positive weight."""
    return (np.asarray(act) != 0) & (np.asarray(w) > 0)


def reduced_matrix(H, Cm, act, w):
    """The dense matrix of the reduced solve: the hard-active variables eliminated, w_i on the diagonal of the soft-active."""
    soft = soft_set(act, w)
    hard = (np.asarray(act) != 0) & ~soft
    M = P.reduced_matrix(H, Cm, hard.astype(np.int8))
    F = np.flatnonzero(~hard)
    M[np.arange(len(F)), np.arange(len(F))] += np.where(soft, w, 0.0)[F]
    return M


def reduced_solve(H, Cm, g, c, lo, hi, w, act):
    """(x, y, lam) of the reduced solve on act: x_i = b_i exactly and y_i = (g - H x - C^T lam)_i on the hard-active set, y_i =
    w_i (x_i - b_i) on the soft-active one, y = 0 elsewhere.  Without a soft-active variable: box_qp_polish_ref.reduced_solve."""
    act = np.asarray(act)
    soft = soft_set(act, w)
    if not soft.any():
        return P.reduced_solve(H, Cm, g, c, lo, hi, act)
    hard = (act != 0) & ~soft
    b = P.bound_values(act, lo, hi)
    d = np.where(soft, w, 0.0)
    A, F = np.flatnonzero(hard), np.flatnonzero(~hard)
    rhs = np.concatenate([g[F] + (d * b)[F] - P._sub(H, F, A) @ b[A], c - P._cols(Cm, A) @ b[A]])
    if ref.is_sparse(H):
        try:
            sol = ref.kkt_solver(P._sub(H, F, F), P._cols(Cm, F), diag=d[F])(rhs)
        except RuntimeError:
            sol = np.full(len(rhs), np.nan)
    else:
        try:
            sol = np.linalg.solve(reduced_matrix(H, Cm, act, w), rhs)
        except np.linalg.LinAlgError:
            sol = np.full(len(rhs), np.nan)
    x = np.zeros(len(g))
    x[A] = b[A]
    x[F] = sol[:len(F)]
    lam = sol[len(F):]
    y = np.zeros(len(g))
    y[A] = (g - H @ x - Cm.T @ lam)[A]
    y[soft] = (w * (x - b))[soft]
    return x, y, lam


def point(H, Cm, g, c, lo, hi, w, act, x, y, lam, eps_abs, eps_rel):
    """z, the residuals (H without the weights) and the acceptance test of the polish on a point: (z, rp, rd, finite, ok)."""
    soft = soft_set(act, w)
    z = np.where(soft, x, np.clip(x, lo, hi))
    with np.errstate(invalid="ignore"):
        rp, rd, sp, sd = ref.residuals(H, Cm, g, c, x, z, y, lam)
    if not all(np.isfinite(v).all() for v in (x, z, y, lam)) or not (np.isfinite(rp) and np.isfinite(rd)):
        return z, rp, rd, False, False
    tol_d = eps_abs + eps_rel * sd
    eq = lo == hi
    sign_ok = np.all(y[(act > 0) & ~eq] >= -tol_d) and np.all(y[(act < 0) & ~eq] <= tol_d)
    return z, rp, rd, True, bool(rp <= eps_abs + eps_rel * sp and rd <= tol_d and sign_ok)


def next_act(act, x, y, lo, hi, w, S):
    """act' of the rule: a hard variable follows box_qp_pdas_ref.next_act; a soft one is decided from x alone, whatever its
    act was (+1 where x > hi, -1 where x < lo, else 0); -1 wherever lo == hi, 0 on the S states of x_0.  Exact comparisons."""
    new = D.next_act(act, x, y, lo, hi, S)
    sv = np.asarray(w) > 0
    with np.errstate(invalid="ignore"):
        new[sv] = np.where(x > hi, 1, np.where(x < lo, -1, 0))[sv]
    new[lo == hi] = -1
    new[:S] = 0
    return new


def decision_margin(act, x, y, lo, hi, w, S):
    """The smallest distance of a bounded soft or free variable (off x_0, lo != hi) to either bound, and the smallest |y| of a
    hard-active non-equality one: how far the rule's exact comparisons are from a tie (inf if there is nothing to compare)."""
    act = np.asarray(act)
    off0 = np.arange(len(act)) >= S
    eq = lo == hi
    sv = np.asarray(w) > 0
    by_x = ((act == 0) | sv) & off0 & ~eq & (np.isfinite(lo) | np.isfinite(hi))
    by_y = (act != 0) & ~sv & ~eq
    m = np.inf
    if by_x.any():
        m = min(m, float(np.minimum(np.abs(x - lo), np.abs(hi - x))[by_x].min()))
    if by_y.any():
        m = min(m, float(np.abs(y[by_y]).min()))
    return m


def pdas_soft(H, Cm, g, c, lo, hi, w, S, act0=None, eps_abs=1e-6, eps_rel=1e-6, max_pdas_iters=30):
    """The iteration of gato_box_qp_pdas_soft with exact reduced solves: box_qp_pdas_ref.pdas's dict (status, iters, act, x, z,
    y, lam, res_prim, res_dual and trace: per solve act, changed - None on the accepted solve - and margin)."""
    N = len(g)
    w = np.broadcast_to(np.asarray(w, np.float64), (N,))
    act = np.zeros(N, np.int8) if act0 is None else np.asarray(act0, np.int8).copy()
    trace = []
    status = MAX_ITERS
    for it in range(1, max_pdas_iters + 1):
        x, y, lam = reduced_solve(H, Cm, g, c, lo, hi, w, act)
        z, rp, rd, finite, ok = point(H, Cm, g, c, lo, hi, w, act, x, y, lam, eps_abs, eps_rel)
        if not finite:
            trace.append(dict(act=act.copy(), changed=None, margin=np.nan))
            status = NONFINITE
            break
        margin = decision_margin(act, x, y, lo, hi, w, S)
        if ok:
            trace.append(dict(act=act.copy(), changed=None, margin=margin))
            status = CONVERGED
            break
        new = next_act(act, x, y, lo, hi, w, S)
        changed = int((new != act).sum())
        trace.append(dict(act=act.copy(), changed=changed, margin=margin))
        if changed == 0 or it == max_pdas_iters:
            break
        act = new
    return dict(status=status, iters=it, act=act, trace=trace, x=x, z=z, y=y, lam=lam, res_prim=rp, res_dual=rd)


def penalised_objective(H, g, lo, hi, w, x):
    """1/2 x^T H x - g^T x + sum (w_i / 2) dist(x_i, [lo_i, hi_i])^2 and its gradient."""
    d = np.where(w > 0, x - np.clip(x, lo, hi), 0.0)
    return float(0.5 * x @ (H @ x) - g @ x + 0.5 * (w * d * d).sum()), H @ x - g + w * d


def kkt_residuals(H, Cm, g, c, lo, hi, w, x, y, lam):
    """Optimality of (x, y, lam) for the penalised problem, independent of the algorithm (infinity norms): stationarity H x - g
    + C^T lam + y, equality C x - c, violation of the hard bounds, |y_i - w_i (x_i - clip(x_i))| on the soft variables and
    box_qp_ref.qp_kkt_residuals' complementarity on the hard ones."""
    x, y, lam = (np.asarray(v, np.float64) for v in (x, y, lam))
    sv = w > 0
    inf = np.full(len(x), np.inf)
    hard = ref.qp_kkt_residuals(H, Cm, g, c, np.where(sv, -inf, lo), np.where(sv, inf, hi), x, np.where(sv, 0.0, y), lam)
    force = np.where(sv, y - w * (x - np.clip(x, lo, hi)), 0.0)
    return dict(stat=float(np.abs(H @ x - g + Cm.T @ lam + y).max()), eq=hard["eq"], bound=hard["bound"], comp=hard["comp"],
                force=float(np.abs(force).max()))


# ---- gradients ---------------------------------------------------------------------------------------------------------------
def adjoint(H, Cm, act, w, xbar, lambar):
    """[a; beta] of the last assembly for upstream gradients (xbar, lambar): a = 0 on the hard-active set."""
    soft = soft_set(act, w)
    hard = (np.asarray(act) != 0) & ~soft
    F = np.flatnonzero(~hard)
    sol = np.linalg.solve(reduced_matrix(H, Cm, act, w), np.concatenate([np.asarray(xbar, np.float64)[F], lambar]))
    a = np.zeros(H.shape[0])
    a[F] = sol[:len(F)]
    return a, sol[len(F):]


def bound_grads(H, Cm, act, w, lo, hi, x, xbar, a, beta):
    """(lo_bar, hi_bar, w_bar) [N]: hard-active i: xbar_i - (H a + C^T beta)_i; soft-active i: w_i a_i, and w_bar_i = a_i (b_i -
    x_i); b_bar to hi for act = +1 and to lo for act = -1 (lo == hi: to lo); 0 elsewhere."""
    act = np.asarray(act)
    soft = soft_set(act, w)
    hard = (act != 0) & ~soft
    b = P.bound_values(act, lo, hi)
    bb = np.where(hard, np.asarray(xbar, np.float64) - (H @ a + Cm.T @ beta), np.where(soft, w * a, 0.0))
    return np.where(act < 0, bb, 0.0), np.where(act > 0, bb, 0.0), np.where(soft, a * (b - x), 0.0)


def soft_grads(H, Cm, act, w, lo, hi, x, lam, xbar, lambar, S, C, K):
    """Gradients of L = xbar . x + lambar . lam through a converged point with respect to all thirteen inputs of
    box_qp_layer(x_soft=, u_soft=): box_qp_polish_ref.grads's dict plus x_soft [K, S], u_soft [K-1, C] and w (dz layout)."""
    a, beta = adjoint(H, Cm, act, w, xbar, lambar)
    out = kgr.grads_math(x, lam, a, beta, S, C, K)
    lo_bar, hi_bar, w_bar = bound_grads(H, Cm, act, w, lo, hi, x, xbar, a, beta)
    out["x_lo"], out["u_lo"] = P.split_states_controls(lo_bar, S, C, K)
    out["x_hi"], out["u_hi"] = P.split_states_controls(hi_bar, S, C, K)
    out["x_soft"], out["u_soft"] = P.split_states_controls(w_bar, S, C, K)
    out.update(a=a, beta=beta, lo=lo_bar, hi=hi_bar, w=w_bar)
    return out


# ---- the iteration on the oracle's stages in a given dtype -------------------------------------------------------------------
def stage_solve(s, lo, hi, w, act, dtype, exit_tol=1e-8, max_iters=1000):
    """box_qp_polish_ref.reduced_stage_solve with the soft rule of soft_prepare_kernel: the identity rows and columns, the
    zeroing and the shifts over the hard-active set only; the diagonal of Q_k, R_k gains w_i and g' gains w_i b_i on the
    soft-active one.  -> (x, lam, pcg iterations)."""
    from oracle import gato_oracle as o
    dt = np.dtype(dtype).type
    S, C, K, n = s.S, s.C, s.K, s.S + s.C
    Q, R, A, B, q, r, c = (np.asarray(t, dt) for t in kgr.blocks_of(s))
    rho = dt(s.rho)
    Q = Q + rho * np.eye(S, dtype=dt)
    R = R + rho * np.eye(C, dtype=dt)
    act = np.asarray(act)
    soft = soft_set(act, w)
    on = (act != 0) & ~soft
    ball = P.bound_values(act, np.asarray(lo, dt), np.asarray(hi, dt)).astype(dt)
    b = np.where(on, ball, dt(0)).astype(dt)
    d = np.where(soft, np.asarray(w, dt), dt(0)).astype(dt)
    db = (d * np.where(soft, ball, dt(0))).astype(dt)
    xs, us = (np.arange(K)[:, None] * n + np.arange(S)), (np.arange(K - 1)[:, None] * n + S + np.arange(C))
    onx, onu, bx, bu = on[xs], on[us], b[xs], b[us]
    eye = lambda m: np.eye(m, dtype=dt)[None]
    mx, mu = onx[:, :, None] | onx[:, None, :], onu[:, :, None] | onu[:, None, :]
    Qw = Q + d[xs][:, :, None] * np.eye(S, dtype=dt)
    Rw = R + d[us][:, :, None] * np.eye(C, dtype=dt)
    Qi = np.where(mx, dt(0), o.gauss_jordan_inverse(np.where(mx, eye(S), Qw)))
    Ri = np.where(mu, dt(0), o.gauss_jordan_inverse(np.where(mu, eye(C), Rw)))
    qp = np.where(onx, dt(0), q + db[xs] - np.einsum("kij,kj->ki", Q, bx))
    rp = np.where(onu, dt(0), r + db[us] - np.einsum("kij,kj->ki", R, bu))
    cp = c - bx
    cp[1:] -= np.einsum("kij,kj->ki", A, bx[:-1]) + np.einsum("kij,kj->ki", B, bu)
    gp = ref.dz_layout(qp, rp, S, C, K).astype(dt)
    Gd, Cd = o.pack_G(Q, R), kgr.pack_C(A, B).astype(dt)
    S_bd, P_bd, gam, Ginv = o.form_schur(Gd, Cd, gp, cp.reshape(-1), S, C, K, inverses=(Qi, Ri))
    P_bd = o.form_ss(S_bd, P_bd, S, K)
    lam, iters = o.pcg(S_bd, P_bd, gam, S, K, exit_tol, max_iters)
    dz = o.compute_dz(Ginv, Cd, gp, lam, S, C, K)
    return np.where(on, b, dz), lam, iters


def soft_stage(s, lo, hi, w, dtype, eps, max_pdas_iters=30, exit_tol=1e-8, max_iters=1000, sooner=False):
    """box_qp_pdas_ref.pdas_stage with soft bounds: every reduced solve through stage_solve in `dtype`, the residuals and the
    rule evaluated in fp64 on its point.  sooner: every PCG stopped one iteration before its own exit.  -> (status, acts)."""
    H, Cm, g, c = ref.parts(s)
    act = np.zeros(s.N, np.int8)
    acts = []
    for it in range(1, max_pdas_iters + 1):
        acts.append(act.copy())
        x, lam, iters = stage_solve(s, lo, hi, w, act, dtype, exit_tol=exit_tol, max_iters=max_iters)
        if sooner and iters >= 1:
            x, lam, _ = stage_solve(s, lo, hi, w, act, dtype, exit_tol=exit_tol, max_iters=iters)
        x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
        if not (np.isfinite(x).all() and np.isfinite(lam).all()):
            return NONFINITE, acts
        soft = soft_set(act, w)
        b = P.bound_values(act, lo, hi)
        y = np.where(soft, w * (x - b), np.where(act != 0, g - H @ x - Cm.T @ lam, 0.0))
        _, _, _, finite, ok = point(H, Cm, g, c, lo, hi, w, act, x, y, lam, eps, eps)
        if ok:
            return CONVERGED, acts
        new = next_act(act, x, y, lo, hi, w, s.S)
        if np.array_equal(new, act):
            return MAX_ITERS, acts
        act = new
    return MAX_ITERS, acts


def f32_ok(p):
    """The further seed condition of the fp32 cases (box_qp_pdas_ref.f32_ok's pattern): on the problem rounded to fp32 the
    fp32 restatement ends CONVERGED over the reference's act sequence, and again with every PCG stopped one iteration sooner."""
    q = rounded(p)
    want = [t["act"] for t in p["run"]["trace"]]
    for sooner in (False, True):
        status, acts = soft_stage(q["s"], q["lo"], q["hi"], q["w"], np.float32, P.F32_EPS, exit_tol=F32_EXIT_TOL, sooner=sooner)
        if status != CONVERGED or len(acts) != len(want) or not all(np.array_equal(a, b) for a, b in zip(acts, want)):
            return False
    return True


def rounded(p):
    """The problem with every input rounded to fp32 (values held in fp64), the weights included."""
    q = P.rounded(dict(p, act=np.zeros_like(p["act"])))
    return dict(q, act=p["act"], w=np.asarray(p["w"], np.float32).astype(np.float64))


# ---- walked problems -------------------------------------------------------------------------------------------------------
def state_weights(s, weight=WEIGHT):
    """weight on every state (those of x_0 included: the device ignores them), 0 on every control."""
    n = s.S + s.C
    return np.where(np.arange(s.N) % n < s.S, float(weight), 0.0)


def soft_problem(S, C, K, seed, sparse=False, weight=WEIGHT):
    """synth.make_system(S, C, K, seed) with box_qp_polish_ref.boxes(s, seed + 1, eq = K >= 3, states=True), every state bound
    soft with `weight`, every control bound hard, and for K >= 3 one soft lo == hi (a tracking term, at a quarter of the
    unconstrained value) on the first state of the last knot.  -> (s, H, Cm, g, c, lo, hi, w)."""
    s = synth.make_system(S, C, K, seed=seed)
    if sparse:
        H, Cm, g, c = ref.sparse_parts(s)
        dz = ref.kkt_solver(H, Cm)(np.concatenate([g, c]))[:s.N]
    else:
        H, Cm, g, c = ref.parts(s)
        dz, _ = synth.dense_kkt_solve(s)
    lo, hi = P.boxes(s, seed + 1, eq=K >= 3, states=True, dz=dz)
    if K >= 3:
        j = (K - 1) * (S + C)
        lo[j] = hi[j] = 0.25 * dz[j]
    return s, H, Cm, g, c, lo, hi, state_weights(s, weight)


def max_cond(run, H, Cm, w):
    return max(float(np.linalg.cond(reduced_matrix(H, Cm, t["act"], w))) for t in run["trace"])


def walk_ok(run, lo, hi, w, H=None, Cm=None):
    """The seed rule on a reference run: box_qp_pdas_ref.walk_ok's (CONVERGED within WALK_SOLVES solves, every margin at
    least MARGIN, every reduced matrix - dense sizes - with cond <= COND_CAP), and a soft non-equality variable active on the way."""
    if not (run["status"] == CONVERGED and run["iters"] <= D.WALK_SOLVES and D.min_margin(run) >= D.MARGIN):
        return False
    if not any((soft_set(t["act"], w) & (lo != hi)).any() for t in run["trace"]):
        return False
    return H is None or ref.is_sparse(H) or max_cond(run, H, Cm, w) <= P.COND_CAP


_SOFT = {}


def soft_box(S, C, K, f32=False, count=1):
    """The first `count` problems soft_problem(S, C, K, seed) of seeds 0, 1, ... < WALK_SEEDS whose cold reference run meets
    walk_ok (f32: with eps = F32_EPS, and f32_ok), as box_qp_pdas_ref.as_problem dicts with "w" and the run under "run"."""
    got = _SOFT.setdefault((S, C, K, f32), dict(next=0, found=[]))
    eps = P.F32_EPS if f32 else 1e-6
    while len(got["found"]) < count and got["next"] < D.WALK_SEEDS:
        seed = got["next"]
        got["next"] += 1
        s, H, Cm, g, c, lo, hi, w = soft_problem(S, C, K, seed)
        run = pdas_soft(H, Cm, g, c, lo, hi, w, S, eps_abs=eps, eps_rel=eps, max_pdas_iters=D.WALK_SOLVES)
        if not walk_ok(run, lo, hi, w, H, Cm):
            continue
        p = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, seed), w=w)
        if f32 and not f32_ok(p):
            continue
        got["found"].append(p)
    return got["found"][:count]


_LONG = {}


def soft_long():
    """soft_problem at box_qp_pdas_ref.LONG (2/1/8197), seed 0, sparse, with its cold reference run (CONVERGED; its margins are
    below MARGIN, so only its final act and point are used)."""
    if "p" not in _LONG:
        S, C, K = D.LONG
        s, H, Cm, g, c, lo, hi, w = soft_problem(S, C, K, 0, sparse=True)
        run = pdas_soft(H, Cm, g, c, lo, hi, w, S, max_pdas_iters=D.WALK_SOLVES)
        _LONG["p"] = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, 0), w=w)
    return _LONG["p"]


# ---- mixed problems: hard and soft bounds side by side, on states and controls, a weight per variable -------------------------
def mixed_weights(N, seed):
    """Per variable, independently: soft with probability 1/2 and then w = 10 ** uniform(0, 3), else w = 0 (a hard bound)."""
    rng = np.random.default_rng([seed, 310])
    return np.where(rng.random(N) < 0.5, 10.0 ** rng.uniform(0.0, 3.0, N), 0.0)


def mixed_problem(S, C, K, seed, sparse=False, hard_states=True):
    """soft_problem's system, boxes and (K >= 3) lo == hi tracking state with mixed_weights: states and controls both draw, so
    both may be soft, and the tracking state may be hard.  hard_states=False: a state that drew 0 draws a weight of the same
    law instead - every state soft, each with its own weight; the controls as before.  -> (s, H, Cm, g, c, lo, hi, w)."""
    s, H, Cm, g, c, lo, hi, _ = soft_problem(S, C, K, seed, sparse=sparse)
    w = mixed_weights(s.N, seed)
    if not hard_states:
        rng = np.random.default_rng([seed, 311])
        state = np.arange(s.N) % (S + C) < S
        w = np.where(state & (w == 0), 10.0 ** rng.uniform(0.0, 3.0, s.N), w)
    return s, H, Cm, g, c, lo, hi, w


def cover(run, w, lo, hi, S, C, K):
    """What a run's trace exercises of the soft kernels' mixed branches, three booleans over the acts it solved on: (a) a
    soft-active control with lo != hi; (b) a knot whose states hold a hard-active and a soft-active variable in one act - a
    masked row next to an augmented diagonal entry in one Q_k; (c) the same among a knot's controls, in one R_k."""
    n = S + C
    idx = np.arange(len(w))
    knot, ctl = idx // n, idx % n >= S
    a = b = c = False
    for t in run["trace"]:
        sa = soft_set(t["act"], w)
        hard = (t["act"] != 0) & ~sa
        a |= bool((sa & ctl & (lo != hi)).any())
        for part in (~ctl, ctl):
            both = np.intersect1d(knot[sa & part], knot[hard & part]).size > 0
            if part is ctl:
                c |= both
            else:
                b |= both
    return a, b, c


def cover_need(S, C, K):
    """The part of cover() a walked mixed problem of the shape must meet: all of it, except that 2/1 has one control and, with
    boxes() bounding every other state, one bounded state per knot - no block of it can be mixed - and that 4/2/2 has two
    bounded states (K = 2: a single control knot, x_0 never active), which no seed below WALK_SEEDS mixes."""
    if S == 2:
        return True, False, False
    if (S, K) == (4, 2):
        return True, False, True
    return True, True, True


def covers(got, need):
    return all(g or not n for g, n in zip(got, need))


_MIXED = {}


def mixed_box(S, C, K, f32=False, count=1):
    """soft_box's seed walk over mixed_problem: the first `count` seeds < WALK_SEEDS whose cold reference run meets walk_ok (f32:
    with eps = F32_EPS, and f32_ok) and whose trace meets cover_need; each dict also holds its cover() under "cover"."""
    got = _MIXED.setdefault((S, C, K, f32), dict(next=0, found=[]))
    eps = P.F32_EPS if f32 else 1e-6
    need = cover_need(S, C, K)
    while len(got["found"]) < count and got["next"] < D.WALK_SEEDS:
        seed = got["next"]
        got["next"] += 1
        s, H, Cm, g, c, lo, hi, w = mixed_problem(S, C, K, seed)
        run = pdas_soft(H, Cm, g, c, lo, hi, w, S, eps_abs=eps, eps_rel=eps, max_pdas_iters=D.WALK_SOLVES)
        cov = cover(run, w, lo, hi, S, C, K)
        if not covers(cov, need) or not walk_ok(run, lo, hi, w, H, Cm):
            continue
        p = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, seed), w=w, cover=cov)
        if f32 and not f32_ok(p):
            continue
        got["found"].append(p)
    return got["found"][:count]


def mixed_layer_box(S, C, K):
    """The first problem of mixed_box(S, C, K) whose final act - the one the layer differentiates through - holds a soft-active
    control with lo != hi."""
    n = S + C
    for count in range(1, D.WALK_SEEDS + 1):
        ps = mixed_box(S, C, K, count=count)
        if len(ps) < count:
            break
        p = ps[-1]
        if (soft_set(p["run"]["act"], p["w"]) & (np.arange(len(p["w"])) % n >= S) & (p["lo"] != p["hi"])).any():
            return p
    return None


def mixed_long():
    """mixed_problem(hard_states=False) at box_qp_pdas_ref.LONG (2/1/8197), sparse, of the first seed whose cold reference run
    converges, with that run (as soft_long: only its final act and point are used).  Soft states, each with its own weight,
    and mixed controls: with hard state bounds drawn over 8197 knots some knot fixes both its state and its control, and the
    reference meets a singular reduced system on its second solve (seeds 0 .. 19, all NONFINITE)."""
    if "mixed" not in _LONG:
        S, C, K = D.LONG
        for seed in range(D.WALK_SEEDS):
            s, H, Cm, g, c, lo, hi, w = mixed_problem(S, C, K, seed, sparse=True, hard_states=False)
            run = pdas_soft(H, Cm, g, c, lo, hi, w, S, max_pdas_iters=D.WALK_SOLVES)
            if run["status"] == CONVERGED:
                break
        _LONG["mixed"] = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, seed), w=w)
    return _LONG["mixed"]


def weight_batch(seed):
    """Four weight vectors on one 14/7/9 system and box: mixed_problem(14, 7, 9, seed) with every state but the first of each
    knot freed (a hard box over half the states never converges at this shape, and one system here is all hard), and as
    weights its mixed ones, the same pattern times 10, all zero and state_weights; with each one's cold reference run.
    -> (problem tuple of mixed_problem, [w], [run])."""
    S, C, K = BATCH[:3]
    s, H, Cm, g, c, lo, hi, w = mixed_problem(S, C, K, seed)
    lane = np.arange(s.N) % (S + C)
    lo[(lane >= 1) & (lane < S)], hi[(lane >= 1) & (lane < S)] = -np.inf, np.inf
    ws = [w, 10.0 * w, np.zeros(s.N), state_weights(s)]
    runs = [pdas_soft(H, Cm, g, c, lo, hi, wi, S, max_pdas_iters=D.WALK_SOLVES) for wi in ws]
    return (s, H, Cm, g, c, lo, hi, w), ws, runs


def weight_batch_ok(prob, ws, runs):
    """The seed rule of weight_batch: every run meets box_qp_pdas_ref.walk_ok's status, solve count and margins, and its worst
    reduced matrix has cond / margin <= COND_CAP / MARGIN - the rounding a solve leaves in a decision, cond * eps, relative to
    the decision's margin is what the walks' two caps bound together, and the all-hard run here has cond 4e8 at a margin of
    9e-4 where the caps pair 1e8 with 1e-5; the mixed and the scaled run end on different points."""
    s, H, Cm = prob[:3]
    for wi, r in zip(ws, runs):
        if not D.walk_ok(r) or max_cond(r, H, Cm, wi) / D.min_margin(r) > P.COND_CAP / D.MARGIN:
            return False
    return bool(np.abs(runs[0]["x"] - runs[1]["x"]).max() > 1e-3)


_WBATCH = {}


def weight_batch_box():
    """weight_batch of the first seed < WALK_SEEDS that meets weight_batch_ok.  -> (seed, problem tuple, [w], [run])."""
    if "p" not in _WBATCH:
        for seed in range(D.WALK_SEEDS):
            got = weight_batch(seed)
            if weight_batch_ok(*got):
                _WBATCH["p"] = (seed,) + got
                break
    return _WBATCH.get("p")


def double_integrator_soft(weight=WEIGHT):
    """box_qp_ref.double_integrator(K=20, u_max=0.5, v_max=0.57), where the hard iteration meets a singular reduced system on
    its second solve, with the velocity bound soft: (s, H, Cm, g, c, lo, hi, w)."""
    s, lo, hi, _ = ref.double_integrator(K=20, u_max=0.5, v_max=0.57)
    return (s,) + tuple(ref.parts(s)) + (lo, hi, state_weights(s, weight))


SHAPES = D.SHAPES
COLD_K = D.COLD_K                                 # K of the cold fp64 cases
F32_CASES = [(S, C, 9) for S, C in SHAPES] + [(14, 7, 3), (32, 16, 3)]
GRAD_K = (2, 3)
LAYER_CASES = [(6, 3, 9), (14, 7, 3)]
MIXED_F32_K = 3                                   # K of the fp32 cases on mixed problems, one per shape
BATCH = D.BATCH


# ---- the cases of tests/test_gpu_box_qp_layer_sweep.py -----------------------------------------------------------------------------
SOFT_KEYS = D.KEYS + ("x_soft", "u_soft")
LAYER_BATCHES = ("control", "constructed", "soft", "mixed")      # the batches whose systems freeze at different solves
LAYER_SHAPE = (6, 3, 9)


def soft_math_arrays(p):
    """box_qp_pdas_ref.math_arrays of the problem plus x_soft [K, S] and u_soft [K-1, C] (zeros without "w"), in SOFT_KEYS' order."""
    s = p["s"]
    w = p["w"] if "w" in p else np.zeros(s.N)
    return D.math_arrays(s, p["lo"], p["hi"]) + [np.ascontiguousarray(t) for t in P.split_states_controls(w, s.S, s.C, s.K)]


def layer_batch(kind, count=5):
    """(problems, soft): the first `count` problems of one of LAYER_BATCHES; soft: they carry weights."""
    S, C, K = LAYER_SHAPE
    if kind == "control":
        return D.control_box(*D.BATCH[:3], count=count), False
    if kind == "constructed":
        return D.constructed_cold(S, C, K, count=count), False
    if kind == "soft":
        return soft_box(S, C, K, count=count), True
    if kind == "mixed":
        return mixed_box(S, C, K, count=count), True
    raise KeyError(kind)


def reference_grads(p, x, lam, xbar, lambar):
    """The gradients through problem p's reference act at the point (x, lam): soft_grads with p["w"], box_qp_polish_ref.grads
    without."""
    s = p["s"]
    if "w" in p:
        return soft_grads(p["H"], p["Cm"], p["run"]["act"], p["w"], p["lo"], p["hi"], x, lam, xbar, lambar, s.S, s.C, s.K)
    return P.grads(p["H"], p["Cm"], p["run"]["act"], x, lam, xbar, lambar, s.S, s.C, s.K)


def di_soft_problem(w, **kw):
    """box_qp_ref.double_integrator(**kw) with the weights w as a problem dict with its cold reference run."""
    s, lo, hi, _ = ref.double_integrator(**kw)
    H, Cm, g, c = ref.parts(s)
    w = np.broadcast_to(np.asarray(w, np.float64), (s.N,)).copy()
    return dict(D.as_problem(s, H, Cm, g, c, lo, hi, pdas_soft(H, Cm, g, c, lo, hi, w, s.S), None), w=w)


_DI = {}


def di_soft_trio():
    """box_qp_pdas_ref.di_trio with per-system weights: the velocity-bounded problem with WEIGHT on its states, the same with
    all weights 0 (it fails as the hard one does), the control-only one from the other start with weights 0."""
    if "trio" not in _DI:
        bad, other = D.DI_TRIO[1], D.DI_TRIO[2]
        s = ref.double_integrator(**bad)[0]
        _DI["trio"] = [di_soft_problem(state_weights(s), **bad), di_soft_problem(0.0, **bad), di_soft_problem(0.0, **other)]
    return _DI["trio"]


def di_soft_pair():
    """Two velocity-bounded 2/1/20 double integrators with WEIGHT on their states, from two starts: one box for both (the
    shared [K, S] bound of the layer's broadcast test)."""
    if "pair" not in _DI:
        s = ref.double_integrator(**D.DI_TRIO[1])[0]
        _DI["pair"] = [di_soft_problem(state_weights(s), **D.DI_TRIO[1]), di_soft_problem(state_weights(s), **dict(D.DI_TRIO[1], x0=(0.8, 0.3)))]
    return _DI["pair"]
