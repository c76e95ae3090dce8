"""numpy reference of the active-set iteration with capped (Huber) soft bounds, fp64.

The problem of box_qp_soft_ref with a cap m_i >= 0 (+inf: none) on the penalty force of every soft variable:

    min 1/2 x^T H x - g^T x + sum_i h_i(dist(x_i, [lo_i, hi_i]))   s.t.  C x = c,  lo_i <= x_i <= hi_i wherever w_i = 0,
    h_i(d) = (w_i / 2) d^2  while w_i d <= m_i,   m_i d - m_i^2 / (2 w_i)  beyond.

The force is clamp(w_i (x_i - clip(x_i)), -m_i, m_i).  act takes two more values: +-2 names a saturated variable (its sign the
sign of the force).  A saturated variable is free in the reduced system - no diagonal term, no shift - with g'_i = g_i - s m_i,
and its multiplier is y_i = s m_i.  pdas_huber() is the iteration of gato_box_qp_pdas_huber with exact reduced solves; with every
cap +inf it is box_qp_soft_ref.pdas_soft, operation for operation.  huber_grads() is the backward pass, huber_stage() the
restatement on the oracle's stages in a given dtype, and the seed walks keep only problems whose every decision has a margin no
rounding on the device can cross."""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import box_qp_soft_ref as SR                      # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402

CONVERGED, MAX_ITERS, NONFINITE = SR.CONVERGED, SR.MAX_ITERS, SR.NONFINITE
WEIGHT, CAP = SR.WEIGHT, 1.0                      # the weight and the cap of the walked problems' soft state bounds
F32_EXIT_TOL = SR.F32_EXIT_TOL


def sat_set(act):
    """The saturated variables: act = +-2."""
    return np.abs(np.asarray(act, np.int64)) == 2


def unsaturated(act):
    """act with the saturated variables free: the act whose quadratic reduced system the saturated one shares."""
    act = np.asarray(act, np.int8)
    return np.where(sat_set(act), 0, act).astype(np.int8)


def quad_set(act, w):
    """The soft quadratic-active variables: soft-active and not saturated."""
    return SR.soft_set(act, w) & ~sat_set(act)


def capped_set(w, m):
    """The variables whose next act the capped rule decides: a positive weight and a finite cap."""
    return (np.asarray(w) > 0) & np.isfinite(m)


def reduced_matrix(H, Cm, act, w):
    return SR.reduced_matrix(H, Cm, unsaturated(act), w)


def reduced_solve(H, Cm, g, c, lo, hi, w, m, act):
    """(x, y, lam) of the reduced solve on act: box_qp_soft_ref.reduced_solve with every saturated variable free, g_i - s m_i in
    its row of the right-hand side and y_i = s m_i.  Without a saturated variable: box_qp_soft_ref.reduced_solve itself."""
    act = np.asarray(act, np.int8)
    sat = sat_set(act)
    if not sat.any():
        return SR.reduced_solve(H, Cm, g, c, lo, hi, w, act)
    push = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), 0.0)
    x, y, lam = SR.reduced_solve(H, Cm, g - push, c, lo, hi, w, unsaturated(act))
    y = np.where(sat, push, y)
    return x, y, lam


def cap_excess(act, x, y, lo, hi, w, m):
    """What the acceptance test adds per variable: max(|y| - m, 0) on the soft quadratic-active set, max(m - s w (x - b), 0) on
    the saturated one, 0 elsewhere."""
    act = np.asarray(act, np.int8)
    b = P.bound_values(act, lo, hi)
    sat, quad = sat_set(act), quad_set(act, w)
    out = np.zeros(len(x))
    with np.errstate(invalid="ignore"):
        out[quad] = np.maximum(np.abs(y) - m, 0.0)[quad]
        out[sat] = np.maximum(m - np.sign(act) * (w * (x - b)), 0.0)[sat]
    return out


def point(H, Cm, g, c, lo, hi, w, m, act, x, y, lam, eps_abs, eps_rel):
    """box_qp_soft_ref.point with the capped additions to the sign test: (z, rp, rd, finite, ok)."""
    z, rp, rd, finite, ok = SR.point(H, Cm, g, c, lo, hi, w, act, x, y, lam, eps_abs, eps_rel)
    if not ok:
        return z, rp, rd, finite, ok
    sd = ref.residuals(H, Cm, g, c, x, z, y, lam)[3]
    return z, rp, rd, finite, bool(cap_excess(act, x, y, lo, hi, w, m).max(initial=0.0) <= eps_abs + eps_rel * sd)


def next_act(act, x, y, lo, hi, w, m, S):
    """act' of the rule: box_qp_soft_ref.next_act, and for a soft variable with a finite cap, from x alone on the product f = w
    (x - hi): +2 where f > m, else +1 where x > hi; mirrored below lo; lo == hi: +2 where f > m, -2 where -f > m, else -1; 0 on
    the S states of x_0.  Exact comparisons."""
    new = SR.next_act(np.sign(np.asarray(act, np.int8)), x, y, lo, hi, w, S)
    cs = capped_set(w, m)
    with np.errstate(invalid="ignore"):
        fh, fl = w * (x - hi), w * (x - lo)
        rule = np.where(fh > m, 2, np.where(x > hi, 1, np.where(-fl > m, -2, np.where(x < lo, -1, 0))))
        rule = np.where(lo == hi, np.where(fh > m, 2, np.where(-fh > m, -2, -1)), rule)
    new[cs] = rule[cs]
    new[:S] = 0
    return new


def decision_margin(act, x, y, lo, hi, w, m, S):
    """box_qp_soft_ref.decision_margin, and for every soft variable with a finite cap (off x_0) the distance | |x - b| - m / w | to
    the switching point of either finite bound b, where the force meets the cap."""
    mar = SR.decision_margin(np.sign(np.asarray(act, np.int8)), x, y, lo, hi, w, S)
    cs = capped_set(w, m) & (np.arange(len(x)) >= S)
    if cs.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(cs, m / np.where(cs, w, 1.0), 0.0)
            d = np.minimum(np.where(np.isfinite(hi), np.abs(np.abs(x - hi) - r), np.inf),
                           np.where(np.isfinite(lo), np.abs(np.abs(x - lo) - r), np.inf))
        mar = min(mar, float(d[cs].min()))
    return mar


def pdas_huber(H, Cm, g, c, lo, hi, w, m, S, act0=None, eps_abs=1e-6, eps_rel=1e-6, max_pdas_iters=30):
    """The iteration of gato_box_qp_pdas_huber with exact reduced solves: box_qp_soft_ref.pdas_soft's dict."""
    N = len(g)
    w = np.broadcast_to(np.asarray(w, np.float64), (N,))
    m = np.broadcast_to(np.asarray(m, np.float64), (N,))
    act = np.zeros(N, np.int8) if act0 is None else np.asarray(act0, np.int8).copy()
    trace = []
    status = MAX_ITERS
    for it in range(1, max_pdas_iters + 1):
        x, y, lam = reduced_solve(H, Cm, g, c, lo, hi, w, m, act)
        z, rp, rd, finite, ok = point(H, Cm, g, c, lo, hi, w, m, act, x, y, lam, eps_abs, eps_rel)
        if not finite:
            trace.append(dict(act=act.copy(), changed=None, margin=np.nan))
            status = NONFINITE
            break
        margin = decision_margin(act, x, y, lo, hi, w, m, S)
        if ok:
            trace.append(dict(act=act.copy(), changed=None, margin=margin))
            status = CONVERGED
            break
        new = next_act(act, x, y, lo, hi, w, m, S)
        changed = int((new != act).sum())
        trace.append(dict(act=act.copy(), changed=changed, margin=margin))
        if changed == 0 or it == max_pdas_iters:
            break
        act = new
    return dict(status=status, iters=it, act=act, trace=trace, x=x, z=z, y=y, lam=lam, res_prim=rp, res_dual=rd)


def huber(w, m, d):
    """h(d) per variable for distances d >= 0 (0 where w = 0)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lin = m * d - m * m / (2.0 * np.where(w > 0, w, 1.0))
        return np.where(w > 0, np.where(w * d <= m, 0.5 * w * d * d, lin), 0.0)


def force(lo, hi, w, m, x):
    """clamp(w (x - clip(x)), -m, m) on the soft variables, 0 on the hard ones."""
    return np.where(w > 0, np.clip(w * (x - np.clip(x, lo, hi)), -m, m), 0.0)


def penalised_objective(H, g, lo, hi, w, m, x):
    """1/2 x^T H x - g^T x + sum h_i(dist(x_i, [lo_i, hi_i])) and its gradient."""
    d = np.abs(x - np.clip(x, lo, hi))
    return float(0.5 * x @ (H @ x) - g @ x + huber(w, m, d).sum()), H @ x - g + force(lo, hi, w, m, x)


def kkt_residuals(H, Cm, g, c, lo, hi, w, m, x, y, lam):
    """Optimality of (x, y, lam) for the Huber-penalised problem, independent of the algorithm: box_qp_soft_ref.kkt_residuals
    with the force |y_i - clamp(w_i (x_i - clip(x_i)), -m_i, m_i)| on the soft variables."""
    x, y, lam = (np.asarray(v, np.float64) for v in (x, y, lam))
    out = SR.kkt_residuals(H, Cm, g, c, lo, hi, w, x, np.where(w > 0, w * (x - np.clip(x, lo, hi)), y), lam)
    out["stat"] = float(np.abs(H @ x - g + Cm.T @ lam + y).max())
    out["force"] = float(np.abs(np.where(w > 0, y - force(lo, hi, w, m, x), 0.0)).max())
    return out


# ---- gradients ---------------------------------------------------------------------------------------------------------------
def huber_grads(H, Cm, act, w, m, lo, hi, x, lam, xbar, lambar, S, C, K):
    """Gradients of L = xbar . x + lambar . lam through a converged point with respect to all fifteen inputs of
    box_qp_layer(x_soft=, u_soft=, x_soft_max=, u_soft_max=): box_qp_soft_ref.soft_grads on the act with the saturated variables
    free - they get 0 in lo, hi and w - plus m_bar_i = -s a_i on the saturated set (x_soft_max [K, S], u_soft_max [K-1, C], m)."""
    act = np.asarray(act, np.int8)
    out = SR.soft_grads(H, Cm, unsaturated(act), w, lo, hi, x, lam, xbar, lambar, S, C, K)
    m_bar = np.where(sat_set(act), -np.sign(act) * out["a"], 0.0)
    out["x_soft_max"], out["u_soft_max"] = P.split_states_controls(m_bar, S, C, K)
    out["m"] = m_bar
    return out


# ---- the iteration on the oracle's stages in a given dtype -------------------------------------------------------------------
def stage_solve(s, lo, hi, w, m, act, dtype, exit_tol=1e-8, max_iters=1000):
    """box_qp_soft_ref.stage_solve with the capped rule of polish_prepare_kernel: a saturated variable free, its g_i - s m_i
    formed in `dtype`."""
    dt = np.dtype(dtype).type
    act = np.asarray(act, np.int8)
    sat = sat_set(act)
    if sat.any():
        push = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), 0.0).astype(dt)
        s = dataclasses.replace(s, g=(np.asarray(s.g, dt) - push).astype(dt))
    return SR.stage_solve(s, lo, hi, w, unsaturated(act), dtype, exit_tol=exit_tol, max_iters=max_iters)


def next_act_in(dtype, act, x, y, lo, hi, w, m, S):
    """next_act with the products w (x - b) formed in `dtype` from the point rounded to it (what the device's step compares)."""
    dt = np.dtype(dtype).type
    new = SR.next_act(np.sign(np.asarray(act, np.int8)), x, y, lo, hi, w, S)
    cs = capped_set(w, m)
    xt, lt, ht, wt, mt = (np.asarray(v, dt) for v in (x, lo, hi, w, m))
    with np.errstate(invalid="ignore"):
        fh, fl = (wt * (xt - ht)).astype(dt), (wt * (xt - lt)).astype(dt)
        rule = np.where(fh > mt, 2, np.where(xt > ht, 1, np.where(-fl > mt, -2, np.where(xt < lt, -1, 0))))
        rule = np.where(lt == ht, np.where(fh > mt, 2, np.where(-fh > mt, -2, -1)), rule)
    new[cs] = rule[cs]
    new[:S] = 0
    return new


def huber_stage(s, lo, hi, w, m, dtype, eps, max_pdas_iters=30, exit_tol=1e-8, max_iters=1000, sooner=False):
    """box_qp_soft_ref.soft_stage with caps: every reduced solve through stage_solve in `dtype`, the residuals evaluated in fp64
    on its point, the capped rule's products in `dtype`.  sooner: every PCG stopped one iteration before its own exit.
    -> (status, acts)."""
    H, Cm, g, c = ref.parts(s)
    act = np.zeros(s.N, np.int8)
    acts = []
    for it in range(1, max_pdas_iters + 1):
        acts.append(act.copy())
        x, lam, iters = stage_solve(s, lo, hi, w, m, act, dtype, exit_tol=exit_tol, max_iters=max_iters)
        if sooner and iters >= 1:
            x, lam, _ = stage_solve(s, lo, hi, w, m, act, dtype, exit_tol=exit_tol, max_iters=iters)
        x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
        if not (np.isfinite(x).all() and np.isfinite(lam).all()):
            return NONFINITE, acts
        soft, sat = SR.soft_set(act, w), sat_set(act)
        b = P.bound_values(act, lo, hi)
        y = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), np.where(soft, w * (x - b), np.where(act != 0, g - H @ x - Cm.T @ lam, 0.0)))
        _, _, _, finite, ok = point(H, Cm, g, c, lo, hi, w, m, act, x, y, lam, eps, eps)
        if ok:
            return CONVERGED, acts
        new = next_act_in(dtype, act, x, y, lo, hi, w, m, s.S)
        if np.array_equal(new, act):
            return MAX_ITERS, acts
        act = new
    return MAX_ITERS, acts


def rounded(p):
    """The problem with every input rounded to fp32 (values held in fp64), the weights and the caps included."""
    return dict(SR.rounded(p), m=np.asarray(p["m"], np.float32).astype(np.float64))


def f32_ok(p):
    """The further seed condition of the fp32 cases: on the problem rounded to fp32 the fp32 restatement ends CONVERGED over the
    reference's act sequence, and again with every PCG stopped one iteration sooner."""
    q = rounded(p)
    want = [t["act"] for t in p["run"]["trace"]]
    for sooner in (False, True):
        status, acts = huber_stage(q["s"], q["lo"], q["hi"], q["w"], q["m"], np.float32, P.F32_EPS, exit_tol=F32_EXIT_TOL, sooner=sooner)
        if status != CONVERGED or len(acts) != len(want) or not all(np.array_equal(a, b) for a, b in zip(acts, want)):
            return False
    return True


# ---- walked problems -------------------------------------------------------------------------------------------------------
def huber_problem(S, C, K, seed, sparse=False, weight=WEIGHT, cap=CAP):
    """box_qp_soft_ref.soft_problem with the cap `cap` on every state.  -> (s, H, Cm, g, c, lo, hi, w, m)."""
    s, H, Cm, g, c, lo, hi, w = SR.soft_problem(S, C, K, seed, sparse=sparse, weight=weight)
    return s, H, Cm, g, c, lo, hi, w, np.where(w > 0, float(cap), np.inf)


def max_cond(run, H, Cm, w):
    return max(float(np.linalg.cond(reduced_matrix(H, Cm, t["act"], w))) for t in run["trace"])


def final_kinds(run, w, lo, hi):
    """(a saturated lo != hi variable, a soft quadratic-active lo != hi one) in the run's final act."""
    ne = lo != hi
    return bool((sat_set(run["act"]) & ne).any()), bool((quad_set(run["act"], w) & ne).any())


def walk_ok(run, lo, hi, w, H=None, Cm=None, both=True):
    """The seed rule on a reference run: CONVERGED within WALK_SOLVES solves, every margin at least MARGIN, every reduced matrix
    (dense sizes) with cond <= COND_CAP, and the final act holds a saturated lo != hi variable (both: and a soft
    quadratic-active one)."""
    if not (run["status"] == CONVERGED and run["iters"] <= D.WALK_SOLVES and D.min_margin(run) >= D.MARGIN):
        return False
    sat, quad = final_kinds(run, w, lo, hi)
    if not sat or (both and not quad):
        return False
    return H is None or ref.is_sparse(H) or max_cond(run, H, Cm, w) <= P.COND_CAP


# the (shape, K) cells whose walk may find no seed (at K = 2 and 3 the two smallest shapes hold too few bounded states for a
# saturated variable under this rule): a test on one of them says so by name; every other cell must have a seed
MAY_BE_EMPTY = {(2, 1, 2), (2, 1, 3), (4, 2, 2), (4, 2, 3)}
_HUBER = {}


def huber_box(S, C, K, f32=False, count=1):
    """The first `count` problems huber_problem(S, C, K, seed) of seeds 0, 1, ... < WALK_SEEDS whose cold reference run meets
    walk_ok (both kinds at K >= 9 and from 6/3 up; f32: with eps = F32_EPS, and f32_ok), as box_qp_pdas_ref.as_problem dicts with
    "w", "m" and the run under "run"."""
    got = _HUBER.setdefault((S, C, K, f32), dict(next=0, found=[]))
    eps = P.F32_EPS if f32 else 1e-6
    while len(got["found"]) < count and got["next"] < D.WALK_SEEDS:
        seed = got["next"]
        got["next"] += 1
        s, H, Cm, g, c, lo, hi, w, m = huber_problem(S, C, K, seed)
        run = pdas_huber(H, Cm, g, c, lo, hi, w, m, S, eps_abs=eps, eps_rel=eps, max_pdas_iters=D.WALK_SOLVES)
        if not walk_ok(run, lo, hi, w, H, Cm, both=(S, C, K) not in MAY_BE_EMPTY):
            continue
        p = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, seed), w=w, m=m)
        if f32 and not f32_ok(p):
            continue
        got["found"].append(p)
    return got["found"][:count]


_LONG = {}
LONG_WEIGHT, LONG_CAP = 10.0, 0.3


def huber_long():
    """huber_problem at box_qp_pdas_ref.LONG (2/1/8197), sparse, with LONG_WEIGHT and LONG_CAP - at weight 100 and cap 1 the
    undamped iteration cycles over 8197 knots (about 100 entries change per solve, seeds 0 .. 3) - of the first seed whose cold
    reference run converges on an act with a saturated variable among the knots >= 8192, with that run (only its final act and
    point are used)."""
    if "p" not in _LONG:
        S, C, K = D.LONG
        for seed in range(D.WALK_SEEDS):
            s, H, Cm, g, c, lo, hi, w, m = huber_problem(S, C, K, seed, sparse=True, weight=LONG_WEIGHT, cap=LONG_CAP)
            run = pdas_huber(H, Cm, g, c, lo, hi, w, m, S, max_pdas_iters=D.WALK_SOLVES)
            if run["status"] == CONVERGED and (np.flatnonzero(sat_set(run["act"])) // (S + C) >= 8192).any():
                break
        _LONG["p"] = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, seed), w=w, m=m)
    return _LONG["p"]


# ---- mixed problems: a weight and a cap per variable, on states and controls ---------------------------------------------------
def mixed_caps(N, seed):
    """Per variable, independently: 10 ** uniform(-1, 1) or +inf with probability 1/2 each."""
    rng = np.random.default_rng([seed, 311, 1])
    return np.where(rng.random(N) < 0.5, 10.0 ** rng.uniform(-1.0, 1.0, N), np.inf)


def mixed_problem(S, C, K, seed):
    """box_qp_soft_ref.mixed_problem with mixed_caps.  -> (s, H, Cm, g, c, lo, hi, w, m)."""
    s, H, Cm, g, c, lo, hi, w = SR.mixed_problem(S, C, K, seed)
    return s, H, Cm, g, c, lo, hi, w, mixed_caps(s.N, seed)


_MIXED = {}


def mixed_box(S, C, K):
    """The first mixed_problem(S, C, K, seed), seed < 4 WALK_SEEDS, whose cold reference run converges within WALK_SOLVES solves
    with every margin at least MARGIN and cond <= COND_CAP and whose final act holds a saturated control with lo != hi; None if
    there is none."""
    if (S, C, K) not in _MIXED:
        _MIXED[(S, C, K)] = None
        n = S + C
        for seed in range(4 * D.WALK_SEEDS):
            s, H, Cm, g, c, lo, hi, w, m = mixed_problem(S, C, K, seed)
            run = pdas_huber(H, Cm, g, c, lo, hi, w, m, S, max_pdas_iters=D.WALK_SOLVES)
            if not (run["status"] == CONVERGED and D.min_margin(run) >= D.MARGIN):
                continue
            if not (sat_set(run["act"]) & (np.arange(s.N) % n >= S) & (lo != hi)).any():
                continue
            if max_cond(run, H, Cm, w) > P.COND_CAP:
                continue
            _MIXED[(S, C, K)] = dict(D.as_problem(s, H, Cm, g, c, lo, hi, run, seed), w=w, m=m)
            break
    return _MIXED[(S, C, K)]


SHAPES = SR.SHAPES
COLD_K = SR.COLD_K
F32_CASES = SR.F32_CASES
HUBER_KEYS = SR.SOFT_KEYS + ("x_soft_max", "u_soft_max")


def huber_math_arrays(p):
    """box_qp_soft_ref.soft_math_arrays plus x_soft_max [K, S] and u_soft_max [K-1, C], in HUBER_KEYS' order."""
    s = p["s"]
    return SR.soft_math_arrays(p) + [np.ascontiguousarray(t) for t in P.split_states_controls(p["m"], s.S, s.C, s.K)]
