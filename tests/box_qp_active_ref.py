"""numpy reference of the primal-dual active-set iteration for box QPs (DESIGN.md sections 3.9 to 3.11), fp64: one iteration
for hard, soft and capped (Huber) bounds.

The problem, per system, with H = G + rho I, weights w >= 0 and caps m >= 0 (+inf: none) in the dz layout:

    min 1/2 x^T H x - g^T x + sum_i h_i(dist(x_i, [lo_i, hi_i]))   s.t.  C x = c,  lo_i <= x_i <= hi_i wherever w_i = 0,
    h_i(d) = (w_i / 2) d^2  while w_i d <= m_i,   m_i d - m_i^2 / (2 w_i)  beyond.

w=None means all hard, m=None no caps.  From an active set act the reduced solve (box_qp_polish_ref.reduced_solve, which holds
the reduced system of all three forms) gives a point; if point() accepts it the iteration ends CONVERGED, otherwise next_act()
gives the next active set.  iterate() also records, per solve, the act it solved on, the count of changed entries and the
decision margin - how far the quantities the rule compares exactly are from their thresholds - and walk() with walk_ok() keeps
only problems whose every decision has a margin that no rounding on the device can cross and whose every reduced system is
well conditioned.  stage_iterate() restates the iteration on the oracle's stages in a given dtype, which is how an fp32 device
run is predicted.  H and C may be dense or scipy.sparse.  The problems the tests walk are in box_qp_pdas_ref (hard),
box_qp_soft_ref and box_qp_huber_ref."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402

CONVERGED, MAX_ITERS, NONFINITE = ref.CONVERGED, ref.MAX_ITERS, ref.NONFINITE
MARGIN = 1e-5                                     # the smallest decision margin a walked seed may show
WALK_SOLVES = 20                                  # the reference run of a walked seed converges within this many solves
WALK_SEEDS = 20
# The PCG exit tolerance of the fp32 cases, restatement and device alike.  All hard: 1e-8, the solver's own.  With weights:
# the PCG stops on eta = r . Pinv r, a squared norm, so the tolerance that matches the acceptance test's eps = F32_EPS = 1e-4 is
# eta = 1e-8: a PCG stopped there leaves |C x - c| at the test's own bar and the decision to the summation order (14/7/9 seed 0
# on the device: 3.8e-4 against a bar of 3.0e-4 on the reference's final act, where the restatement has 2.4e-5, and 1.7e-4 one
# iteration sooner).  One decade in the residual, two in eta, takes the solve's error out of the decision, which is what a case
# about the soft kernels must do.
HARD_F32_EXIT_TOL, F32_EXIT_TOL = 1e-8, 1e-10


def capped_set(w, m):
    """The variables whose next act the capped rule decides: a positive weight and a finite cap."""
    return (np.asarray(w) > 0) & np.isfinite(m)


def quad_set(act, w):
    """The soft quadratic-active variables: soft-active and not saturated."""
    return P.soft_set(act, w) & ~P.sat_set(act)


def cap_excess(act, x, y, lo, hi, w, m):
    """What the acceptance test adds per variable: max(|y| - m, 0) on the soft quadratic-active set, max(m - s w (x - b), 0) on
    the saturated one, 0 elsewhere."""
    act = np.asarray(act, np.int8)
    b = P.bound_values(act, lo, hi)
    sat, quad = P.sat_set(act), quad_set(act, w)
    out = np.zeros(len(x))
    with np.errstate(invalid="ignore"):
        out[quad] = np.maximum(np.abs(y) - m, 0.0)[quad]
        out[sat] = np.maximum(m - np.sign(act) * (w * (x - b)), 0.0)[sat]
    return out


def point(H, Cm, g, c, lo, hi, act, x, y, lam, eps_abs, eps_rel, w=None, m=None):
    """z, the residuals (H without the weights) and the acceptance test of the polish on a point, with the cap excess added to
    the sign test where caps are given: (z, rp, rd, finite, ok)."""
    z = np.where(P.soft_set(act, w), x, np.clip(x, lo, hi))
    with np.errstate(invalid="ignore"):
        rp, rd, sp, sd = ref.residuals(H, Cm, g, c, x, z, y, lam)
    if not all(np.isfinite(v).all() for v in (x, z, y, lam)) or not (np.isfinite(rp) and np.isfinite(rd)):
        return z, rp, rd, False, False
    tol_d = eps_abs + eps_rel * sd
    eq = lo == hi
    ok = rp <= eps_abs + eps_rel * sp and rd <= tol_d and np.all(y[(act > 0) & ~eq] >= -tol_d) and np.all(y[(act < 0) & ~eq] <= tol_d)
    if ok and m is not None:
        ok = cap_excess(act, x, y, lo, hi, w, m).max(initial=0.0) <= tol_d
    return z, rp, rd, True, bool(ok)


def next_act(act, x, y, lo, hi, S, w=None, m=None, dtype=None):
    """act' of the rule.  A hard variable: a free one becomes active on the side it left (x > hi: +1, x < lo: -1); an active one
    stays while its multiplier has the bound's sign (upper: y > 0, lower: y < 0) and is released otherwise.  A soft one is
    decided from x alone, whatever its act was (+1 where x > hi, -1 where x < lo, else 0), and with a finite cap on the product
    f = w (x - hi): +2 where f > m, else +1 where x > hi; mirrored below lo; lo == hi: +2 where f > m, -2 where -f > m, else -1.
    -1 wherever lo == hi otherwise, 0 on the S states of x_0.  Exact comparisons; an infinite bound can never become active.
    dtype: the capped rule's products formed in it from the point rounded to it (what the device's step compares)."""
    act = np.sign(np.asarray(act, np.int8))
    new = np.zeros(act.shape, np.int8)
    with np.errstate(invalid="ignore"):
        new[(act == 0) & (x > hi)] = 1
        new[(act == 0) & (x < lo)] = -1
        new[(act > 0) & (y > 0)] = 1
        new[(act < 0) & (y < 0)] = -1
        if w is not None:
            sv = np.asarray(w) > 0
            new[sv] = np.where(x > hi, 1, np.where(x < lo, -1, 0))[sv]
    new[lo == hi] = -1
    if m is not None:
        cs = capped_set(w, m)
        xt, lt, ht, wt, mt = (np.asarray(v, dtype or np.float64) for v in (x, lo, hi, w, m))
        with np.errstate(invalid="ignore"):
            fh, fl = (wt * (xt - ht)).astype(xt.dtype), (wt * (xt - lt)).astype(xt.dtype)
            rule = np.where(fh > mt, 2, np.where(xt > ht, 1, np.where(-fl > mt, -2, np.where(xt < lt, -1, 0))))
            rule = np.where(lt == ht, np.where(fh > mt, 2, np.where(-fh > mt, -2, -1)), rule)
        new[cs] = rule[cs]
    new[:S] = 0
    return new


def decision_margin(act, x, y, lo, hi, S, w=None, m=None):
    """How far the rule's exact comparisons are from a tie (inf if there is nothing to compare): the smallest distance of a
    bounded soft or free variable (off x_0, lo != hi) to either bound, the smallest |y| of a hard-active non-equality one, and
    for every soft variable with a finite cap (off x_0) the distance | |x - b| - m / w | to the switching point of either finite
    bound b, where the force meets the cap."""
    act = np.sign(np.asarray(act, np.int8))
    off0 = np.arange(len(act)) >= S
    eq = lo == hi
    sv = np.asarray(w) > 0 if w is not None else np.zeros(len(act), bool)
    by_x = ((act == 0) | sv) & off0 & ~eq & (np.isfinite(lo) | np.isfinite(hi))
    by_y = (act != 0) & ~sv & ~eq
    mar = np.inf
    if by_x.any():
        mar = min(mar, float(np.minimum(np.abs(x - lo), np.abs(hi - x))[by_x].min()))
    if by_y.any():
        mar = min(mar, float(np.abs(y[by_y]).min()))
    cs = capped_set(w, m) & off0 if m is not None else np.zeros(len(act), bool)
    if cs.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(cs, m / np.where(cs, w, 1.0), 0.0)
            d = np.minimum(np.where(np.isfinite(hi), np.abs(np.abs(x - hi) - r), np.inf),
                           np.where(np.isfinite(lo), np.abs(np.abs(x - lo) - r), np.inf))
        mar = min(mar, float(d[cs].min()))
    return mar


def iterate(H, Cm, g, c, lo, hi, S, w=None, m=None, act0=None, eps_abs=1e-6, eps_rel=1e-6, max_pdas_iters=30):
    """The iteration of gato_box_qp_pdas (_soft, _huber) with exact reduced solves.  -> dict status, iters (reduced solves), act
    (that of the last solve), x, z, y, lam, res_prim, res_dual (of the last solve's point; the device writes them only where
    CONVERGED) and trace: per solve a dict act, changed (None on the accepted solve), margin."""
    N = len(g)
    w, m = (v if v is None else np.broadcast_to(np.asarray(v, np.float64), (N,)) for v in (w, m))
    act = np.zeros(N, np.int8) if act0 is None else np.asarray(act0, np.int8).copy()
    trace = []
    status = MAX_ITERS
    for it in range(1, max_pdas_iters + 1):
        x, y, lam = P.reduced_solve(H, Cm, g, c, lo, hi, act, w, m)
        z, rp, rd, finite, ok = point(H, Cm, g, c, lo, hi, act, x, y, lam, eps_abs, eps_rel, w, m)
        if not finite:
            trace.append(dict(act=act.copy(), changed=None, margin=np.nan))
            status = NONFINITE
            break
        margin = decision_margin(act, x, y, lo, hi, S, w, m)
        if ok:
            trace.append(dict(act=act.copy(), changed=None, margin=margin))
            status = CONVERGED
            break
        new = next_act(act, x, y, lo, hi, S, w, m)
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


def _weights_and_caps(N, w, m):
    return np.zeros(N) if w is None else w, np.full(N, np.inf) if m is None else m


def penalised_objective(H, g, lo, hi, x, w=None, m=None):
    """1/2 x^T H x - g^T x + sum h_i(dist(x_i, [lo_i, hi_i])) and its gradient."""
    w, m = _weights_and_caps(len(x), w, m)
    d = np.abs(x - np.clip(x, lo, hi))
    return float(0.5 * x @ (H @ x) - g @ x + huber(w, m, d).sum()), H @ x - g + force(lo, hi, w, m, x)


def kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam, w=None, m=None):
    """Optimality of (x, y, lam) for the penalised problem, independent of the algorithm (infinity norms): stationarity H x - g
    + C^T lam + y, equality C x - c, violation of the hard bounds, the force |y_i - clamp(w_i (x_i - clip(x_i)), -m_i, m_i)| on
    the soft variables and box_qp_ref.qp_kkt_residuals' complementarity on the hard ones."""
    x, y, lam = (np.asarray(v, np.float64) for v in (x, y, lam))
    w, m = _weights_and_caps(len(x), w, m)
    sv = w > 0
    inf = np.full(len(x), np.inf)
    hard = ref.qp_kkt_residuals(H, Cm, g, c, np.where(sv, -inf, lo), np.where(sv, inf, hi), x, np.where(sv, 0.0, y), lam)
    return dict(stat=float(np.abs(H @ x - g + Cm.T @ lam + y).max()), eq=hard["eq"], bound=hard["bound"], comp=hard["comp"],
                force=float(np.abs(np.where(sv, y - force(lo, hi, w, m, x), 0.0)).max()))


# ---- the iteration on the oracle's stages in a given dtype -------------------------------------------------------------------
def stage_iterate(s, lo, hi, dtype, eps, w=None, m=None, max_pdas_iters=30, exit_tol=1e-8, max_iters=1000, sooner=False):
    """The iteration with every reduced solve through box_qp_polish_ref.reduced_stage_solve in `dtype`, the residuals and the
    rule evaluated in fp64 on its point, the capped rule's products in `dtype`.  sooner: every PCG stopped one iteration before
    its own exit.  -> (status, list of acts solved on)."""
    H, Cm, g, c = ref.parts(s)
    act = np.zeros(s.N, np.int8)
    acts = []
    for it in range(1, max_pdas_iters + 1):
        acts.append(act.copy())
        x, lam, iters = P.reduced_stage_solve(s, lo, hi, act, dtype, exit_tol, max_iters, w, m)
        if sooner and iters >= 1:
            x, lam, _ = P.reduced_stage_solve(s, lo, hi, act, dtype, exit_tol, iters, w, m)
        x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
        if not (np.isfinite(x).all() and np.isfinite(lam).all()):
            return NONFINITE, acts
        y = np.where(act != 0, g - H @ x - Cm.T @ lam, 0.0)
        if w is not None:
            y = np.where(P.soft_set(act, w), w * (x - P.bound_values(act, lo, hi)), y)
        if m is not None:
            sat = P.sat_set(act)
            y = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), y)
        if point(H, Cm, g, c, lo, hi, act, x, y, lam, eps, eps, w, m)[4]:
            return CONVERGED, acts
        new = next_act(act, x, y, lo, hi, s.S, w, m, dtype)
        if np.array_equal(new, act):
            return MAX_ITERS, acts
        act = new
    return MAX_ITERS, acts


def f32_ok(p):
    """The further seed condition of the fp32 cases (box_qp_polish_ref.f32_ok's pattern): on the problem rounded to fp32 the
    fp32 restatement ends CONVERGED over the reference's act sequence, and does so again with every PCG stopped one iteration
    sooner.  The PCG exit tolerance is the form's: HARD_F32_EXIT_TOL without weights, F32_EXIT_TOL with."""
    q = P.rounded(p)
    want = [t["act"] for t in p["run"]["trace"]]
    for sooner in (False, True):
        status, acts = stage_iterate(q["s"], q["lo"], q["hi"], np.float32, P.F32_EPS, q.get("w"), q.get("m"),
                                     exit_tol=F32_EXIT_TOL if "w" in q else HARD_F32_EXIT_TOL, sooner=sooner)
        if status != CONVERGED or len(acts) != len(want) or not all(np.array_equal(a, b) for a, b in zip(acts, want)):
            return False
    return True


# ---- the seed rule and the seed walk ---------------------------------------------------------------------------------------
def min_margin(run):
    return min(t["margin"] for t in run["trace"])


def max_cond(run, H, Cm, w=None):
    """The largest condition number among the reduced matrices the run solved (dense sizes)."""
    return max(float(np.linalg.cond(P.reduced_matrix(H, Cm, t["act"], w))) for t in run["trace"])


def walk_ok(run, H=None, Cm=None, w=None, also=None):
    """The seed rule on a reference run: CONVERGED within WALK_SOLVES solves, every decision margin at least MARGIN, also(run) -
    what the form asks of the acts - and - dense H and Cm given - every reduced matrix on the way with a condition number of at
    most box_qp_polish_ref.COND_CAP, the cap constructed() puts on the final one: a run can pass through an active set without
    LICQ (12/6/3 seed 0: cond 1e19 on its fourth solve) and still converge in exact arithmetic, but what the dense solve
    returns there is rounding, and no margin on it means anything."""
    if not (run["status"] == CONVERGED and run["iters"] <= WALK_SOLVES and min_margin(run) >= MARGIN):
        return False
    if also is not None and not also(run):
        return False
    return H is None or ref.is_sparse(H) or max_cond(run, H, Cm, w) <= P.COND_CAP


def as_problem(s, H, Cm, g, c, lo, hi, run, seed, **more):
    """The dict of box_qp_polish_ref.constructed_problem for a problem whose solution the reference run found, the run under
    "run"; more: "w", "m" and what else the form keeps."""
    return dict(s=s, H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, act=run["act"], x=run["x"], y=run["y"], lam=run["lam"], seed=seed, run=run, **more)


_WALKS = {}


def walk(key, make_problem, accept, count=1, limit=WALK_SEEDS):
    """The first `count` problems make_problem(seed) of seeds 0, 1, ... < limit that accept(p) keeps, as a list (fewer if the
    walk runs out).  Memoised under key and resumable: a later call with a larger count goes on from the seed the last one
    stopped at.  make_problem may return None for a seed it has no problem for."""
    got = _WALKS.setdefault(key, dict(next=0, found=[]))
    while len(got["found"]) < count and got["next"] < limit:
        p = make_problem(got["next"])
        got["next"] += 1
        if p is not None and accept(p):
            got["found"].append(p)
    return got["found"][:count]
