"""numpy reference of the augmented-Lagrangian outer loop for hard bounds, fp64, over
box_qp_linesearch_ref.iterate_ls, plus a restatement whose reduced solves run on the oracle's stages in a given dtype.

For x in [lo, hi] the augmented Lagrangian with multiplier mu and weight w is the all-soft problem of section 3.12 on the bounds
shifted by -mu / w, and the multiplier update is that solve's penalty force y.  An ALM variable has a finite bound, no user weight
and is off the S states of x_0; a variable with a user weight keeps its soft bound (weight, cap, no multiplier, no shift).

    outer step k:  inner run on (lo - mu / w, hi - mu / w, weight w, no cap) from the act of the step before
                   v = max dist(x_i, [lo_i, hi_i]) over the ALM variables,  mu <- y there
                   accept iff v <= eps_abs + eps_rel |x|_inf;  else w <- growth w where v > v_prev / 4 and w < weight_max

refined_inner runs the same loop over a dense solve with iterative refinement: what an infeasible box, whose multiplier grows
without bound, needs for its stalled violation to be free of the solve's rounding.  PINNED lists, per cell, the seed the walk found, the form of its state box (boxes(states=True) as it is, widened around a feasible
trajectory, or that trajectory's tube) and the one margin the cell drops, if any; HARD_PINNED the same for the cells of
tests/box_qp_hard_cells.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_linesearch_ref as LS                # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
from gato_python_amd import synth                 # noqa: E402

CONVERGED, MAX_ITERS, NONFINITE = AS.CONVERGED, AS.MAX_ITERS, AS.NONFINITE
ACCEPT, GROW, KEEP, LAST, INNER = 0, 1, 2, 3, 4    # the decisions of a step (GATO_ALM_*)
WEIGHT, GROWTH, WEIGHT_MAX, OUTER, SOLVES = 100.0, 10.0, 1e8, 50, 30      # the defaults of box_qp(method="alm")


def alm_set(lo, hi, S, w=None):
    """The ALM variables: a finite bound, no user weight, off the states of x_0."""
    out = np.isfinite(lo) | np.isfinite(hi)
    if w is not None:
        out &= ~(np.asarray(w) > 0)
    out[:S] = False
    return out


def violation(x, lo, hi, av):
    return float(np.abs(x - np.clip(x, lo, hi))[av].max(initial=0.0))


def inner_inputs(lo, hi, av, w, m, mu, wk, dtype=np.float64):
    """(lo', hi', w', m') of an inner run, formed in `dtype`: shifted bounds and the weight wk on the ALM variables, the caller's
    elsewhere (w None: 0); m' is None without user caps, else +inf on the ALM variables."""
    dt = np.dtype(dtype).type
    lo, hi, mu = (np.asarray(t, dt) for t in (lo, hi, mu))
    wt = dt(wk)
    with np.errstate(invalid="ignore"):
        sh = np.where(av, mu / wt, dt(0)).astype(dt)
        lo2, hi2 = np.where(av, lo - sh, lo).astype(dt), np.where(av, hi - sh, hi).astype(dt)
    w2 = np.where(av, wt, dt(0) if w is None else np.asarray(w, dt)).astype(dt)
    m2 = None if (w is None or m is None) else np.where(av | ~(np.asarray(w) > 0), dt(np.inf), np.asarray(m, dt)).astype(dt)
    return lo2, hi2, w2, m2


def decide(v, xinf, wk, v_prev, eps_abs, eps_rel, growth, weight_max, last):
    """(decision, next weight) of a step whose inner run converged."""
    if v <= eps_abs + eps_rel * xinf:
        return ACCEPT, wk
    if last:
        return LAST, wk
    if v > 0.25 * v_prev and wk < weight_max:
        return GROW, growth * wk
    return KEEP, wk


def step_update(x, y, lo, hi, S, w, mu, wk, v_prev, eps_abs, eps_rel, growth=GROWTH, weight_max=WEIGHT_MAX, last=False, dtype=np.float64):
    """What the update and the decision give on a converged inner point held in `dtype`: dict v, xinf (doubles of the values in
    `dtype`), dec, mu (y on the ALM variables), w (the next weight, a double) and, unless the step stops, lo2, hi2, w2."""
    dt = np.dtype(dtype).type
    x, y, lo, hi, mu = (np.asarray(t, dt) for t in (x, y, lo, hi, mu))
    av = alm_set(lo, hi, S, w)
    v = float(np.abs((x - np.clip(x, lo, hi)).astype(dt))[av].max(initial=0.0))
    xinf = float(np.abs(x).max())
    mu = np.where(av, y, mu).astype(dt)
    dec, wn = decide(v, xinf, wk, v_prev, eps_abs, eps_rel, growth, weight_max, last)
    out = dict(v=v, xinf=xinf, dec=dec, mu=mu, w=wn, alm=av)
    if dec in (GROW, KEEP):
        out["lo2"], out["hi2"], out["w2"], _ = inner_inputs(lo, hi, av, w, None, mu, wn, dtype)
    return out


def iterate_alm(H, Cm, g, c, lo, hi, S, w=None, m=None, act0=None, mu0=None, eps_abs=1e-6, eps_rel=1e-6, alm_weight=WEIGHT,
                alm_growth=GROWTH, alm_weight_max=WEIGHT_MAX, max_alm_iters=OUTER, max_pdas_iters=SOLVES, inner=None):
    """The outer loop with exact inner runs (iterate_ls; inner: another callable of the same arguments).  -> dict status, outer,
    iters (reduced solves over all steps), weight (of the last step), x, z, y, lam, act, res_prim, res_dual (of the last inner
    point: the device writes x, z, y, lam, res_dual only where CONVERGED) and steps: per outer step a dict v, w, dec, solves, act
    (the act the inner run ended on), run (the inner run) and lo2, hi2, w2, m2 (its inputs)."""
    N = len(g)
    w, m = (t if t is None else np.broadcast_to(np.asarray(t, np.float64), (N,)) for t in (w, m))
    av = alm_set(lo, hi, S, w)
    mu = np.zeros(N) if mu0 is None else np.where(av, np.asarray(mu0, np.float64), 0.0)
    act = np.zeros(N, np.int8) if act0 is None else np.asarray(act0, np.int8).copy()
    inner = LS.iterate_ls if inner is None else inner
    wk, v_prev, steps, total, status = float(alm_weight), np.inf, [], 0, MAX_ITERS
    x = z = y = lam = None
    v = rd = np.nan
    for k in range(1, max_alm_iters + 1):
        lo2, hi2, w2, m2 = inner_inputs(lo, hi, av, w, m, mu, wk)
        run = inner(H, Cm, g, c, lo2, hi2, S, w2, m2, act0=act, eps_abs=eps_abs, eps_rel=eps_rel, max_pdas_iters=max_pdas_iters)
        total += run["iters"]
        act = run["act"]
        step = dict(v=np.nan, w=wk, dec=INNER, solves=run["iters"], act=act.copy(), run=run, lo2=lo2, hi2=hi2, w2=w2, m2=m2)
        steps.append(step)
        if run["status"] != CONVERGED:
            status = run["status"]
            break
        x, y, lam, rd = run["x"], run["y"], run["lam"], run["res_dual"]
        v = violation(x, lo, hi, av)
        mu = np.where(av, y, mu)
        dec, wn = decide(v, float(np.abs(x).max()), wk, v_prev, eps_abs, eps_rel, alm_growth, alm_weight_max, k == max_alm_iters)
        step.update(v=v, dec=dec)
        if dec == ACCEPT:
            status = CONVERGED
            break
        if dec == LAST:
            break
        wk, v_prev = wn, v
    if x is not None:
        z = np.where(av, np.clip(x, lo, hi), run["z"] if run["status"] == CONVERGED else x)
    rp = v if x is None else max(v, float(np.abs(Cm @ x - c).max()))
    return dict(status=status, outer=k, iters=total, weight=wk, x=x, z=z, y=y, lam=lam, act=act, res_prim=rp, res_dual=rd, steps=steps,
                mu=mu)


def loop_inner(solve, dtype=np.float64):
    """An inner run for iterate_alm over solve(H, Cm, g, c, lo, hi, act, w, m) -> (x, lam): the loop of
    box_qp_linesearch_ref.iterate_ls / stage_iterate_ls from a start act - the search in fp64 on the solve's point, xc kept in
    `dtype`, the capped rule's products in `dtype`.  -> iterate_ls's dict without the trace, plus "used": how much of its bar
    the accepted solve uses (the larger of its two residuals over their tolerances)."""
    def run(H, Cm, g, c, lo, hi, S, w, m, act0, eps_abs, eps_rel, max_pdas_iters):
        wl = LS.off_x0(w, S)
        act = np.asarray(act0, np.int8).copy()
        xc, status, used, rd = None, MAX_ITERS, np.nan, np.nan
        for it in range(1, max_pdas_iters + 1):
            x, lam = (np.asarray(t, np.float64) for t in solve(H, Cm, g, c, lo, hi, act, w, m))
            y = np.where(P.soft_set(act, w), w * (x - P.bound_values(act, lo, hi)), 0.0)
            if m is not None:
                sat = P.sat_set(act)
                y = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), y)
            if not (np.isfinite(x).all() and np.isfinite(lam).all()):
                status = NONFINITE
                break
            z, rp, rd, _, ok = AS.point(H, Cm, g, c, lo, hi, act, x, y, lam, eps_abs, eps_rel, w, m)
            if ok:
                _, _, sp, sd = ref.residuals(H, Cm, g, c, x, z, y, lam)
                used = max(rp / (eps_abs + eps_rel * sp), rd / (eps_abs + eps_rel * sd))
                status = CONVERGED
                break
            alpha = 1.0 if xc is None else LS.exact_alpha(H, g, lo, hi, wl, m, xc, x)["alpha"]
            xc = x if alpha == 1.0 else np.asarray(xc + alpha * (x - xc), dtype).astype(np.float64)
            new = AS.next_act(act, xc, y, lo, hi, S, w, m, None if np.dtype(dtype) == np.float64 else dtype)
            if np.array_equal(new, act) or it == max_pdas_iters:
                break
            act = new
        return dict(status=status, iters=it, act=act, x=x, y=y, lam=lam, z=x, res_dual=rd, trace=[], used=used)
    return run


def stage_inner(s, dtype, exit_tol=AS.F32_EXIT_TOL, max_iters=1000, sooner=False):
    """loop_inner whose reduced solves are box_qp_polish_ref.reduced_stage_solve in `dtype` on the oracle's stages (sooner: every
    PCG stopped one iteration before its own exit)."""
    def solve(H, Cm, g, c, lo, hi, act, w, m):
        x, lam, iters = P.reduced_stage_solve(s, lo, hi, act, dtype, exit_tol, max_iters, w, m)
        if sooner and iters >= 1:
            x, lam, _ = P.reduced_stage_solve(s, lo, hi, act, dtype, exit_tol, iters, w, m)
        return x, lam
    return loop_inner(solve, dtype)


def refined_solve(H, Cm, g, c, lo, hi, act, w=None, m=None):
    """box_qp_polish_ref.reduced_solve's system (dense) solved with two steps of iterative refinement, the residual and the
    right-hand side's products in extended precision.  -> (x, lam).  Why: the unrefined dense solve carries an absolute error in
    x of about eps cond |b'|, b' = b - mu / w the shifted bounds.  On a feasible problem mu stays bounded and that is far below
    every bar; on an infeasible one mu grows by w v per step, |b'| grows with the step count, and the stalled violation then
    drifts by a constant per step that is pure rounding (2/1/3 seed 1 at w = 1e8: -1.30e-9 per step, x_0 off its pinned value by
    1e-8; with refinement, and in 40-digit arithmetic, the violation repeats to the last bit)."""
    ld = np.longdouble
    act = np.asarray(act, np.int8)
    sat = P.sat_set(act)
    if sat.any():
        g, act = g - np.where(sat, np.sign(act) * np.where(sat, m, 0.0), 0.0), P.unsaturated(act)
    soft, hard = P.soft_set(act, w), P.hard_set(act, w)
    F, A = np.flatnonzero(~hard), np.flatnonzero(hard)
    b = P.bound_values(act, lo, hi)
    M = P.reduced_matrix(H, Cm, act, w)
    d = np.where(soft, w, 0.0) if soft.any() else np.zeros(len(g))
    bl, Hl, Cl = b.astype(ld), H.astype(ld), Cm.astype(ld)
    rhs = np.concatenate([(g.astype(ld) + d.astype(ld) * np.where(soft, bl, ld(0)))[F] - Hl[np.ix_(F, A)] @ bl[A],
                          c.astype(ld) - Cl[:, A] @ bl[A]])
    try:
        z = np.linalg.solve(M, rhs.astype(np.float64))
        for _ in range(2):
            z = z + np.linalg.solve(M, (rhs - M.astype(ld) @ z.astype(ld)).astype(np.float64))
    except np.linalg.LinAlgError:
        z = np.full(len(rhs), np.nan)
    x = np.zeros(len(g))
    x[A], x[F] = b[A], z[:len(F)]
    return x, z[len(F):]


refined_inner = loop_inner(refined_solve)


# How much of the acceptance bar an accepted inner solve of the fp32 restatement may use (its residuals over their tolerances).
# In fp32 the PCG leaves |C x - c| within a factor of two of the bar at eps = F32_EPS on the large shapes (32/16/3 seed 7: 0.9
# to 1.05 of it on every step), and another summation order then decides the solve - the device ended that seed MAX_ITERS on the
# last of the reference's 16 solves.  Stopping the PCG one iteration sooner does not show it: the floor is the same.
F32_ACCEPT_SLACK = 0.5


# ---- the problems --------------------------------------------------------------------------------------------------------------
def as_problem(s, lo, hi, seed=None, **more):
    H, Cm, g, c = ref.parts(s)
    return dict(s=s, H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, seed=seed, **more)


def named(name):
    """The three problems no earlier method solves: "di57" and "di60", double_integrator(v_max=0.57 / 0.6) (the second one is
    degenerate by construction), and "6_3_20", make_system(6, 3, 20, seed=2) with boxes(s, 3)."""
    if name in ("di57", "di60"):
        s, lo, hi, _ = ref.double_integrator(K=20, u_max=0.5, v_max=0.57 if name == "di57" else 0.6)
    else:
        s, lo, hi, _ = P.problem("6_3_20")
    return as_problem(s, lo, hi)


NAMED = ("di57", "di60", "6_3_20")


def rollout(s, lo, hi, shrink=1.0):
    """A feasible trajectory in the dz layout: the dynamics from x_0 under the unconstrained solution's controls clipped to the
    control box (shrink: to the box scaled by it about its centre)."""
    S, C, K, n = s.S, s.C, s.K, s.S + s.C
    _, Cm, _, c = ref.parts(s)
    dz, _ = synth.dense_kkt_solve(s)
    x = np.zeros(s.N)
    for k in range(K):
        r = slice(k * S, (k + 1) * S)
        xs = slice(k * n, k * n + S)
        # row block k of C x = c: x_k + (C x)_k's part on knot k-1 = c_k
        x[xs] = 0.0
        x[xs] = c[r] - Cm[r] @ x
        if k < K - 1:
            us = slice(k * n + S, (k + 1) * n)
            mid, half = 0.5 * (lo[us] + hi[us]), 0.5 * shrink * (hi[us] - lo[us])
            x[us] = np.clip(dz[us], mid - half, mid + half)
    return x


TUBE = 0.005                                      # half width of the state tube of the "tube" boxes


def widen_states(s, lo, hi, tube=False):
    """The state box widened around rollout(): lo <- min(lo, x^f - 0.05), hi <- max(hi, x^f + 0.05) on the bounded states.
    tube: the state box replaced by the tube x^f -+ TUBE instead, x^f rolled out with the controls clipped to half their box -
    feasible by that trajectory, also with every bound moved inward by 1e-3, and narrow enough that the optimum, whose controls
    want to leave the half box, leans on it (the cells of 2/1 with K <= 3, where neither boxes() nor its
    widened form has a seed with an active state bound among the first 20)."""
    n = s.S + s.C
    xf = rollout(s, lo, hi, 0.5 if tube else 1.0)
    idx = np.arange(s.N)
    st = ((idx % n) < s.S) & (np.isfinite(lo) | np.isfinite(hi)) & (lo != hi)
    lo, hi = lo.copy(), hi.copy()
    if tube:
        lo[st], hi[st] = (xf - TUBE)[st], (xf + TUBE)[st]
    else:
        lo[st], hi[st] = np.minimum(lo, xf - 0.05)[st], np.maximum(hi, xf + 0.05)[st]
    return lo, hi


def state_problem(S, C, K, seed, widen=False, system=synth.make_system):
    """system(S, C, K, seed) (synth.make_system, or a family of tests/box_qp_hard_cells.py) with box_qp_polish_ref.boxes(s, seed + 1, eq=K >= 3, states=True): bounds on the controls
    and on every other state; widen: widen_states on it ("tube": its tube form)."""
    s = system(S, C, K, seed)
    lo, hi = P.boxes(s, seed + 1, eq=K >= 3, states=True)
    if widen:
        lo, hi = widen_states(s, lo, hi, tube=widen == "tube")
    return as_problem(s, lo, hi, seed)


def feasible(p, inward=0.0):
    """scipy.optimize.linprog: C x = c has a point in the box (the bounds on x_0 dropped, as the solver does; every finite
    bound of a variable with lo < hi moved inward by `inward`)."""
    from scipy.optimize import linprog
    lo, hi = p["lo"].copy(), p["hi"].copy()
    S = p["s"].S
    lo[:S], hi[:S] = -np.inf, np.inf
    mv = lo < hi
    lo[mv], hi[mv] = (lo + inward)[mv], (hi - inward)[mv]
    if np.any(lo > hi):
        return False
    bounds = [(None if np.isinf(a) else a, None if np.isinf(b) else b) for a, b in zip(lo, hi)]
    out = linprog(np.zeros(len(lo)), A_eq=p["Cm"], b_eq=p["c"], bounds=bounds, method="highs")
    return out.status == 0


def run_alm(p, eps=1e-6, **kw):
    return iterate_alm(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], p["s"].S, p.get("w"), p.get("m"), eps_abs=eps, eps_rel=eps, **kw)


EXACT_EPS, EXACT_WEIGHT_MAX = 1e-10, 1e10


def exact(p):
    """x* of the hard QP: the reference run at eps = 1e-10 with alm_weight_max = 1e10, held to qp_kkt_residuals: stationarity
    and equality 1e-8, the bound violation within the run's own bar 1e-10 (1 + |x|_inf), complementarity within |y|_inf times that
    bar (a multiplier on a bound that is met to the bar).  -> the run; AssertionError if it is no KKT point."""
    run = run_alm(p, eps=EXACT_EPS, alm_weight_max=EXACT_WEIGHT_MAX, max_pdas_iters=60)
    assert run["status"] == CONVERGED, (p.get("seed"), run["status"], run["outer"])
    hard_lo, hard_hi = hard_box(p)
    k = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], hard_lo, hard_hi, run["x"], run["y"], run["lam"])
    bar = bar_of(run, EXACT_EPS)
    assert k["stat"] <= 1e-8 and k["eq"] <= 1e-8 and k["bound"] <= bar and k["comp"] <= bar * max(1.0, np.abs(run["y"]).max()), k
    return run


def hard_box(p):
    """The box the hard QP enforces: the caller's off x_0, none on x_0 and on user-soft variables."""
    av = alm_set(p["lo"], p["hi"], p["s"].S, p.get("w"))
    return np.where(av, p["lo"], -np.inf), np.where(av, p["hi"], np.inf)


# ---- the seed rule and the seed walk -------------------------------------------------------------------------------------------
WALK_OUTER, WALK_SOLVES = 15, 60
SHAPES = P.SWEEP_SHAPES
F64_CASES = [(S, C, K) for S, C in SHAPES for K in (2, 3, 9)]
F32_CASES = [(S, C, 3) for S, C in SHAPES]
FORMS = ("box", "wide", "tube")                    # boxes(states=True), widen_states on it, its tube form
# the one margin a cell may drop; feasibility and the active state never ("slack": fp32 only, F32_ACCEPT_SLACK)
DROPS = (None, "growth", "accept", "inner", "slack")


def bar_of(run, eps):
    return eps + eps * float(np.abs(run["x"]).max())


def inner_margins_ok(p, run):
    """Every inner run within section 3.12's margins: AS.MARGIN on xc and cond_cap(w) on its dense reduced matrices."""
    for st in run["steps"]:
        r = st["run"]
        if not r["trace"]:
            continue
        if not AS.min_margin(r) >= AS.MARGIN:
            return False
        if AS.max_cond(r, p["H"], p["Cm"], st["w2"]) > LS.cond_cap(st["w"]):
            return False
    return True


def seed_checks(p, run, eps):
    """The conditions of the seed rule on a reference run, by name (the later ones only where the earlier ones hold)."""
    S, n = p["s"].S, p["s"].S + p["s"].C
    out = dict(converged=run["status"] == CONVERGED and run["outer"] <= WALK_OUTER and run["iters"] <= WALK_SOLVES)
    if not out["converged"]:
        return out
    out["feasible"] = feasible(p) and feasible(p, 1e-3)
    if not out["feasible"]:
        return out
    idx = np.arange(len(p["g"]))
    state = ((idx % n) < S) & alm_set(p["lo"], p["hi"], S, p.get("w"))
    try:
        xs = exact(p)
    except AssertionError:                            # no x* to measure against: not a seed
        out["active_state"] = False
        return out
    p["exact"] = xs
    on = state & ((xs["x"] >= p["hi"] - 1e-9) | (xs["x"] <= p["lo"] + 1e-9))
    out["active_state"] = bool(np.any(on & (np.abs(xs["y"]) >= 1e-3)))
    vs = [st["v"] for st in run["steps"]]
    ratios = [vs[i] / vs[i - 1] for i in range(1, len(vs) - 1)]       # the decisions after the first step and before the accepted one
    out["growth"] = all(not (0.2 <= r <= 0.3) for r in ratios)
    bar = bar_of(run, eps)
    out["accept"] = vs[-1] <= 0.5 * bar and (len(vs) < 2 or vs[-2] >= 2 * bar)
    out["inner"] = out["active_state"] and inner_margins_ok(p, run)
    return out


def cell_problem(S, C, K, f32, seed, form, weight_max=None, system=synth.make_system):
    """state_problem(S, C, K, seed) in the form `form` with its reference run ("run"), eps ("eps") and seed_checks ("checks");
    f32: the problem rounded to fp32, eps = F32_EPS, alm_weight_max = weight_max (None: F32_WEIGHT_MAX)."""
    p = state_problem(S, C, K, seed, {"box": False, "wide": True, "tube": "tube"}[form], system)
    eps, kw = 1e-6, {}
    if f32:
        p, eps = rounded(p), P.F32_EPS
        kw = dict(alm_weight_max=F32_WEIGHT_MAX if weight_max is None else weight_max)
    p.update(run=run_alm(p, eps=eps, **kw), eps=eps, alm=kw, form=form)
    p["checks"] = seed_checks(p, p["run"], eps)
    return p


def meets(p, drop=None, f32=False):
    """The seed rule without the margin `drop`; f32: and f32_follows."""
    ck = p["checks"]
    if "inner" not in ck or not all(v for k, v in ck.items() if k != drop):
        return False
    return not f32 or f32_follows(p, slack=drop != "slack")


def walk_cell(S, C, K, f32=False, weight_max=None, system=synth.make_system):
    """The walk of a cell: the first seed < WALK_SEEDS that meets the rule on the plain box, else on the widened one, else on the
    tube; if none does, the same again with one margin dropped.  -> (seed, form, drop) or None.  Slow at the large shapes (minutes
    at 32/16/9): PINNED holds its results, and the tests check the pinned seed against the rule."""
    for drop in DROPS:
        for form in FORMS:
            for seed in range(AS.WALK_SEEDS):
                if meets(cell_problem(S, C, K, f32, seed, form, weight_max, system), drop, f32):
                    return seed, form, drop
    return None


_CELLS = {}


def alm_box(S, C, K, f32=False, system=synth.make_system, pinned=None):
    """The pinned problem of a cell (cell_problem of PINNED's seed and form, memoised) with "drop", the margin PINNED drops for it,
    or None where the walk found none.  system, pinned: another family of systems and its table (HARD_PINNED)."""
    cell = (S, C, K, bool(f32))
    if (cell, system) not in _CELLS:
        pin = (PINNED if pinned is None else pinned).get(cell)
        _CELLS[cell, system] = None if pin is None else dict(cell_problem(S, C, K, f32, pin[0], pin[1], system=system), drop=pin[2])
    return _CELLS[cell, system]


def rounded(p):
    """The problem with every input rounded to fp32 (values held in fp64)."""
    s = p["s"].astype(np.float32).astype(np.float64)
    s.rho = float(np.float32(p["s"].rho))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return as_problem(s, f32(p["lo"]), f32(p["hi"]), p["seed"])


def stage_run(p, eps, sooner=False, **kw):
    """run_alm with the reduced solves of the fp32 stage restatement."""
    return run_alm(p, eps=eps, inner=stage_inner(p["s"], np.float32, sooner=sooner), **kw)


def f32_follows(p, slack=True):
    """The fp32 stage restatement, and again with every PCG stopped one iteration sooner, ends CONVERGED over the reference's
    outer count, weights, solve counts and acts; every accepted inner solve of the first one within F32_ACCEPT_SLACK of its bar."""
    want = p["run"]
    for sooner in (False, True):
        got = stage_run(p, p["eps"], sooner, **p["alm"])
        if got["status"] != CONVERGED or got["outer"] != want["outer"]:
            return False
        for a, b in zip(got["steps"], want["steps"]):
            if a["w"] != b["w"] or a["solves"] != b["solves"] or not np.array_equal(a["act"], b["act"]):
                return False
            if slack and not sooner and not a["run"]["used"] <= F32_ACCEPT_SLACK:     # the run stopped sooner is itself the PCG's margin
                return False
    return True


# The fp32 default of alm_weight_max (DESIGN.md section 3.14 says how it was found): the fp32 walk has a seed in every cell at the
# caps 1e5 and 1e6 and loses 4/2/3 at 1e4; with the weight held at W from the first step the fp32 stage restatement of the six
# seeds converges on five at W = 1e5 (not 14/7/3), on one at 1e6 and on none from 1e7 on.
F32_WEIGHT_MAX = 1e5

# walk_cell's results: cell (S, C, K, f32) -> (seed, form, the margin dropped).  `python tests/box_qp_alm_ref.py` walks them again.
PINNED = {
    (2, 1, 2, False): (2, "tube", None),
    (2, 1, 3, False): (4, "tube", None),
    (2, 1, 9, False): (5, "box", None),
    (4, 2, 2, False): (1, "tube", None),
    (4, 2, 3, False): (18, "box", None),
    (4, 2, 9, False): (10, "box", None),
    (6, 3, 2, False): (3, "tube", None),
    (6, 3, 3, False): (14, "wide", None),
    (6, 3, 9, False): (8, "box", None),
    (12, 6, 2, False): (2, "box", None),
    (12, 6, 3, False): (16, "wide", "growth"),
    (12, 6, 9, False): (13, "wide", None),
    (14, 7, 2, False): (3, "box", None),
    (14, 7, 3, False): (17, "wide", None),
    (14, 7, 9, False): (10, "wide", None),
    (32, 16, 2, False): (15, "box", None),
    (32, 16, 3, False): (14, "wide", None),
    (32, 16, 9, False): (0, "box", "inner"),
    (2, 1, 3, True): (4, "tube", None),
    (4, 2, 3, True): (12, "box", "slack"),         # the cell's only seed: its last accepted solve uses 0.63 of the bar
    (6, 3, 3, True): (6, "box", "growth"),
    (12, 6, 3, True): (10, "box", "growth"),
    (14, 7, 3, True): (1, "wide", "growth"),
    (32, 16, 3, True): (16, "box", None),
}

# walk_cell's results on the hard family of tests/box_qp_hard_cells.py (asm_ref.hard_blocks at grade 4, fp64): dense graded Q_k and
# R_k under weights up to alm_weight_max.  tests/test_box_qp_hard_cpu.py checks each pinned seed against the rule.
HARD_PINNED = {
    (4, 2, 3, False): (6, "box", None),
    (6, 3, 9, False): (19, "wide", "growth"),
    (14, 7, 3, False): (4, "wide", None),
}


if __name__ == "__main__":
    import time
    f32 = "f32" in sys.argv[1:]
    wmax = [float(a) for a in sys.argv[1:] if a != "f32"] or [None]
    for wm in wmax:
        for S, C, K in (F32_CASES if f32 else F64_CASES):
            t = time.time()
            print("    (%d, %d, %d, %s): %r,    # weight_max %s, %.0f s" % (S, C, K, f32, walk_cell(S, C, K, f32, wm), wm, time.time() - t), flush=True)
