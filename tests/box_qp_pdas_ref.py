"""numpy reference of the primal-dual active-set iteration for box QPs, fp64: the polish of
box_qp_polish_ref iterated.  From an active set act the reduced solve gives a point; if it passes the polish's acceptance test
the iteration ends CONVERGED, otherwise next_act() gives the next active set.  H and C may be dense or scipy.sparse.  pdas()
also records, per solve, the act it solved on, the count of changed entries and the decision margin - how far the quantities
the rule compares exactly are from their thresholds - and the seed walks below keep only problems whose every decision has a
margin that no rounding on the device can cross and whose every reduced system is well conditioned.  pdas_stage() restates
the iteration on the oracle's stages in a given dtype (box_qp_polish_ref.reduced_stage_solve), which is how an fp32 device
run is predicted."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
from gato_python_amd import synth                 # noqa: E402

CONVERGED, MAX_ITERS, NONFINITE = ref.CONVERGED, ref.MAX_ITERS, ref.NONFINITE
MARGIN = 1e-5                                     # the smallest decision margin a walked seed may show
WALK_SOLVES = 20                                  # the reference run of a walked seed converges within this many solves
WALK_SEEDS = 20


def next_act(act, x, y, lo, hi, S):
    """act' of the rule: 0 on the S states of x_0, -1 where lo == hi; a free variable becomes active on the side it left
    (x > hi: +1, x < lo: -1); an active one stays while its multiplier has the bound's sign (upper: y > 0, lower: y < 0) and is
    released otherwise.  Exact comparisons; an infinite bound can never become active."""
    act = np.asarray(act)
    new = np.zeros(act.shape, np.int8)
    free = act == 0
    with np.errstate(invalid="ignore"):
        new[free & (x > hi)] = 1
        new[free & (x < lo)] = -1
        new[(act > 0) & (y > 0)] = 1
        new[(act < 0) & (y < 0)] = -1
    new[lo == hi] = -1
    new[:S] = 0
    return new


def decision_margin(act, x, y, lo, hi, S):
    """min over the free bounded variables off x_0 of their distance to either bound and over the active non-equality
    variables of |y|: the distance of the rule's comparisons from a tie (inf if there is nothing to compare)."""
    act = np.asarray(act)
    off0 = np.arange(len(act)) >= S
    eq = lo == hi
    fb = (act == 0) & off0 & ~eq & (np.isfinite(lo) | np.isfinite(hi))
    on = (act != 0) & ~eq
    m = np.inf
    if fb.any():
        m = min(m, float(np.minimum(np.abs(x - lo), np.abs(hi - x))[fb].min()))
    if on.any():
        m = min(m, float(np.abs(y[on]).min()))
    return m


def pdas(H, Cm, g, c, lo, hi, S, act0=None, eps_abs=1e-6, eps_rel=1e-6, max_pdas_iters=30):
    """The iteration of gato_box_qp_pdas with exact reduced solves.  -> dict status, iters (reduced solves), act (that of the
    last solve), x, z, y, lam, res_prim, res_dual (of the last solve's point; the device writes them only where CONVERGED)
    and trace: per solve a dict act, changed (None on the accepted solve), margin."""
    N = len(g)
    act = np.zeros(N, np.int8) if act0 is None else np.asarray(act0, np.int8).copy()
    trace = []
    status = MAX_ITERS
    for it in range(1, max_pdas_iters + 1):
        out = P.polish(H, Cm, g, c, lo, hi, None, None, S, eps_abs=eps_abs, eps_rel=eps_rel, act=act)
        if out["decision"] == P.NONFINITE:
            trace.append(dict(act=act.copy(), changed=None, margin=np.nan))
            status = NONFINITE
            break
        margin = decision_margin(act, out["x"], out["y"], lo, hi, S)
        if out["decision"] == P.ACCEPTED:
            trace.append(dict(act=act.copy(), changed=None, margin=margin))
            status = CONVERGED
            break
        new = next_act(act, out["x"], out["y"], lo, hi, S)
        changed = int((new != act).sum())
        trace.append(dict(act=act.copy(), changed=changed, margin=margin))
        if changed == 0 or it == max_pdas_iters:
            break
        act = new
    return dict(status=status, iters=it, act=act, trace=trace, **{k: out[k] for k in ("x", "z", "y", "lam", "res_prim", "res_dual")})


def min_margin(run):
    return min(t["margin"] for t in run["trace"])


def max_cond(run, H, Cm):
    """The largest condition number among the reduced matrices the run solved (dense sizes)."""
    return max(float(np.linalg.cond(P.reduced_matrix(H, Cm, t["act"]))) for t in run["trace"])


def walk_ok(run, H=None, Cm=None):
    """The seed rule on a reference run: CONVERGED within WALK_SOLVES solves, every decision margin at least MARGIN and - dense
    H and Cm given - every reduced matrix on the way with a condition number of at most box_qp_polish_ref.COND_CAP, the cap
    constructed() puts on the final one: a run can pass through an active set without LICQ (12/6/3 seed 0: cond 1e19 on its
    fourth solve) and still converge in exact arithmetic, but what the dense solve returns there is rounding, and no
    margin on it means anything."""
    if not (run["status"] == CONVERGED and run["iters"] <= WALK_SOLVES and min_margin(run) >= MARGIN):
        return False
    return H is None or ref.is_sparse(H) or max_cond(run, H, Cm) <= P.COND_CAP


# ---- the iteration on the oracle's stages in a given dtype -------------------------------------------------------------------
def pdas_stage(s, lo, hi, dtype, eps, max_pdas_iters=30, exit_tol=1e-8, max_iters=1000, sooner=False):
    """The iteration with every reduced solve through reduced_stage_solve in `dtype` (the residuals and the rule evaluated in
    fp64 on its point).  sooner: every PCG stopped one iteration before its own exit.  -> (status, list of acts solved on)."""
    H, Cm, g, c = ref.parts(s)
    S = s.S
    act = np.zeros(s.N, np.int8)
    acts = []
    for it in range(1, max_pdas_iters + 1):
        acts.append(act.copy())
        x, lam, iters = P.reduced_stage_solve(s, lo, hi, act, dtype, exit_tol=exit_tol, max_iters=max_iters)
        if sooner and iters >= 1:
            x, lam, _ = P.reduced_stage_solve(s, lo, hi, act, dtype, exit_tol=exit_tol, max_iters=iters)
        x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
        if not (np.isfinite(x).all() and np.isfinite(lam).all()):
            return NONFINITE, acts
        on, eq = act != 0, lo == hi
        y = np.where(on, g - H @ x - Cm.T @ lam, 0.0)
        rp, rd, sp, sd = ref.residuals(H, Cm, g, c, x, np.clip(x, lo, hi), y, lam)
        tol_d = eps + eps * sd
        sign_ok = np.all(y[(act > 0) & ~eq] >= -tol_d) and np.all(y[(act < 0) & ~eq] <= tol_d)
        if rp <= eps + eps * sp and rd <= tol_d and sign_ok:
            return CONVERGED, acts
        new = next_act(act, x, y, lo, hi, S)
        if np.array_equal(new, act):
            return MAX_ITERS, acts
        act = new
    return MAX_ITERS, acts


def f32_ok(p, run):
    """The further seed condition of the fp32 cases (box_qp_polish_ref.f32_ok's pattern): on the problem rounded to fp32 the
    fp32 restatement ends CONVERGED over the reference's act sequence, and does so again with every PCG stopped one iteration
    sooner."""
    q = P.rounded(p)
    want = [t["act"] for t in run["trace"]]
    for sooner in (False, True):
        status, acts = pdas_stage(q["s"], q["lo"], q["hi"], np.float32, P.F32_EPS, sooner=sooner)
        if status != CONVERGED or len(acts) != len(want) or not all(np.array_equal(a, b) for a, b in zip(acts, want)):
            return False
    return True


# ---- walked problems -------------------------------------------------------------------------------------------------------
def as_problem(s, H, Cm, g, c, lo, hi, run, seed):
    """The dict of box_qp_polish_ref.constructed_problem for a problem whose solution the reference run found."""
    return dict(s=s, H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, act=run["act"], x=run["x"], y=run["y"], lam=run["lam"], seed=seed, run=run)


_CONTROL, _CONSTRUCTED = {}, {}


def control_box(S, C, K, f32=False, count=1, sparse=False):
    """The first `count` control-only problems - synth.make_system(S, C, K, seed) with box_qp_polish_ref.boxes(s, seed + 1,
    eq = K >= 3, states=False) - of seeds 0, 1, ... < WALK_SEEDS whose cold reference run meets walk_ok (f32: with eps =
    F32_EPS, and f32_ok), as a list of problem dicts with the run under "run"."""
    key = (S, C, K, f32, sparse)
    got = _CONTROL.setdefault(key, dict(next=0, found=[]))
    eps = P.F32_EPS if f32 else 1e-6
    while len(got["found"]) < count and got["next"] < WALK_SEEDS:
        seed = got["next"]
        got["next"] += 1
        s = synth.make_system(S, C, K, seed=seed)
        if sparse:
            H, Cm, g, c = ref.sparse_parts(s)
            dz = ref.kkt_solver(H, Cm)(np.concatenate([g, c]))[:s.N]
        else:
            H, Cm, g, c = ref.parts(s)
            dz = None
        lo, hi = P.boxes(s, seed + 1, eq=K >= 3, states=False, dz=dz)
        run = pdas(H, Cm, g, c, lo, hi, S, eps_abs=eps, eps_rel=eps, max_pdas_iters=WALK_SOLVES)
        if not walk_ok(run, H, Cm):
            continue
        p = as_problem(s, H, Cm, g, c, lo, hi, run, seed)
        if f32 and not f32_ok(p, run):
            continue
        got["found"].append(p)
    return got["found"][:count]


def constructed_cold(S, C, K, count=1):
    """The first `count` problems of box_qp_polish_ref.constructed(S, C, K) (active states, dense Q and R, its own seed rule)
    whose cold reference run also meets walk_ok; each dict gains "run"."""
    got = _CONSTRUCTED.setdefault((S, C, K), dict(next=0, found=[]))
    while len(got["found"]) < count:
        ps = P.constructed(S, C, K, count=got["next"] + 1)
        if len(ps) <= got["next"]:
            break
        p = ps[got["next"]]
        got["next"] += 1
        run = pdas(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], S, max_pdas_iters=WALK_SOLVES)
        if walk_ok(run, p["H"], p["Cm"]):
            got["found"].append(dict(p, run=run))
    return got["found"][:count]


SHAPES = P.SWEEP_SHAPES
COLD_K = (2, 3, 9)                                # K of the cold control-only cases: 2, 3 and one K >= 9
CONSTRUCTED_K = (3, 9)
LONG = P.SWEEP_LONG                               # 2/1/8197: past the 8192-workgroup cap of the grid
BATCH = P.SWEEP_BATCH                             # 14/7/9, five systems


def named(name):
    """(s, H, C, g, c, lo, hi) of pendulum_box(0.2) ("pendulum") or box_qp_polish_ref.problem(name)."""
    s, lo, hi, _ = P.problem(name)
    return (s,) + tuple(ref.parts(s)) + (lo, hi)


# ---- the inputs of box_qp_layer as numpy arrays (tests/test_gpu_box_qp_layer_sweep.py) ---------------------------------------
KEYS = ("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi")


def math_arrays(s, lo, hi):
    """[Q, R, A, B, q, r, c, x_lo, x_hi, u_lo, u_hi] of a system and its box (dz layout) as box_qp takes them, in KEYS' order."""
    xl, ul = P.split_states_controls(lo, s.S, s.C, s.K)
    xh, uh = P.split_states_controls(hi, s.S, s.C, s.K)
    return [np.ascontiguousarray(t, np.float64) for t in (*kgr.blocks_of(s), xl, xh, ul, uh)]


def batched(arrays):
    """The per-system lists of math_arrays (or box_qp_soft_ref.soft_math_arrays) stacked along a leading batch dimension."""
    return [np.stack(ts) for ts in zip(*arrays)]


def sum_to(full, shape):
    """The gradient of an argument of `shape` that broadcasts to full's shape: full summed over the leading dimensions the
    argument lacks and over those where it has size 1."""
    full, shape = np.asarray(full, np.float64), tuple(shape)
    out = full.sum(axis=tuple(range(full.ndim - len(shape))))
    axes = tuple(i for i, n in enumerate(shape) if n == 1 and out.shape[i] != 1)
    return (out.sum(axis=axes, keepdims=True) if axes else out).reshape(shape)


def di_problem(**kw):
    """box_qp_ref.double_integrator(**kw) as a problem dict with its cold reference run (30 solves at most, the layer's default)."""
    s, lo, hi, _ = ref.double_integrator(**kw)
    H, Cm, g, c = ref.parts(s)
    return as_problem(s, H, Cm, g, c, lo, hi, pdas(H, Cm, g, c, lo, hi, s.S), None)


DI_TRIO = (dict(K=20, u_max=0.5, v_max=None), dict(K=20, u_max=0.5, v_max=0.57), dict(K=20, u_max=0.5, v_max=None, x0=(0.8, 0.3)))
_DI = {}


def di_trio():
    """Three 2/1/20 double integrators: bounded controls alone, the velocity-bounded one whose second reduced system is
    singular, bounded controls alone from another start."""
    if "hard" not in _DI:
        _DI["hard"] = [di_problem(**kw) for kw in DI_TRIO]
    return _DI["hard"]


def di_broadcast():
    """double_integrator(K=8, u_max=0.5, v_max=None): every bound one number (the 0-d bounds of the layer's broadcast test)."""
    if "k8" not in _DI:
        _DI["k8"] = di_problem(K=8, u_max=0.5, v_max=None)
    return _DI["k8"]
