"""The soft-bound problems of the active-set iteration's tests (box_qp_active_ref): soft state boxes
over hard control boxes, mixed problems with a weight per variable on states and controls, the weight batch, the long
horizons, the double integrators with soft velocity bounds, and the case tables."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
from gato_python_amd import synth                 # noqa: E402

WEIGHT = 100.0                                    # the weight of the walked problems' soft state bounds


# ---- walked problems -------------------------------------------------------------------------------------------------------
def state_weights(s, weight=WEIGHT):
    """weight on every state (those of x_0 included: the device ignores them), 0 on every control."""
    n = s.S + s.C
    return np.where(np.arange(s.N) % n < s.S, float(weight), 0.0)


def soft_problem(S, C, K, seed, sparse=False, weight=WEIGHT, system=synth.make_system):
    """system(S, C, K, seed) (synth.make_system, or a family of tests/box_qp_hard_cells.py) with box_qp_polish_ref.boxes(s, seed + 1, eq = K >= 3, states=True), every state bound
    soft with `weight`, every control bound hard, and for K >= 3 one soft lo == hi (a tracking term, at a quarter of the
    unconstrained value) on the first state of the last knot.  -> (s, H, Cm, g, c, lo, hi, w)."""
    s = system(S, C, K, seed)
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


def soft_active_on_the_way(p):
    """A soft non-equality variable is active in some act of the run's trace."""
    return lambda run: any((P.soft_set(t["act"], p["w"]) & (p["lo"] != p["hi"])).any() for t in run["trace"])


def walked(make_problem, S, C, K, seed, eps=1e-6, **kw):
    """make_problem(S, C, K, seed, **kw) -> (s, H, Cm, g, c, lo, hi, w[, m]) with its cold reference run of at most WALK_SOLVES
    solves at eps_abs = eps_rel = eps, as a problem dict with "w" (and "m")."""
    s, H, Cm, g, c, lo, hi, *wm = make_problem(S, C, K, seed, **kw)
    run = AS.iterate(H, Cm, g, c, lo, hi, S, *wm, eps_abs=eps, eps_rel=eps, max_pdas_iters=AS.WALK_SOLVES)
    return AS.as_problem(s, H, Cm, g, c, lo, hi, run, seed, **dict(zip(("w", "m"), wm)))


def soft_box(S, C, K, f32=False, count=1, system=synth.make_system):
    """The first `count` problems soft_problem(S, C, K, seed) of seeds 0, 1, ... < WALK_SEEDS whose cold reference run meets
    walk_ok with a soft non-equality variable active on the way (f32: with eps = F32_EPS, and f32_ok), as problem dicts with "w"
    and the run under "run"."""
    return AS.walk(("soft", S, C, K, f32, system), lambda seed: walked(soft_problem, S, C, K, seed, P.F32_EPS if f32 else 1e-6, system=system),
                  lambda p: AS.walk_ok(p["run"], p["H"], p["Cm"], p["w"], soft_active_on_the_way(p)) and (not f32 or AS.f32_ok(p)), count)


_LONG = {}


def soft_long():
    """soft_problem at box_qp_pdas_ref.LONG (2/1/8197), seed 0, sparse, with its cold reference run (CONVERGED; its margins are
    below MARGIN, so only its final act and point are used)."""
    if "p" not in _LONG:
        _LONG["p"] = walked(soft_problem, *D.LONG, 0, sparse=True)
    return _LONG["p"]


# ---- mixed problems: hard and soft bounds side by side, on states and controls, a weight per variable -------------------------
def mixed_weights(N, seed):
    """Per variable, independently: soft with probability 1/2 and then w = 10 ** uniform(0, 3), else w = 0 (a hard bound)."""
    rng = np.random.default_rng([seed, 310])
    return np.where(rng.random(N) < 0.5, 10.0 ** rng.uniform(0.0, 3.0, N), 0.0)


def mixed_problem(S, C, K, seed, sparse=False, hard_states=True, system=synth.make_system):
    """soft_problem's system, boxes and (K >= 3) lo == hi tracking state with mixed_weights: states and controls both draw, so
    both may be soft, and the tracking state may be hard.  hard_states=False: a state that drew 0 draws a weight of the same
    law instead - every state soft, each with its own weight; the controls as before.  -> (s, H, Cm, g, c, lo, hi, w)."""
    s, H, Cm, g, c, lo, hi, _ = soft_problem(S, C, K, seed, sparse=sparse, system=system)
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
        sa = P.soft_set(t["act"], w)
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


def mixed_box(S, C, K, f32=False, count=1, system=synth.make_system):
    """soft_box's seed walk over mixed_problem: the first `count` seeds < WALK_SEEDS whose trace meets cover_need and whose cold
    reference run meets walk_ok (f32: with eps = F32_EPS, and f32_ok); each dict also holds its cover() under "cover"."""
    need = cover_need(S, C, K)

    def make(seed):
        p = walked(mixed_problem, S, C, K, seed, P.F32_EPS if f32 else 1e-6, system=system)
        return dict(p, cover=cover(p["run"], p["w"], p["lo"], p["hi"], S, C, K))
    return AS.walk(("mixed", S, C, K, f32, system), make, lambda p: covers(p["cover"], need) and
                  AS.walk_ok(p["run"], p["H"], p["Cm"], p["w"], soft_active_on_the_way(p)) and (not f32 or AS.f32_ok(p)), count)


def mixed_layer_box(S, C, K):
    """The first problem of mixed_box(S, C, K) whose final act - the one the layer differentiates through - holds a soft-active
    control with lo != hi."""
    n = S + C
    for count in range(1, AS.WALK_SEEDS + 1):
        ps = mixed_box(S, C, K, count=count)
        if len(ps) < count:
            break
        p = ps[-1]
        if (P.soft_set(p["run"]["act"], p["w"]) & (np.arange(len(p["w"])) % n >= S) & (p["lo"] != p["hi"])).any():
            return p
    return None


def mixed_long():
    """mixed_problem(hard_states=False) at box_qp_pdas_ref.LONG (2/1/8197), sparse, of the first seed whose cold reference run
    converges, with that run (as soft_long: only its final act and point are used).  Soft states, each with its own weight,
    and mixed controls: with hard state bounds drawn over 8197 knots some knot fixes both its state and its control, and the
    reference meets a singular reduced system on its second solve (seeds 0 .. 19, all NONFINITE)."""
    if "mixed" not in _LONG:
        for seed in range(AS.WALK_SEEDS):
            _LONG["mixed"] = walked(mixed_problem, *D.LONG, seed, sparse=True, hard_states=False)
            if _LONG["mixed"]["run"]["status"] == AS.CONVERGED:
                break
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
    runs = [AS.iterate(H, Cm, g, c, lo, hi, S, wi, max_pdas_iters=AS.WALK_SOLVES) for wi in ws]
    return (s, H, Cm, g, c, lo, hi, w), ws, runs


def weight_batch_ok(prob, ws, runs):
    """The seed rule of weight_batch: every run meets box_qp_active_ref.walk_ok's status, solve count and margins, and its worst
    reduced matrix has cond / margin <= COND_CAP / MARGIN - the rounding a solve leaves in a decision, cond * eps, relative to
    the decision's margin is what the walks' two caps bound together, and the all-hard run here has cond 4e8 at a margin of
    9e-4 where the caps pair 1e8 with 1e-5; the mixed and the scaled run end on different points."""
    s, H, Cm = prob[:3]
    for wi, r in zip(ws, runs):
        if not AS.walk_ok(r) or AS.max_cond(r, H, Cm, wi) / AS.min_margin(r) > P.COND_CAP / AS.MARGIN:
            return False
    return bool(np.abs(runs[0]["x"] - runs[1]["x"]).max() > 1e-3)


_WBATCH = {}


def weight_batch_box():
    """weight_batch of the first seed < WALK_SEEDS that meets weight_batch_ok.  -> (seed, problem tuple, [w], [run])."""
    if "p" not in _WBATCH:
        for seed in range(AS.WALK_SEEDS):
            got = weight_batch(seed)
            if weight_batch_ok(*got):
                _WBATCH["p"] = (seed,) + got
                break
    return _WBATCH.get("p")


def hard_state_box_that_fails(S, C, K):
    """The first seed whose hard state box (box_qp_polish_ref.boxes(states=True), no weights) does not converge in the reference."""
    for seed in range(AS.WALK_SEEDS):
        s = synth.make_system(S, C, K, seed=seed)
        H, Cm, g, c = ref.parts(s)
        lo, hi = P.boxes(s, seed + 1, eq=True, states=True)
        if AS.iterate(H, Cm, g, c, lo, hi, S)["status"] != AS.CONVERGED:
            return dict(s=s, H=H, Cm=Cm, g=g, c=c, lo=lo, hi=hi, w=np.zeros(s.N))
    raise AssertionError("no such seed")


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
    """The gradients through problem p's reference act at the point (x, lam), with p's weights and caps where it has them."""
    s = p["s"]
    wm = {k: p[k] for k in ("w", "m") if k in p}
    return P.grads(p["H"], p["Cm"], p["run"]["act"], x, lam, xbar, lambar, s.S, s.C, s.K, lo=p["lo"], hi=p["hi"], **wm)


def di_soft_problem(w, **kw):
    """box_qp_ref.double_integrator(**kw) with the weights w as a problem dict with its cold reference run."""
    s, lo, hi, _ = ref.double_integrator(**kw)
    H, Cm, g, c = ref.parts(s)
    w = np.broadcast_to(np.asarray(w, np.float64), (s.N,)).copy()
    return AS.as_problem(s, H, Cm, g, c, lo, hi, AS.iterate(H, Cm, g, c, lo, hi, s.S, w), None, w=w)


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
