"""The capped (Huber) soft-bound problems of the active-set iteration's tests (box_qp_active_ref):
box_qp_soft_ref's problems with a cap on the penalty force, walked for final acts that hold saturated variables, and the case
tables."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_soft_ref as SR                      # noqa: E402
from gato_python_amd import synth                 # noqa: E402

WEIGHT, CAP = SR.WEIGHT, 1.0                      # the weight and the cap of the walked problems' soft state bounds


# ---- walked problems -------------------------------------------------------------------------------------------------------
def huber_problem(S, C, K, seed, sparse=False, weight=WEIGHT, cap=CAP, system=synth.make_system):
    """box_qp_soft_ref.soft_problem with the cap `cap` on every state.  -> (s, H, Cm, g, c, lo, hi, w, m)."""
    s, H, Cm, g, c, lo, hi, w = SR.soft_problem(S, C, K, seed, sparse=sparse, weight=weight, system=system)
    return s, H, Cm, g, c, lo, hi, w, np.where(w > 0, float(cap), np.inf)


def final_kinds(run, w, lo, hi):
    """(a saturated lo != hi variable, a soft quadratic-active lo != hi one) in the run's final act."""
    ne = lo != hi
    return bool((P.sat_set(run["act"]) & ne).any()), bool((AS.quad_set(run["act"], w) & ne).any())


# the (shape, K) cells whose walk may find no seed (at K = 2 and 3 the two smallest shapes hold too few bounded states for a
# saturated variable under this rule): a test on one of them says so by name; every other cell must have a seed
MAY_BE_EMPTY = {(2, 1, 2), (2, 1, 3), (4, 2, 2), (4, 2, 3)}


def huber_box(S, C, K, f32=False, count=1, system=synth.make_system):
    """The first `count` problems huber_problem(S, C, K, seed) of seeds 0, 1, ... < WALK_SEEDS whose cold reference run meets
    walk_ok and whose final act holds a saturated lo != hi variable and - off MAY_BE_EMPTY - a soft quadratic-active one (f32:
    with eps = F32_EPS, and f32_ok), as problem dicts with "w", "m" and the run under "run"."""
    def kinds(p):
        sat, quad = final_kinds(p["run"], p["w"], p["lo"], p["hi"])
        return sat and (quad or (S, C, K) in MAY_BE_EMPTY)
    return AS.walk(("huber", S, C, K, f32, system), lambda seed: SR.walked(huber_problem, S, C, K, seed, P.F32_EPS if f32 else 1e-6, system=system),
                  lambda p: AS.walk_ok(p["run"], p["H"], p["Cm"], p["w"], lambda run: kinds(p)) and (not f32 or AS.f32_ok(p)), count)


_LONG = {}
LONG_WEIGHT, LONG_CAP = 10.0, 0.3


def huber_long():
    """huber_problem at box_qp_pdas_ref.LONG (2/1/8197), sparse, with LONG_WEIGHT and LONG_CAP - at weight 100 and cap 1 the
    undamped iteration cycles over 8197 knots (about 100 entries change per solve, seeds 0 .. 3) - of the first seed whose cold
    reference run converges on an act with a saturated variable among the knots >= 8192, with that run (only its final act and
    point are used)."""
    if "p" not in _LONG:
        S, C, K = D.LONG
        for seed in range(AS.WALK_SEEDS):
            p = _LONG["p"] = SR.walked(huber_problem, S, C, K, seed, sparse=True, weight=LONG_WEIGHT, cap=LONG_CAP)
            if p["run"]["status"] == AS.CONVERGED and (np.flatnonzero(P.sat_set(p["run"]["act"])) // (S + C) >= 8192).any():
                break
    return _LONG["p"]


# ---- mixed problems: a weight and a cap per variable, on states and controls ---------------------------------------------------
def mixed_caps(N, seed):
    """Per variable, independently: 10 ** uniform(-1, 1) or +inf with probability 1/2 each."""
    rng = np.random.default_rng([seed, 311, 1])
    return np.where(rng.random(N) < 0.5, 10.0 ** rng.uniform(-1.0, 1.0, N), np.inf)


def mixed_problem(S, C, K, seed, system=synth.make_system):
    """box_qp_soft_ref.mixed_problem with mixed_caps.  -> (s, H, Cm, g, c, lo, hi, w, m)."""
    s, H, Cm, g, c, lo, hi, w = SR.mixed_problem(S, C, K, seed, system=system)
    return s, H, Cm, g, c, lo, hi, w, mixed_caps(s.N, seed)


def mixed_box(S, C, K):
    """The first mixed_problem(S, C, K, seed), seed < 4 WALK_SEEDS, whose cold reference run meets walk_ok and whose final act
    holds a saturated control with lo != hi; None if there is none."""
    def saturated_control(p):
        return (P.sat_set(p["run"]["act"]) & (np.arange(p["s"].N) % (S + C) >= S) & (p["lo"] != p["hi"])).any()
    ps = AS.walk(("capped mixed", S, C, K), lambda seed: SR.walked(mixed_problem, S, C, K, seed),
                lambda p: AS.walk_ok(p["run"], p["H"], p["Cm"], p["w"], lambda run: saturated_control(p)), 1, 4 * AS.WALK_SEEDS)
    return ps[0] if ps else None


SHAPES = SR.SHAPES
COLD_K = SR.COLD_K
F32_CASES = SR.F32_CASES
HUBER_KEYS = SR.SOFT_KEYS + ("x_soft_max", "u_soft_max")


def huber_math_arrays(p):
    """box_qp_soft_ref.soft_math_arrays plus x_soft_max [K, S] and u_soft_max [K-1, C], in HUBER_KEYS' order."""
    s = p["s"]
    return SR.soft_math_arrays(p) + [np.ascontiguousarray(t) for t in P.split_states_controls(p["m"], s.S, s.C, s.K)]
