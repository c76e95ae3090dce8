"""The all-hard problems of the active-set iteration's tests (box_qp_active_ref): the walked
control-only boxes, the constructed problems whose cold run meets the seed rule, the double integrators, the case tables and
the inputs of box_qp_layer as numpy arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
from gato_python_amd import synth                 # noqa: E402


def control_problem(S, C, K, seed, sparse=False, eps=1e-6, system=synth.make_system):
    """system(S, C, K, seed) (a callable -> KKTSystem; synth.make_system, or a family of tests/box_qp_hard_cells.py) with
    box_qp_polish_ref.boxes(s, seed + 1, eq = K >= 3, states=False) and its cold reference run, as a problem dict."""
    s = system(S, C, K, seed)
    if sparse:
        H, Cm, g, c = ref.sparse_parts(s)
        dz = ref.kkt_solver(H, Cm)(np.concatenate([g, c]))[:s.N]
    else:
        H, Cm, g, c = ref.parts(s)
        dz = None
    lo, hi = P.boxes(s, seed + 1, eq=K >= 3, states=False, dz=dz)
    run = AS.iterate(H, Cm, g, c, lo, hi, S, eps_abs=eps, eps_rel=eps, max_pdas_iters=AS.WALK_SOLVES)
    return AS.as_problem(s, H, Cm, g, c, lo, hi, run, seed)


def control_box(S, C, K, f32=False, count=1, sparse=False, system=synth.make_system):
    """The first `count` control-only problems control_problem(S, C, K, seed) of seeds 0, 1, ... < WALK_SEEDS whose cold
    reference run meets walk_ok (f32: with eps = F32_EPS, and f32_ok), as a list of problem dicts with the run under "run".
    system: the family of systems the walk draws from, part of the walk's cache key."""
    return AS.walk(("control", S, C, K, f32, sparse, system),
                   lambda seed: control_problem(S, C, K, seed, sparse, P.F32_EPS if f32 else 1e-6, system),
                  lambda p: AS.walk_ok(p["run"], p["H"], p["Cm"]) and (not f32 or AS.f32_ok(p)), count)


def constructed_cold(S, C, K, count=1):
    """The first `count` problems of box_qp_polish_ref.constructed(S, C, K) (active states, dense Q and R, its own seed rule)
    whose cold reference run also meets walk_ok; each dict gains "run"."""
    def make(i):
        ps = P.constructed(S, C, K, count=i + 1)
        if len(ps) <= i:
            return None
        p = ps[i]
        return dict(p, run=AS.iterate(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], S, max_pdas_iters=AS.WALK_SOLVES))
    return AS.walk(("constructed", S, C, K), make, lambda p: AS.walk_ok(p["run"], p["H"], p["Cm"]), count)


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
    return AS.as_problem(s, H, Cm, g, c, lo, hi, AS.iterate(H, Cm, g, c, lo, hi, s.S), None)


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
