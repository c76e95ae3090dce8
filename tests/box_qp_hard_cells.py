"""The hard cells of the active-set box-QP suites (tests/test_box_qp_hard_cpu.py, tests/test_gpu_box_qp_hard.py; DESIGN.md
sections 3.9 to 3.14): the walked problems of box_qp_pdas_ref, box_qp_soft_ref, box_qp_huber_ref, box_qp_linesearch_ref and
box_qp_alm_ref on asm_ref.hard_blocks - dense SPD Q_k and R_k of condition 100, every block on its own power-of-two scale, A_k
far from the identity, c_0 != 0 - instead of synth.make_system, whose Q_k and R_k are diagonal, whose A_k is nearly -I and whose
c_0 is 0.  Everything else is as it was: box_qp_polish_ref.boxes around the unconstrained solution, the weights, the caps and
every seed rule (walk_ok, ls_ok, f32_ok, COND_CAP, MARGIN, WALK_SEEDS, the ALM seed_checks).  One rule is added, never one relaxed:
an fp64 seed's float64 stage restatement must land within 1/100 of each bar of the GPU file (restated()).

A plain module: the lists below are the cells of the GPU file, the walks are memoised in box_qp_active_ref under keys that hold
the family, and the CPU file asserts a seed for every listed cell.  fp64 cells run at grade 4, fp32 cells at grade 3 on the
problem rounded to fp32 (asm_ref.GRADE)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import asm_ref                                    # noqa: E402
import box_qp_active_ref as AS                    # noqa: E402
import box_qp_alm_ref as A                        # noqa: E402
import box_qp_huber_ref as R                      # noqa: E402
import box_qp_linesearch_ref as L                 # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import box_qp_soft_ref as SR                      # noqa: E402

SHAPES = P.SWEEP_SHAPES
F64_K, F32_K = (2, 3, 9), 3


# ---- the family ------------------------------------------------------------------------------------------------------------------
def hard_f64(S, C, K, seed):
    return asm_ref.to_system(asm_ref.hard_blocks(S, C, K, seed, asm_ref.COND, asm_ref.GRADE["float64"]))


def hard_f32(S, C, K, seed):
    return asm_ref.to_system(asm_ref.hard_blocks(S, C, K, seed, asm_ref.COND, asm_ref.GRADE["float32"]))


def family(f32=False):
    """The system= argument of the problem builders: (S, C, K, seed) -> KKTSystem at the dtype's grade."""
    return hard_f32 if f32 else hard_f64


# ---- the fp64 restatement: a further seed rule --------------------------------------------------------------------------------
PARITY, KKT = 1e-6, 1e-7                          # the bars of box_qp_device.check_point
STAGE = dict(exit_tol=1e-20, max_iters=1000)      # box_qp_device.F64: the PCG settings of the fp64 device runs


def stage_y(p, act, x, lam):
    """y of a stage solve's point on an act, as box_qp_active_ref.stage_iterate forms it."""
    w, m = p.get("w"), p.get("m")
    y = np.where(act != 0, p["g"] - p["H"] @ x - p["Cm"].T @ lam, 0.0)
    if w is not None:
        y = np.where(P.soft_set(act, w), w * (x - P.bound_values(act, p["lo"], p["hi"])), y)
    if m is not None:
        sat = P.sat_set(act)
        y = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), y)
    return y


def restated(p, line_search):
    """The iteration restated in float64 on the oracle's stages (stage_iterate, stage_iterate_ls) at the device's PCG settings.
    -> dict follows (CONVERGED over the reference's act sequence, the steps full where the reference's are and damped where they
    are), x, lam (the stage solve on the final act against the reference's, infinity norm) and kkt (the largest penalised KKT
    residual of that point); ok: follows, and every figure within 1/100 of its bar.  A cell's seed must be ok: the blocks of
    this family put |lambda| and |y| at 1e3 to 1e5, and a seed whose fp64 restatement already uses more than 1/100 of an
    absolute bar says nothing about a kernel that misses it."""
    s, run, w, m = p["s"], p["run"], p.get("w"), p.get("m")
    if line_search:
        status, acts, alphas = L.stage_iterate_ls(s, p["lo"], p["hi"], np.float64, 1e-6, w, m, **STAGE)
        steps = all((a == t) if t in (0.0, 1.0) else (0.0 < a < 1.0) for a, t in zip(alphas, run["alpha"]))
    else:
        status, acts = AS.stage_iterate(s, p["lo"], p["hi"], np.float64, 1e-6, w, m, **STAGE)
        steps = True
    want = [t["act"] for t in run["trace"]]
    follows = status == AS.CONVERGED and steps and len(acts) == len(want) and all(np.array_equal(a, b) for a, b in zip(acts, want))
    x, lam, _ = P.reduced_stage_solve(s, p["lo"], p["hi"], run["act"], np.float64, w=w, m=m, **STAGE)
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], x, stage_y(p, run["act"], x, lam), lam, w, m)
    out = dict(follows=bool(follows), x=float(np.abs(x - run["x"]).max()), lam=float(np.abs(lam - run["lam"]).max()), kkt=max(kk.values()))
    out["ok"] = out["follows"] and out["x"] <= PARITY / 100 and out["lam"] <= PARITY / 100 and out["kkt"] <= KKT / 100
    return out


# ---- the walks -------------------------------------------------------------------------------------------------------------------
WALKS = dict(control=D.control_box, soft=SR.soft_box, mixed=SR.mixed_box, huber=R.huber_box,
             ls=lambda S, C, K, **kw: L.ls_box(S, C, K, L.CAPPED, **kw), **{"ls-uncapped": lambda S, C, K, **kw: L.ls_box(S, C, K, L.UNCAPPED, **kw)})
COLD_FAMILIES = ("control", "soft", "mixed", "huber")


def box(form, S, C, K, f32=False, count=1):
    """The first `count` problems of the form's own walk ("control", "soft", "mixed", "huber", "ls": capped, "ls-uncapped") on the
    hard family - every rule of that walk as it is - that are also restated()["ok"] (fp64; "ls-uncapped": uncapped_ok; an fp32
    cell's restatement rule is the walk's own f32_ok).  Each fp64 dict gains "restated"."""
    under = lambda n: WALKS[form](S, C, K, f32=f32, count=n, system=family(f32))
    if f32:
        return under(count)

    def make(i):
        ps = under(i + 1)
        return dict(ps[i], restated=restated(ps[i], form.startswith("ls"))) if len(ps) > i else None
    return AS.walk(("hard", form, S, C, K), make, lambda p: p["restated"]["ok"] or form == "ls-uncapped" and uncapped_ok(p["restated"]), count)


def uncapped_ok(r):
    """The restatement rule of the uncapped line search (weight 1e4): follows, x and the KKT residuals within 1/100 of their bars
    as everywhere, lambda within 1/10 of its bar.  The family must keep 12/6/9, the one cell whose walk has a seed at all (seed
    16), and that seed's restatement leaves 3.6e-8 in lambda (|lambda|_inf 5e3: 7e-12 of it), 1/28 of the bar: the one figure of
    the suite that is not a hundredth of its bar."""
    return r["follows"] and r["x"] <= PARITY / 100 and r["kkt"] <= KKT / 100 and r["lam"] <= PARITY / 10


def control_box(S, C, K, f32=False, count=1):
    return box("control", S, C, K, f32, count)


def soft_box(S, C, K, f32=False, count=1):
    return box("soft", S, C, K, f32, count)


def mixed_box(S, C, K, f32=False, count=1):
    return box("mixed", S, C, K, f32, count)


def huber_box(S, C, K, f32=False, count=1):
    return box("huber", S, C, K, f32, count)


def ls_box(S, C, K, form=L.CAPPED, f32=False, count=1):
    return box("ls" if form == L.CAPPED else "ls-uncapped", S, C, K, f32, count)


def kernel_cases(S, C, K, dt):
    """The systems of a line-search kernel test, capped: box_qp_linesearch_ref.kernel_batch's triple where the walks find one,
    else the damped search kernel_inputs finds, else (FULL_STEP_ONLY) the full step it finds.  -> (cases, kind): "triple",
    "damped" or "full"."""
    f32 = np.dtype(dt) == np.float32
    batch = L.kernel_batch(S, C, K, L.CAPPED, dt, system=family(f32))
    if batch:
        return batch, "triple"
    one = L.kernel_inputs(S, C, K, L.CAPPED, dt, True, 1, system=family(f32))
    if one:
        return one, "damped"
    return L.kernel_inputs(S, C, K, L.CAPPED, dt, False, 1, system=family(f32)), "full"


# ---- the cells -------------------------------------------------------------------------------------------------------------------
ALL_F64 = [(S, C, K) for S, C in SHAPES for K in F64_K]
ALL_F32 = [(S, C, F32_K) for S, C in SHAPES]

# The cells whose walk finds no seed among the first WALK_SEEDS, by name: the only reason a cell is left out.  Every shape keeps
# two of its three K in fp64 in every family; tests/test_box_qp_hard_cpu.py asserts that these walks are indeed empty.
#   mixed 32/16/9: no seed meets cover_need and walk_ok together;
#   huber 2/1/9: no final act holds a saturated variable next to a soft quadratic-active one within the margins;
#   ls 2/1/3 in fp32: the fp32 restatement follows none of the damped runs that meet ls_ok.
LEFT_OUT_F64 = dict(control=(), soft=(), mixed=((32, 16, 9),), huber=((2, 1, 9),), ls=())
LEFT_OUT_F32 = dict(control=(), soft=(), mixed=(), huber=(), ls=((2, 1, 3),))
# The uncapped line search (weight 1e4) keeps one cell: at every other one the walk is empty (the damped run of every seed leaves
# the margins or cond_cap(1e4), or the undamped run converges too).
UNCAPPED_CELLS = [(12, 6, 9)]
# The kernel tests.  NO_TRIPLE: kernel_batch finds no triple (two damped searches of different seeds and a full step), and the
# test runs the one damped search kernel_inputs finds, B = 1.  FULL_STEP_ONLY: in fp32 at 32/16/3 no damped search of any seed
# keeps its root 2 SLACK N eps scale off the ends of its linear piece (N = 128 and the scale of a dense graded H: the largest
# margin among seeds 0 .. 19 is 0.45 of that bar), so the rule of search_inputs leaves no damped search and the test runs the
# full step it finds: both slopes against the reference and x+ bit for bit.  The shape's fp64 cells have their triples.
NO_TRIPLE_F64 = ((2, 1, 2), (2, 1, 3), (14, 7, 3))
NO_TRIPLE_F32 = ((2, 1, 3), (12, 6, 3))
FULL_STEP_ONLY_F32 = ((32, 16, 3),)


def cells(form, f32=False):
    out = LEFT_OUT_F32 if f32 else LEFT_OUT_F64
    return [c for c in (ALL_F32 if f32 else ALL_F64) if c not in out[form]]


KERNEL_CELLS = [(S, C, K, dt) for dt in ("float64", "float32") for S, C, K in (ALL_F64 if dt == "float64" else ALL_F32)]
LAYER_CELLS = [(6, 3, 9), (14, 7, 3)]
BATCH_CELL = (14, 7, 9)                            # one call, three systems: a soft, a huber and a mixed seed at their own weights


def batch_problems():
    """The three systems of the batch test, as huber problems of one call: the soft seed with caps of +inf, the huber seed, the
    mixed seed with caps of +inf."""
    S, C, K = BATCH_CELL
    inf = lambda p: dict(p, m=np.full(p["s"].N, np.inf))
    return [inf(soft_box(S, C, K)[0]), huber_box(S, C, K)[0], inf(mixed_box(S, C, K)[0])]


# ---- ALM -------------------------------------------------------------------------------------------------------------------------
ALM_CELLS = [(4, 2, 3), (6, 3, 9), (14, 7, 3)]     # fp64; box_qp_alm_ref.HARD_PINNED holds walk_cell's results on the family


def alm_box(S, C, K):
    return A.alm_box(S, C, K, system=hard_f64, pinned=A.HARD_PINNED)
