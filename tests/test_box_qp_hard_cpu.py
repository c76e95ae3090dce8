"""CPU suite of the hard cells of the active-set box-QP kernels (tests/box_qp_hard_cells.py): that every
listed cell has a seed inside the unchanged seed rules and every left-out cell has none, that the walks are the recorded ones
(tests/golden/box_qp_hard_walks.json, the fields of tests/golden/box_qp_walks.json), that the fp64 restatement of the iteration on
the oracle's stages follows the reference's acts and lands within 1/100 of each bar of tests/test_gpu_box_qp_hard.py - so no bar
there is set from the device - and that these cells see errors which the cells of synth.make_system cannot see at all:

    (a)  the off-diagonals of R_k dropped from H in the line search's slope;
    (a') the strictly lower triangle of R_k dropped there - a staging of ls_knot_kernel's sR that is wrong and not symmetric;
    (b)  the off-diagonals of Q_k dropped from H x in the stationarity row y_A = g - H x - C^T lambda;
    (c)  the hard shift H_FA b_A dropped from g' in every block that also holds a soft-active variable;
    (c') that shift dropped in every block of a problem with weights and no caps - the g' loop of polish_prepare_kernel's
         BOUNDS_SOFT instantiation without its terms (every one of them is off-diagonal: the row is free, the column active).

Each wrong restatement passes the bar of the old GPU test on the synth cell of the same shape - bit for bit, its blocks are
diagonal - and on the hard cell fails by at least 100 times the bar or by a different act sequence.  Where the mathematics makes
a variant the right one (a 1 x 1 R_k; no block with a hard-active and a free or soft-active variable) the test asserts equality.

`python tests/test_box_qp_hard_cpu.py` records the manifest again."""
import json
import os

import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_alm_ref as A
import box_qp_hard_cells as HC
import box_qp_huber_ref as R
import box_qp_linesearch_ref as L
import box_qp_pdas_ref as D
import box_qp_polish_ref as P
import box_qp_ref as ref
import box_qp_soft_ref as SR
import kkt_grad_ref as kgr
from test_box_qp_walks_cpu import record, sha

MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_qp_hard_walks.json")
PARITY, KKT, STAGE = HC.PARITY, HC.KKT, HC.STAGE
FORMS = ("control", "soft", "mixed", "huber", "ls")
cid = lambda c: "-".join(str(v) for v in c)

LISTED = [(form, S, C, K, f32) for form in FORMS for f32 in (False, True) for S, C, K in HC.cells(form, f32)]
LISTED += [("ls-uncapped", S, C, K, False) for S, C, K in HC.UNCAPPED_CELLS]
LEFT_OUT = [(form, S, C, K, f32) for form in FORMS for f32, out in ((False, HC.LEFT_OUT_F64), (True, HC.LEFT_OUT_F32)) for S, C, K in out[form]]
LISTED_F64 = [c for c in LISTED if not c[4]]


def name_of(form, S, C, K, f32):
    return "%s%s/%d-%d-%d" % (form, "-f32" if f32 else "", S, C, K)


def problem(form, S, C, K, f32=False):
    ps = HC.box(form, S, C, K, f32)
    assert ps, "the walk finds no seed"
    return ps[0]


def synth_problem(form, S, C, K):
    """The walked problem of the old GPU tests at the same shape, or None where their walk has no seed."""
    if form == "ls":
        ps = L.ls_box(S, C, K, L.CAPPED)
    else:
        ps = dict(control=D.control_box, soft=SR.soft_box, mixed=SR.mixed_box, huber=R.huber_box)[form](S, C, K)
    return ps[0] if ps else None


# ---- the cells -----------------------------------------------------------------------------------------------------------------
def test_the_tables_keep_what_they_must():
    """Every shape keeps two of its three K in fp64 in every family; the families keep at least the cells the walks found when
    the cells were chosen; only 2/1/3 may go without a damped kernel test in both dtypes."""
    for form in FORMS:
        for S, C in HC.SHAPES:
            assert sum((S, C, K) in HC.cells(form) for K in HC.F64_K) >= 2, (form, S, C)
    assert set(HC.cells("control")) == set(HC.cells("soft")) == set(HC.cells("ls")) == set(HC.ALL_F64)
    assert set(HC.ALL_F64) - set(HC.cells("mixed")) <= {(32, 16, 9)} and set(HC.ALL_F64) - set(HC.cells("huber")) <= {(2, 1, 9)}
    for form in ("control", "soft", "mixed", "huber"):
        assert HC.cells(form, True) == HC.ALL_F32
    assert set(HC.ALL_F32) - set(HC.cells("ls", True)) <= {(2, 1, 3)}
    assert (12, 6, 9) in HC.UNCAPPED_CELLS
    assert set(HC.NO_TRIPLE_F64) <= {(2, 1, 2), (2, 1, 3), (14, 7, 3)}
    assert set(HC.ALL_F32) - set(HC.NO_TRIPLE_F32) - set(HC.FULL_STEP_ONLY_F32) >= {(4, 2, 3), (6, 3, 3), (14, 7, 3)}
    assert set(HC.ALM_CELLS) == {c[:3] for c in A.HARD_PINNED} and len(A.HARD_PINNED) >= 2


@pytest.mark.parametrize("cell", LISTED, ids=cid)
def test_every_listed_cell_has_a_seed_inside_the_rules(cell):
    """The walk finds its seed; the run's decision margins and the reduced matrices' condition are inside the existing rules."""
    form, S, C, K, f32 = cell
    p = problem(form, S, C, K, f32)
    run = p["run"]
    assert p["seed"] < AS.WALK_SEEDS and run["status"] == AS.CONVERGED and AS.min_margin(run) >= AS.MARGIN
    cond = AS.max_cond(run, p["H"], p["Cm"], p.get("w"))
    print("seed", p["seed"], "solves", run["iters"], "margin", AS.min_margin(run), "cond", cond)
    if form.startswith("ls"):
        assert L.ls_ok(p) and run["iters"] <= L.LS_SOLVES and cond <= L.cond_cap(p["w"].max())
        assert L.damped_on_the_way(run) and p["undamped"]["status"] != AS.CONVERGED
        assert not f32 or L.f32_ok(p)
    else:
        assert AS.walk_ok(run, p["H"], p["Cm"], p.get("w")) and run["iters"] <= AS.WALK_SOLVES and cond <= P.COND_CAP
        assert not f32 or AS.f32_ok(p)
    if form == "mixed":
        assert SR.covers(p["cover"], SR.cover_need(S, C, K))
    if form == "huber":
        sat, quad = R.final_kinds(run, p["w"], p["lo"], p["hi"])
        assert sat and (quad or (S, C, K) in R.MAY_BE_EMPTY)
    # the cell is what it is for: a dense Q_k and, C > 1, a dense R_k, blocks on different scales, c_0 != 0
    Q, Rk, Ak = (np.asarray(t) for t in kgr.blocks_of(p["s"])[:3])
    off = lambda M: np.abs(M - np.einsum("kij,ij->kij", M, np.eye(M.shape[1]))).max()
    assert off(Q) > 0.1 and (C == 1 or off(Rk) > 0.1) and np.abs(Ak + np.eye(S)).max() > 0.3 and np.abs(p["c"][:S]).max() > 0


@pytest.mark.parametrize("cell", LEFT_OUT + [("ls-uncapped", 14, 7, 9, False)], ids=cid)
def test_left_out_cells_have_no_seed(cell):
    form, S, C, K, f32 = cell
    assert HC.box(form, S, C, K, f32) == []


def kernel_cells():
    return [(S, C, K, dt) for S, C, K, dt in HC.KERNEL_CELLS]


@pytest.mark.parametrize("cell", kernel_cells(), ids=cid)
def test_kernel_cells_have_the_inputs_the_module_says(cell):
    S, C, K, dt = cell
    cases, kind = HC.kernel_cases(S, C, K, np.dtype(dt).type)
    f32 = dt == "float32"
    want = "full" if f32 and (S, C, K) in HC.FULL_STEP_ONLY_F32 else "damped" if (S, C, K) in (HC.NO_TRIPLE_F32 if f32 else HC.NO_TRIPLE_F64) else "triple"
    assert kind == want and len(cases) == (3 if kind == "triple" else 1)
    if kind == "triple":
        assert 0 < cases[0][3]["alpha"] < 1 and cases[1][3]["alpha"] == 1.0 and 0 < cases[2][3]["alpha"] < 1


# ---- the manifest --------------------------------------------------------------------------------------------------------------
def alm_record(p):
    """The ALM run as a manifest record: the fields of `record`, the trace being the steps' acts and solves, the margin the last
    violation over its bar."""
    run = p["run"]
    return [dict(seed=p["seed"], form=p["form"], drop=p["drop"], status=int(run["status"]), outer=int(run["outer"]), iters=int(run["iters"]),
                 weight=float(run["weight"]).hex(), trace=sha([np.asarray(st["act"], np.int8) for st in run["steps"]] + [np.array([st["solves"] for st in run["steps"]], np.int64)]),
                 point=sha([np.asarray(run[k], np.float64) for k in ("x", "z", "y", "lam")]))]


def manifest_entry(name):
    kind, cell = name.split("/")
    S, C, K = (int(v) for v in cell.split("-"))
    if kind == "alm":
        return alm_record(HC.alm_box(S, C, K))
    f32 = kind.endswith("-f32")
    return record(HC.box(kind[:-4] if f32 else kind, S, C, K, f32))


NAMES = [name_of(*c) for c in LISTED] + ["alm/%d-%d-%d" % c for c in HC.ALM_CELLS]


def test_the_manifest_names_every_walk():
    with open(MANIFEST) as f:
        assert sorted(json.load(f)) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_walk_is_the_recorded_one(name):
    with open(MANIFEST) as f:
        assert manifest_entry(name) == json.load(f)[name]


# ---- the fp64 stage restatement --------------------------------------------------------------------------------------------------
def same_acts(acts, run):
    want = [t["act"] for t in run["trace"]]
    return len(acts) == len(want) and all(np.array_equal(a, b) for a, b in zip(acts, want))


@pytest.mark.parametrize("cell", LISTED_F64, ids=cid)
def test_fp64_stage_restatement_holds_a_hundredth_of_each_bar(cell):
    """box_qp_hard_cells.restated: stage_iterate / stage_iterate_ls in float64 at the device's PCG settings ends CONVERGED over
    the reference's act sequence; the stage solve on the final act is within PARITY / 100 of the reference's x and lambda and its
    penalised KKT residuals are <= KKT / 100.  12/6/9 uncapped: lambda within PARITY / 10 (box_qp_hard_cells.uncapped_ok says
    why: 3.6e-8)."""
    form, S, C, K, _ = cell
    r = HC.restated(problem(form, S, C, K), form.startswith("ls"))
    print(r)
    assert r["follows"] and r["x"] <= PARITY / 100 and r["kkt"] <= KKT / 100
    assert r["lam"] <= (PARITY / 10 if form == "ls-uncapped" else PARITY / 100)


@pytest.mark.parametrize("cell", HC.ALM_CELLS, ids=cid)
def test_alm_pinned_seed_meets_the_rule_and_the_fp64_restatement_follows(cell):
    """The pinned seed is walk_cell's (the seeds before it fail the rule on the pinned form without the pinned drop), and the
    fp64 stage restatement of the outer loop takes the reference's steps, weights, solves and acts and ends within KKT / 100."""
    S, C, K = cell
    p = HC.alm_box(S, C, K)
    seed, form, drop = A.HARD_PINNED[(S, C, K, False)]
    assert A.meets(p, drop) and (drop is None or not A.meets(p, None))
    run = p["run"]
    got = A.run_alm(p, inner=A.stage_inner(p["s"], np.float64, **STAGE))
    assert got["status"] == A.CONVERGED and (got["outer"], got["iters"], got["weight"]) == (run["outer"], run["iters"], run["weight"])
    for a, b in zip(got["steps"], run["steps"]):
        assert a["w"] == b["w"] and a["solves"] == b["solves"] and np.array_equal(a["act"], b["act"])
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], *A.hard_box(p), got["x"], got["y"], got["lam"])
    own, dist = np.abs(run["x"] - p["exact"]["x"]).max(), np.abs(got["x"] - p["exact"]["x"]).max()
    print("weights", [st["w"] for st in run["steps"]], "kkt", kk, "|x - x*|", dist, "the reference's", own)
    assert kk["stat"] <= KKT / 100 and kk["eq"] <= KKT / 100 and dist <= 1.1 * own
    assert max(st["w"] for st in run["steps"]) >= 1e3             # the weights on the dense blocks' diagonals grow


# ---- wrong on purpose ------------------------------------------------------------------------------------------------------------
def block_masks(s):
    """[N, N] bools: both indices among the states of one knot (Q_k), among the controls of one knot (R_k)."""
    n = s.S + s.C
    idx = np.arange(s.N)
    same = (idx[:, None] // n) == (idx[None, :] // n)
    st = idx % n < s.S
    return same & st[:, None] & st[None, :], same & ~st[:, None] & ~st[None, :]


def without(H, mask, lower_only=False):
    """H with its off-diagonal entries under `mask` zeroed (lower_only: the strictly lower triangle alone)."""
    i, j = np.indices(H.shape)
    return np.where(mask & ((i > j) if lower_only else (i != j)), 0.0, H)


def search_verdict(p, xc, xp, e, Hwrong):
    """The bar of box_qp_device.check_search on the step length that exact_alpha gives with Hwrong in the slope: (alpha on the
    reference's linear piece, |phi'(alpha)| / (N eps scale) with the true H)."""
    S, N = p["s"].S, p["s"].N
    w = L.off_x0(p["w"], S)
    a = L.exact_alpha(Hwrong, p["g"], p["lo"], p["hi"], w, p.get("m"), xc, xp)["alpha"]
    d = xp - xc
    unit = N * np.finfo(np.float64).eps * L.slope_scale(p["H"], p["g"], p["lo"], p["hi"], w, p.get("m"), xc, d, a)
    return e["piece"][0] <= a <= e["piece"][1], abs(L.slope(p["H"], p["g"], p["lo"], p["hi"], w, p.get("m"), xc, d, a)) / unit, a


SEARCH_CELLS = [c[:3] for c in HC.KERNEL_CELLS if c[3] == "float64"]


@pytest.mark.parametrize("lower_only", (False, True), ids=("a-offdiagonal", "a-lower-triangle"))
@pytest.mark.parametrize("cell", SEARCH_CELLS, ids=cid)
def test_a_slope_without_the_off_diagonals_of_R(cell, lower_only):
    """(a), (a'): invisible on the synth cell's first damped search - the same step length bit for bit - and on the hard cell's
    either off the reference's piece or at least 100 SLACK N eps scale from the root.  C = 1: R_k is a scalar, the variant is
    the right slope."""
    S, C, K = cell
    (ps, xc, xp, e), = L.kernel_inputs(S, C, max(K, 3), L.CAPPED, np.float64, True, 1)       # K = 2 is no cell of the old kernel test
    a = L.exact_alpha(without(ps["H"], block_masks(ps["s"])[1], lower_only), ps["g"], ps["lo"], ps["hi"], L.off_x0(ps["w"], S), ps["m"], xc, xp)
    assert a["alpha"] == e["alpha"] and search_verdict(ps, xc, xp, e, without(ps["H"], block_masks(ps["s"])[1], lower_only))[1] <= L.SLACK
    cases, kind = HC.kernel_cases(S, C, K, np.float64)
    caught = False
    for p, xc, xp, e in cases:
        on, slope, alpha = search_verdict(p, xc, xp, e, without(p["H"], block_masks(p["s"])[1], lower_only))
        print("seed", p["seed"], "alpha", alpha, "reference", e["alpha"], "on the piece", on, "slope / (N eps scale)", slope)
        if C == 1:
            assert alpha == e["alpha"]
        caught |= (alpha != 1.0) if e["alpha"] == 1.0 else ((not on) or slope >= 100 * L.SLACK)     # a full step: check_search asks alpha == 1
    assert caught == (C > 1)


def wrong_solve(y_without_Q=False, shift="keep"):
    """box_qp_polish_ref.reduced_solve with an error.  y_without_Q: the stationarity row without the off-diagonals of Q_k.
    shift: "soft blocks" - H_FA b_A dropped from the rows of every Q_k or R_k that holds a soft-active variable; "weights" -
    dropped from every row wherever weights and no caps are given."""
    def solve(H, Cm, g, c, lo, hi, act, w=None, m=None):
        act = np.asarray(act)
        n_state = None
        sat = P.sat_set(act)
        g0 = g
        if sat.any():
            push = np.where(sat, np.sign(act) * np.where(sat, m, 0.0), 0.0)
            g, act = g - push, P.unsaturated(act)
        soft = P.soft_set(act, w)
        Aset = np.flatnonzero(P.hard_set(act, w))
        b = P.bound_values(act, lo, hi)
        solver, F = P._reduced_solver(H, Cm, act, w)
        top = g[F] + (np.where(soft, w, 0.0) * b)[F] if soft.any() else g[F]
        hard_shift = np.zeros(len(g))
        hard_shift[F] = P._sub(H, F, Aset) @ b[Aset]
        if shift == "weights" and w is not None and m is None:
            hard_shift[:] = 0.0
        if shift == "soft blocks" and soft.any():
            blocks = SOLVE_BLOCKS[len(g)]
            hard_shift[np.isin(blocks, blocks[soft])] = 0.0
        sol = solver(np.concatenate([top - hard_shift[F], c - P._cols(Cm, Aset) @ b[Aset]]))
        x = np.zeros(len(g))
        x[Aset] = b[Aset]
        x[F] = sol[:len(F)]
        lam = sol[len(F):]
        y = np.zeros(len(g))
        Hy = without(H, SOLVE_QMASK[len(g)]) if y_without_Q else H
        y[Aset] = (g - Hy @ x - Cm.T @ lam)[Aset]
        if soft.any():
            y[soft] = (w * (x - b))[soft]
        if sat.any():
            y = np.where(sat, push, y)
        return x, y, lam
    return solve


SOLVE_BLOCKS, SOLVE_QMASK = {}, {}


def wrong_run(monkeypatch, p, **kw):
    """box_qp_active_ref.iterate on problem p with wrong_solve(**kw) for its reduced solve."""
    s = p["s"]
    n = s.S + s.C
    idx = np.arange(s.N)
    SOLVE_BLOCKS[s.N] = 2 * (idx // n) + (idx % n >= s.S)
    SOLVE_QMASK[s.N] = block_masks(s)[0]
    monkeypatch.setattr(P, "reduced_solve", wrong_solve(**kw))
    run = AS.iterate(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], s.S, p.get("w"), p.get("m"), max_pdas_iters=AS.WALK_SOLVES)
    monkeypatch.undo()
    return run


def point_verdict(p, got):
    """box_qp_device.check_point's bars on a run: (the reference's solves and acts, the largest of the parity errors over PARITY
    and the penalised KKT residuals over KKT)."""
    run = p["run"]
    if not (got["status"] == AS.CONVERGED and got["iters"] == run["iters"] and same_acts([t["act"] for t in got["trace"]], run)):
        return False, np.inf
    kk = AS.kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], got["x"], got["y"], got["lam"], p.get("w"), p.get("m"))
    return True, max(np.abs(got["x"] - run["x"]).max() / PARITY, np.abs(got["lam"] - run["lam"]).max() / PARITY, max(kk.values()) / KKT)


def exposed(p, kind):
    """Whether the mathematics lets the error show on problem p's run at all.  (b): some act holds a hard-active state.  (c): some
    act holds, in one Q_k or R_k, a soft-active variable, a hard-active one with b != 0 and a free row.  (c'): the problem has
    weights and no caps, and some act a block with a hard-active variable and a row that is not."""
    s, w = p["s"], p.get("w")
    n = s.S + s.C
    idx = np.arange(s.N)
    block, state = 2 * (idx // n) + (idx % n >= s.S), idx % n < s.S
    for t in p["run"]["trace"]:
        act = t["act"]
        hard, soft = P.hard_set(act, w), P.soft_set(P.unsaturated(act), w)
        if kind == "b" and (hard & state).any():
            return True
        for k in np.unique(block[hard]):
            rows = (block == k) & ~hard
            if kind == "c" and rows.any() and (soft & (block == k)).any():
                return True
            if kind == "c'" and rows.any() and w is not None and p.get("m") is None:
                return True
    return False


WRONG = dict(b=dict(y_without_Q=True), c=dict(shift="soft blocks"), **{"c'": dict(shift="weights")})
WRONG_CELLS = [(kind, form) + c for kind, forms in (("b", ("mixed",)), ("c", ("mixed",)), ("c'", ("soft", "mixed")))
               for form in forms for c in HC.cells(form)]


@pytest.mark.parametrize("cell", WRONG_CELLS, ids=cid)
def test_b_c_wrong_solves_are_invisible_on_synth_cells_and_caught_on_hard_ones(cell, monkeypatch):
    kind, form, S, C, K = cell
    q = synth_problem(form, S, C, K)
    assert q is not None
    ok, worst = point_verdict(q, wrong_run(monkeypatch, q, **WRONG[kind]))
    assert ok and worst <= 1.0, worst                              # the old test's cell passes with the error in
    p = problem(form, S, C, K)
    ok, worst = point_verdict(p, wrong_run(monkeypatch, p, **WRONG[kind]))
    print("follows the reference's acts", ok, "worst figure over its bar", worst, "exposed", exposed(p, kind))
    if exposed(p, kind):
        assert not ok or worst >= 100.0
    else:
        assert ok and worst <= 0.01


def test_every_shape_exposes_every_error_somewhere():
    """Per error and shape, some listed K is exposed - except (c) at 2/1, where boxes() bounds one state and the one control per
    knot, so no block of a 2/1 system holds two bounded variables (cover_need says the same of the mixed walks)."""
    for kind, forms in (("b", ("mixed",)), ("c", ("mixed",)), ("c'", ("soft", "mixed"))):
        for S, C in HC.SHAPES:
            hit = any(exposed(problem(form, S, C, K), kind) for form in forms for (s_, c_, K) in HC.cells(form) if (s_, c_) == (S, C))
            assert hit == (not (S == 2 and kind == "c")), (kind, S, C)


if __name__ == "__main__":
    with open(MANIFEST, "w") as f:
        json.dump({name: manifest_entry(name) for name in NAMES}, f, indent=1, sort_keys=True)
        f.write("\n")
