"""The active-set box-QP kernels on dense graded blocks (tests/box_qp_hard_cells.py): the bodies of the
old GPU tests, at their old bars, on problems whose Q_k and R_k are dense SPD of condition 100, every block on its own
power-of-two scale, A_k far from the identity and c_0 != 0.  The cells of synth.make_system have diagonal Q_k and R_k, so the
staging of sQ / sR in ls_knot_kernel, the w_i added to the diagonal of a dense block before the Gauss-Jordan, the hard shift
g' = g - H_:A b_A next to soft rows and the stationarity row of polished_point_knot had never seen an off-diagonal entry.

tests/test_box_qp_hard_cpu.py asserts on the CPU that every cell here has a seed inside the unchanged seed rules, that the fp64
restatement of the iteration holds 1/100 of every bar used here, and that wrong restatements which the old cells pass fail on
these.  Every test prints its figures on lines that start with "figure": family, name, measured, bar."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_active_ref as AS                    # noqa: E402
import box_qp_hard_cells as HC                    # noqa: E402
import box_qp_linesearch_ref as L                 # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import (alm_cold_case, check_point, check_search, cold_case, dev_inputs, dev_w, fp32_case, ls_converges_case,  # noqa: E402
                           ls_fp32_case, ls_layer_gradients_case, pdas, point_bits, solver)

cid = lambda c: "-".join(str(v) for v in c)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def figures(family, got):
    for k, v in got.items():
        print("figure", family, k, v, dict(x=HC.PARITY, lam=HC.PARITY, kkt=HC.KKT)[k])


def first(form, S, C, K, f32=False):
    ps = HC.box(form, S, C, K, f32)
    assert ps, "the walk finds no seed"
    p = ps[0]
    print("seed", p["seed"], "solves", p["run"]["iters"], "margin", AS.min_margin(p["run"]))
    return p


# ---- 1. cold runs ----------------------------------------------------------------------------------------------------------------
COLD = [(form, S, C, K) for form in HC.COLD_FAMILIES for S, C, K in HC.cells(form)]


@pytest.mark.parametrize("cell", COLD, ids=cid)
def test_cold_run(cell):
    """box_qp_device.cold_case: one assembly per reference solve, check_point, the same bits on a repeat."""
    form, S, C, K = cell
    figures(form, cold_case(first(form, S, C, K)))


# ---- 2. fp32 ---------------------------------------------------------------------------------------------------------------------
F32 = [(form, S, C, K) for form in HC.COLD_FAMILIES for S, C, K in HC.cells(form, True)]


@pytest.mark.parametrize("cell", F32, ids=cid)
def test_fp32_ends_on_the_reference_act(cell):
    """box_qp_device.fp32_case on the problem rounded to fp32 (grade 3): the bodies of test_fp32_ends_on_the_reference_act in
    test_gpu_box_qp_pdas.py (control: no solve count), _soft.py, _huber.py and of test_fp32_mixed_ends_on_the_reference_act."""
    form, S, C, K = cell
    fp32_case(first(form, S, C, K, True), iters=form != "control")


# ---- 3. the line-search kernels alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", HC.KERNEL_CELLS, ids=cid)
def test_line_search_kernels(cell):
    """check_search, capped: the first system alone (B = 1) and, where the walks find a triple, the full step alone and the three
    as a batch.  No triple: the damped search kernel_inputs finds; 32/16/3 in fp32: the full step (box_qp_hard_cells says why)."""
    S, C, K, name = cell
    dt = np.dtype(name).type
    cases, kind = HC.kernel_cases(S, C, K, dt)
    assert cases, "no inputs at %d/%d/%d" % (S, C, K)
    worst = check_search(solver(S, C, K, dt), cases[:1], dt)
    if kind == "triple":
        worst = max(worst, check_search(solver(S, C, K, dt), cases[1:2], dt), check_search(solver(S, C, K, dt, batch=3), cases, dt))
    assert kind == "full" or worst > 0.0
    print("figure", "ls-kernel-" + name, "slope", worst, L.SLACK)


# ---- 4. the line search end to end -------------------------------------------------------------------------------------------------
E2E = [("ls",) + c for c in HC.cells("ls")] + [("ls-uncapped",) + c for c in HC.UNCAPPED_CELLS]


@pytest.mark.parametrize("cell", E2E, ids=cid)
def test_line_search_converges_where_the_undamped_iteration_does_not(cell):
    form, S, C, K = cell
    figures(form, ls_converges_case(first(form, S, C, K)))


@pytest.mark.parametrize("cell", HC.cells("ls", True), ids=cid)
def test_line_search_fp32_follows_the_reference(cell):
    ls_fp32_case(first("ls", *cell, True))


# ---- 5. the layer ------------------------------------------------------------------------------------------------------------------
LAYER = [c + (st,) for c in HC.LAYER_CELLS for st in (False, True)]


@pytest.mark.parametrize("S,C,K,stale", LAYER, ids=["%d-%d-%d-%s" % (S, C, K, "stale" if st else "fresh") for S, C, K, st in LAYER])
def test_layer_gradients(S, C, K, stale):
    """box_qp_layer(method="pdas", line_search=True): all fifteen gradients against box_qp_polish_ref.grads, err < 1e-6 max(1,
    |want|); stale: a kkt_solve of the cell's control problem replaces the assembly between the passes."""
    worst = ls_layer_gradients_case(first("ls", S, C, K), stale, first("control", S, C, K))
    print("figure", "layer", "grad", worst, 1e-6)


# ---- 6. ALM ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", HC.ALM_CELLS, ids=cid)
def test_alm_converges_on_hard_state_bounds(cell):
    p = HC.alm_box(*cell)
    assert p is not None, "no pinned seed"
    dist, own = alm_cold_case(p)
    print("figure", "alm", "dist-over-own", dist / own, 10.0)
    print("weights", [st["w"] for st in p["run"]["steps"]])


# ---- 7. a batch --------------------------------------------------------------------------------------------------------------------
def test_batch_of_a_soft_a_huber_and_a_mixed_system():
    """One call, three different 14/7/9 systems at their own weights (the soft and the mixed one with caps of +inf): every system
    meets check_point and has the bits of its solo run in its own form."""
    S, C, K = HC.BATCH_CELL
    ps = HC.batch_problems()
    sol = solver(S, C, K, np.float64, batch=3)
    inp = dev_inputs(sol, [p["s"] for p in ps], [(p["lo"], p["hi"]) for p in ps])
    r = pdas(sol, inp, ps[0]["s"].rho, soft_weight=dev_w(sol, [p["w"] for p in ps]), soft_cap=dev_w(sol, [p["m"] for p in ps]))
    print("seeds", [p["seed"] for p in ps], "iters", r.iters.tolist())
    assert len({p["run"]["iters"] for p in ps}) > 1 or len({p["seed"] for p in ps}) > 1
    one = solver(S, C, K, np.float64)
    for b, (p, capped) in enumerate(zip(ps, (False, True, False))):
        q = p if capped else {k: v for k, v in p.items() if k != "m"}
        figures("batch", check_point(sol, r, b, q, p["run"]))
        wm = {k: dev_w(one, [q[v]]) for k, v in (("soft_weight", "w"), ("soft_cap", "m")) if v in q}
        solo = pdas(one, dev_inputs(one, [p["s"]], [(p["lo"], p["hi"])]), p["s"].rho, **wm)
        assert point_bits(r, b, sol) == point_bits(solo, 0, one), b
