"""The cross-term kernels (DESIGN.md sections 3.15 to 3.17) on dense R_k, graded blocks and A_k far from I: the cells of
tests/cross_hard_cells.py (asm_ref.hard_blocks with the M of synth.make_cross) through the bodies and at the bars of
tests/test_gpu_cross.py, tests/test_gpu_box_qp_cross.py and tests/test_gpu_cross_tangent.py, whose own cells have diagonal R_k,
A_k = -(I + 1 % noise), c_0 = 0 and one scale at every knot.  On those the Gauss-Jordan of cross_prepare_kernel inverts diagonal
matrices, sRi is read where a transposed index changes nothing, the control rows of H x in qp_update_cross_kernel and
qp_update_kernel have no off-diagonal term of R, and W_k-1 for W_k costs little.

  (a) cross_prepare per block, (b) cross_rhs and cross_finish from the W of (a): fp64 against the longdouble restatement at
      BLOCK_BAR, fp32 beside the float32 restatement (f32_parity.check_f32); poisoned work area, inputs off the 16-byte grid.
  (c) whole solves and re-solves at the PCG settings asm_ref.EXIT_TOL / MAX_ITERS against cross_ref.dense_solve at SOLVE_BAR, the
      same bits twice and solo; fp32 at F32_TIGHT within 10 x the error of cross_ref.oracle32_solve.
  (d) the eight gradients of kkt_solve(M=) against cross_ref.dense_reference at SOLVE_BAR (the formulas themselves: central
      differences on the CPU, tests/test_cross_hard_cpu.py).
  (e) 25 ADMM iterations at eps 0 through Solver.box_qp_cross and, without M, Solver.box_qp: x, z, y, lam within 1e-8 of
      box_qp_ref.admm, and - what the parity tests of the older files do not look at - the reported res_prim and res_dual against
      box_qp_ref.residuals in float64 on the device's own x, z, y, lam, at 1e-9 max(scale, 1).  The residual is where a wrong
      control row of H x shows: it feeds nothing else but the freeze test.  (A maximum over rows: on 4/2/3 a state row holds it
      and a wrong R row would not move it; see test_cross_hard_cpu.py.  The converged cells of (f) have no such blind spot.)
  (f) converged box QPs (grade 0, control-only boxes, eps 1e-7; fp32 at eps 1e-4 and F32_EXIT_TOL) by check_converged.  The
      reference converges on the float32-rounded inputs of both fp32 cells (51 and 312 iterations): none is left out.
  (g) kkt_solve_tangents(M=) with tangents of all eight inputs, R = 3, against cross_tangent_ref.dense_tangent at SOLVE_BAR.

tests/test_cross_hard_cpu.py asserts on the CPU that every cell here is positive definite and conditioned within the caps of the
cross suite, that the references' own errors sit a factor 100 below these bars, and that the reference ADMM converges on (f).
A whole run writes profiles/cross_hard_accuracy.json."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import asm_ref                                      # noqa: E402
import box_qp_cross_ref as XR                       # noqa: E402
import box_qp_ref as ref                            # noqa: E402
import cross_hard_cells as HC                       # noqa: E402
from box_qp_device import PARITY, admm_host, admm_run, solver as qp_solver       # noqa: E402
from gato_python_amd import _lib                    # noqa: E402
from test_gpu_box_qp_cross import F32_EXIT_TOL, RHO, SYN, check_converged, check_parity, cross_run, inputs      # noqa: E402
from test_gpu_cross import (BLOCK_BAR, SOLVE_BAR, gradients_of_a_batch_case, prepare_fp32_case, prepare_fp64_case,      # noqa: E402
                            rhs_and_finish_case, rounded, solve_rhs_cross_case, whole_solve_fp32_case, whole_solve_fp64_case)
from test_gpu_cross_tangent import tangents_case    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARD = dict(exit_tol=asm_ref.EXIT_TOL, max_iters=asm_ref.MAX_ITERS)         # the fp64 PCG settings of every whole solve here
RES_BAR = 1e-9                                      # check_converged's: reported against re-evaluated residuals, x max(scale, 1)
EPS = float(np.finfo(np.float64).eps)
G64, G32 = HC.GRADE["float64"], HC.GRADE["float32"]
BLOCKS, SOLVES, F32, RESIDUALS = [], [], [], []     # the record of a run

KERNEL_CELLS = [(S, C, K) for S, C in HC.SHAPES for K in HC.KERNEL_K]
WHOLE = [(S, C, K, B) for S, C, K in HC.SOLVE_CELLS for B in HC.SOLVE_B]
cell_ids = lambda cells: ["-".join(str(v) for v in c) for c in cells]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()
    yield
    whole = (len(BLOCKS) == len(KERNEL_CELLS) and len(SOLVES) == len(WHOLE) and len(F32) == sum(B for _, _, _, B in WHOLE)
             and len(RESIDUALS) == 2 * len(HC.PARITY_CELLS) + 3)
    if whole:                                                               # a selection does not replace the record
        worst = dict(block_err_eps=max(e["err_eps"] for e in BLOCKS), solve_err=max(e["err"] for e in SOLVES),
                     fp32_device_over_restatement=max(e["err_device"] / e["err_restatement32"] for e in F32),
                     residual_diff_over_scale=max(max(e["prim"], e["dual"]) for e in RESIDUALS))
        try:
            with open(os.path.join(ROOT, "profiles", "cross_hard_accuracy.json"), "w") as f:
                json.dump(dict(bars=dict(block_err_eps=BLOCK_BAR / EPS, solve_err=SOLVE_BAR, fp32_device_over_restatement=10.0,
                                         residual_diff_over_scale=RES_BAR),
                               worst=worst, blocks_fp64=BLOCKS, solves_fp64=SOLVES, solves_fp32=F32, residuals=RESIDUALS), f, indent=1)
        except OSError:                                                     # a read-only tree: the record stays as committed
            pass


def hard(S, C, K, B, dt=np.float64):
    """Seeds 0 .. B-1 at the grade of dt, every value rounded to dt."""
    return rounded(HC.hard_batch(S, C, K, B, HC.grade_of(dt)), dt)


# ---- (a), (b): the kernels alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", KERNEL_CELLS, ids=cell_ids(KERNEL_CELLS))
def test_prepare_fp64_per_block(S, C, K):
    """W, Q'', A^' and g' of seeds 0, 1, 2 per block within BLOCK_BAR of the longdouble restatement: the Gauss-Jordan on a dense
    R_k + rho I of condition 100, A^' from an A far from I, every block on a scale of its own; the copies bit for bit."""
    e = prepare_fp64_case(S, C, K, hard(S, C, K, 3))
    BLOCKS.append(dict(S=S, C=C, K=K, err_eps=float(e / EPS)))


@pytest.mark.parametrize("S,C,K", KERNEL_CELLS, ids=cell_ids(KERNEL_CELLS))
def test_prepare_fp32_beside_the_float32_restatement(S, C, K):
    prepare_fp32_case(S, C, K, hard(S, C, K, 3, np.float32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("S,C,K", KERNEL_CELLS, ids=cell_ids(KERNEL_CELLS))
def test_rhs_and_finish_alone(S, C, K, dt):
    """R = 2 vectors per system through the dense, graded W that cross_prepare stored."""
    rhs_and_finish_case(S, C, K, dt, hard(S, C, K, 3, dt))


# ---- (c): whole solves and re-solves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K,B", WHOLE, ids=cell_ids(WHOLE))
def test_whole_solve_fp64_against_the_dense_cross_kkt(S, C, K, B):
    """lambda and dz of every system within SOLVE_BAR of cross_ref.dense_solve; the same bits twice, and solo."""
    e = whole_solve_fp64_case(S, C, K, hard(S, C, K, B), HARD)
    SOLVES.append(dict(S=S, C=C, K=K, B=B, err=float(e)))


@pytest.mark.parametrize("S,C,K", HC.RESOLVE_CELLS, ids=cell_ids(HC.RESOLVE_CELLS))
def test_solve_rhs_cross_against_the_dense_solve(S, C, K):
    """R = 3 right-hand sides for each of two systems."""
    solve_rhs_cross_case(S, C, K, 3, hard(S, C, K, 2), HARD)


@pytest.mark.parametrize("S,C,K,B", WHOLE, ids=cell_ids(WHOLE))
def test_whole_solve_fp32_beside_the_float32_restatement(S, C, K, B):
    """Grade 3 at F32_TIGHT: the device's error at most 10 x that of cross_ref.oracle32_solve, which leaves its loop by tolerance
    on every one of these cells (tests/test_cross_hard_cpu.py).  Both numbers per system go to the record."""
    whole_solve_fp32_case(S, C, K, hard(S, C, K, B, np.float32), F32)


# ---- (d): gradients -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", HC.GRAD_CELLS, ids=cell_ids(HC.GRAD_CELLS))
def test_gradients_of_a_batch_against_the_dense_reference(S, C, K):
    """All eight gradients of seeds 0 and 1 within SOLVE_BAR of cross_ref.dense_reference; seed 2 has a zero upstream gradient
    and exactly zero gradients."""
    gradients_of_a_batch_case(S, C, K, hard(S, C, K, 3), **HARD)


# ---- (e): the ADMM iteration and its reported residuals -----------------------------------------------------------------------------
def check_residuals(got, H, p, tag, with_M):
    """The reported res_prim and res_dual against box_qp_ref.residuals in float64 on the device's own x, z, y, lam."""
    rp, rd, sp, sd = ref.residuals(H, p["Cm"], p["g"], p["c"], got["x"], got["z"], got["y"], got["lam"])
    dp, dd = abs(got["res_prim"] - rp) / max(sp, 1.0), abs(got["res_dual"] - rd) / max(sd, 1.0)
    print(tag, "res_prim %.6g against %.6g, res_dual %.6g against %.6g: %.3g, %.3g of the scales" % (got["res_prim"], rp, got["res_dual"], rd, dp, dd))
    RESIDUALS.append(dict(cell=tag, with_M=with_M, prim=float(dp), dual=float(dd)))
    assert dp <= RES_BAR and dd <= RES_BAR, (tag, got["res_prim"], rp, got["res_dual"], rd)


def parity_case(keys, with_M):
    """PARITY (25 iterations, eps 0) at admm_rho = 10 on problem(*key) of every key in one call: Solver.box_qp_cross, or
    Solver.box_qp on the same blocks and box without M."""
    S, C, K = keys[0][:3]
    ps = [HC.problem(*k) for k in keys]
    sol = qp_solver(S, C, K, np.float64, batch=len(keys))
    inp, Mb = inputs(sol, ps)
    r = cross_run(sol, inp, Mb, **PARITY, **SYN) if with_M else admm_run(sol, inp, RHO, **PARITY, **SYN)
    for b, (k, p) in enumerate(zip(keys, ps)):
        want = HC.parity_reference(k, with_M)
        assert np.any(want["y"] != 0) and np.any(want["z"] != want["x"])
        tag = "%d-%d-%d seed %d%s" % (k[:4] + ("" if with_M else " without M",))
        got = admm_host(r, b, sol)
        check_parity(got, want, XR.PARITY_ITERS, tag)
        check_residuals(got, p["H"] if with_M else p["H0"], p, tag, with_M)
    sol.close()


@pytest.mark.parametrize("with_M", [True, False], ids=["box_qp_cross", "box_qp"])
@pytest.mark.parametrize("key", HC.parity_keys(), ids=cell_ids([k[:3] for k in HC.parity_keys()]))
def test_iterates_and_reported_residuals_match_reference(key, with_M):
    """Full boxes (state clips, one lo == hi control) around the dense solution, grade 4."""
    parity_case([key], with_M)


def test_iterates_and_reported_residuals_match_reference_batch():
    """B = 3 at 4/2/9: seed 1 has M = 0, seed 2 a control-only box."""
    keys = HC.batch_keys()
    assert not HC.problem(*keys[1])["M"].any() and np.isinf(HC.problem(*keys[2])["lo"][6:10]).all()
    parity_case(keys, True)


@pytest.mark.parametrize("shape", HC.SHAPES, ids=cell_ids(HC.SHAPES))
def test_a_control_of_every_full_knot_is_at_a_bound_on_some_cell(shape):
    """From the reference alone: on some cell of each shape, with and without M, every full knot has a control on a bound."""
    for with_M in (True, False):
        assert any(HC.knots_with_a_control_at_a_bound(HC.parity_reference(k, with_M), HC.problem(*k)).all()
                   for k in HC.parity_keys() if k[:2] == shape)


# ---- (f): converged box QPs ---------------------------------------------------------------------------------------------------------
CONVERGED = [(k, np.float64, 1e-7) for k in HC.converged_keys()] + [(k, np.float32, 1e-4) for k in HC.converged_keys("float32")]


@pytest.mark.parametrize("key,dt,eps", CONVERGED, ids=["%d-%d-%d-%s" % (k[:3] + (k[7],)) for k, _, _ in CONVERGED])
def test_converged_solves(key, dt, eps):
    """Grade 0, control-only boxes, admm_rho = 10: KKT residuals, reported against re-evaluated residuals, z inside the box."""
    S, C, K = key[:3]
    p = HC.problem(*key)
    sol = qp_solver(S, C, K, dt)
    inp, Mb = inputs(sol, [p])
    pcg = dict(exit_tol=F32_EXIT_TOL) if dt == np.float32 else {}
    r = cross_run(sol, inp, Mb, eps_abs=eps, eps_rel=eps, **pcg, **SYN)
    got = check_converged(sol, r, 0, p, eps)
    assert np.any(got["y"] != 0)
    sol.close()


# ---- (g): tangents end to end -------------------------------------------------------------------------------------------------------
TANGENTS = [(S, C, K, B) for S, C, K in HC.RESOLVE_CELLS for B in (1, 3)]


@pytest.mark.parametrize("S,C,K,B", TANGENTS, ids=cell_ids(TANGENTS))
def test_kkt_solve_tangents_with_M_against_the_dense_reference(S, C, K, B):
    """R = 3 directions over all eight inputs: the point and every tangent within SOLVE_BAR of cross_tangent_ref.dense_tangent."""
    tangents_case(S, C, K, hard(S, C, K, B), (3,), HARD)
