"""CPU suite of the hard cells of the cross-term kernels (tests/cross_hard_cells.py; DESIGN.md sections 3.15 to 3.17): that the bars
of tests/test_gpu_cross_hard.py sit far above what the references alone do on dense R_k, graded blocks and A_k far from I, that
the reference ADMM converges where the GPU file asks the device to, and that these cells see three errors which the cells of
cross_ref.batch_cells cannot see at all.

Measured while the cells were chosen (all six shapes, K in 2, 3, 5, 9, seeds 0 .. 2; grade 0 | grade 4 in fp64, 3 in fp32):
    float64 transform against longdouble, per block (W, Q'', A^')       7.4e-15 | 5.9e-15      (BLOCK_BAR 1e-11)
    cond(R_k + rho I)                                                   99.9    | 100          (cap 1e4)
    cond(dense cross KKT)                                               8.6e4   | 4.2e6        (cap 1e8)
    transformed_solve (float64) against dense_solve                     3.5e-14 | 1.7e-13      (SOLVE_BAR 1e-6)
    float32 transform against longdouble of the rounded inputs          1.7e-6  | 4.4e-6
    oracle32_solve at F32_TIGHT: iterations at exit, error              <= 65, 4.3e-5 | <= 114, 2.1e-4     (max_iters 300)
    ADMM, LU x-step against the x-step through transformed_solve        8.9e-13 | 3.7e-13      (asserted at 1e-10)"""
import numpy as np
import pytest

import asm_ref
import box_qp_cross_ref as XR
import box_qp_ref as ref
import cross_hard_cells as HC
import cross_ref as X
from oracle import c_oracle as co
from gato_python_amd import synth
from test_cross_cpu import central_differences_hold, rel
from test_gpu_cross import BLOCK_BAR, F32_TIGHT, SOLVE_BAR

LD = np.longdouble
RES_BAR = 1e-9                                    # check_converged: reported against re-evaluated residuals, x max(scale, 1)
G64, G32 = HC.GRADE["float64"], HC.GRADE["float32"]
SHAPE_K = [(S, C, K) for S, C in HC.SHAPES for K in (2, 3, 5, 9)]          # every (shape, K) of (a) .. (e) and (g)
cid = lambda c: "%d/%d/%d" % tuple(c[:3])


def cells_of(S, C, K):
    """Every (blocks, M, grade) the GPU file builds at this shape and K: seeds 0 .. 2 at the fp64 and the fp32 grade, and the
    grade-0 cell of (f) and of the central differences."""
    out = [HC.hard_cell(S, C, K, seed, g) + (g,) for g in (G64, G32) for seed in range(3)]
    if (S, C, K) in HC.CONVERGED_CELLS + HC.FD_CELLS:
        out.append(HC.hard_cell(S, C, K, 0, 0) + (0,))
    return out


def blockwise(got, want):
    return max(rel(got[k], want[k]) for k in range(want.shape[0]))


def test_every_cell_of_the_gpu_file_is_listed():
    have = set(SHAPE_K)
    for cells in (HC.SOLVE_CELLS, HC.RESOLVE_CELLS, HC.GRAD_CELLS, HC.FD_CELLS, HC.PARITY_CELLS, [HC.BATCH_CELL], HC.CONVERGED_CELLS):
        assert set(cells) <= have
    assert {(S, C, K) for S, C in HC.SHAPES for K in HC.KERNEL_K} <= have


# ---- conditioning and the references' own error ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", SHAPE_K, ids=cid)
def test_cells_are_positive_definite_and_the_references_sit_below_the_bars(cell):
    """Every G_k positive definite; cond(R_k + rho I) <= 1e4 and cond(KKT) <= 1e8, the caps of
    test_gpu_cells_are_positive_definite_and_well_conditioned; the float64 restatement of every block within BLOCK_BAR / 100 of
    the longdouble one; the transformed float64 solve within SOLVE_BAR / 100 of the dense one."""
    S, C, K = cell
    for blocks, M, grade in cells_of(S, C, K):
        Q, R, A, B, q, r, c = blocks
        assert np.abs(c[0]).max() > 0 and (C == 1 or np.abs(R[0] - np.diag(np.diag(R[0]))).max() > 0)
        for k in range(K - 1):
            assert np.linalg.eigvalsh(np.block([[Q[k], M[k]], [M[k].T, R[k]]])).min() > 0
            assert np.linalg.cond(R[k] + X.RHO * np.eye(C)) <= 1e4
        assert np.linalg.cond(X.dense_kkt(Q, R, A, B, M)) <= 1e8
        t, t64 = X.transform(Q, R, A, B, q, r, M, X.RHO, LD), X.transform(Q, R, A, B, q, r, M, X.RHO, np.float64)
        e = max(blockwise(t64[n], t[n]) for n in ("W", "Q2", "A2", "q2"))
        dz, lam = X.dense_solve(blocks, M)
        dz_t, lam_t = X.transformed_solve(blocks, M, dtype=np.float64)
        es = max(rel(dz_t, dz), rel(lam_t, lam))
        print(cid(cell), "grade", grade, "blocks %.2g solve %.2g" % (e, es))
        assert e <= BLOCK_BAR / 100 and es <= SOLVE_BAR / 100, (grade, e, es)


SOLVED = sorted(set(HC.SOLVE_CELLS + HC.RESOLVE_CELLS + HC.GRAD_CELLS))


@pytest.mark.parametrize("cell", SOLVED, ids=cid)
def test_c_oracle_solve_of_the_transformed_system_is_within_a_tenth_of_the_solve_bar(cell):
    """The PCG settings of the GPU file's fp64 whole solves (asm_ref.EXIT_TOL, MAX_ITERS; the pattern of tests/test_asm_ref_cpu.py):
    with them the C oracle's fp64 solve of the transformed system, finished, is within SOLVE_BAR / 10 of the dense cross solve
    and leaves its loop by tolerance, so a device miss at SOLVE_BAR is not the iteration's."""
    S, C, K = cell
    for seed in range(3):
        blocks, M = HC.hard_cell(S, C, K, seed, G64)
        Q, R, A, B, q, r, c = blocks
        t = X.transform(Q, R, A, B, q, r, M, X.RHO, np.float64)
        s = synth.blocks_to_csr(t["Q2"], R, t["A2"], B, t["q2"], r, c, rho=X.RHO, dense_q=True)
        lam, dzp, it = co.linsys_solve(*s.csr_args(), S, C, K, asm_ref.EXIT_TOL, asm_ref.MAX_ITERS, X.RHO, dtype=np.float64)
        dz_w, lam_w = X.dense_solve(blocks, M)
        e = max(rel(X.finish(t["W"], np.asarray(dzp), S, C, K), dz_w), rel(lam, lam_w))
        print(cid(cell), "seed", seed, "iterations", it, "error %.2g" % e)
        assert it < asm_ref.MAX_ITERS and e <= SOLVE_BAR / 10, (seed, it, e)


@pytest.mark.parametrize("cell", HC.SOLVE_CELLS, ids=cid)
def test_float32_oracle_leaves_its_loop_by_tolerance(cell):
    """Every fp32 whole-solve cell (grade 3, rounded to float32) at F32_TIGHT: cross_ref.oracle32_solve stops below max_iters, so
    the device and the restatement are both compared at rounding, not at the stop rule."""
    S, C, K = cell
    r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    for seed in range(3):
        blocks, M = HC.hard_cell(S, C, K, seed, G32)
        blocks, M = tuple(r32(b) for b in blocks), r32(M)
        dz, lam, it = X.oracle32_solve(blocks, M, F32_TIGHT["exit_tol"], F32_TIGHT["max_iters"], iters=True)
        dz_w, lam_w = X.dense_solve(blocks, M, rho=np.float64(np.float32(X.RHO)))
        print(cid(cell), "seed", seed, "iterations", it, "error %.2g" % max(rel(dz, dz_w), rel(lam, lam_w)))
        assert it < F32_TIGHT["max_iters"], (seed, it)


@pytest.mark.parametrize("cell", HC.FD_CELLS, ids=cid)
def test_analytic_gradients_match_central_differences_on_hard_cells(cell):
    """cross_ref.dense_reference's eight gradients on dense R_k and A_k far from I (grade 0: a central difference of step 1e-5
    wants blocks of one scale), at the bar of test_analytic_gradients_match_central_differences."""
    central_differences_hold(*HC.hard_cell(*cell, 0, 0))


# ---- the box QPs -----------------------------------------------------------------------------------------------------------------
def x_step_through_the_transform(p):
    """A stand-in for box_qp_ref.kkt_solver on problem p: the x-step matrix H + diag(d) solved by the change of variables
    (cross_ref.transformed_solve on the blocks with d added to the diagonals of Q_k and R_k) - the device's order."""
    Q, R, A, B, q, r, c = p["blocks"]
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    n, N = S + C, p["s"].N

    def kkt_solver(H, Cm, diag=None):
        d = np.broadcast_to(diag, (N,))
        Qd, Rd = Q.copy(), R.copy()
        for k in range(K):
            Qd[k] += np.diag(d[k * n:k * n + S])
            if k < K - 1:
                Rd[k] += np.diag(d[k * n + S:(k + 1) * n])
        return lambda rhs: np.concatenate(X.transformed_solve((Qd, Rd, A, B, q, r, c), p["M"], X.RHO, np.float64, g=rhs[:N], c=rhs[N:]))
    return kkt_solver


@pytest.mark.parametrize("key", HC.parity_keys() + HC.batch_keys()[1:], ids=lambda k: cid(k) + "-seed%d" % k[3])
def test_the_two_admm_orders_agree_and_the_box_is_active(key, monkeypatch):
    """PARITY_ITERS iterations at eps 0 and admm_rho = 10: the reference with LU x-steps and with x-steps through the change of
    variables agree within 1e-10 in x, z, y and lam (measured 8.9e-13), a hundredth of the device's 1e-8; the iterate has
    y != 0 and z != x."""
    p = HC.problem(*key)
    want = HC.parity_reference(key)
    admm = dict(eps_abs=0.0, eps_rel=0.0, max_admm_iters=XR.PARITY_ITERS, admm_rho=XR.ADMM_RHO)
    monkeypatch.setattr(ref, "kkt_solver", x_step_through_the_transform(p))
    got = ref.admm(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], **admm)
    e = max(float(np.abs(got[k] - want[k]).max() / max(np.abs(want[k]).max(), 1.0)) for k in ("x", "z", "y", "lam"))
    print(cid(key), "orders apart by %.2g" % e)
    assert e <= 1e-10, e
    assert np.any(want["y"] != 0) and np.any(want["z"] != want["x"])


@pytest.mark.parametrize("shape", HC.SHAPES, ids=lambda s: "%d/%d" % s)
def test_a_control_of_every_full_knot_is_at_a_bound_on_some_cell(shape):
    """From the reference alone: on some parity cell of each shape, with and without M, every full knot has a control whose z
    sits on a bound after PARITY_ITERS iterations - the clip of a control row is exercised at every knot position."""
    for with_M in (True, False):
        hits = [HC.knots_with_a_control_at_a_bound(HC.parity_reference(k, with_M), HC.problem(*k)) for k in HC.parity_keys() if k[:2] == shape]
        print(shape, with_M, [int(h.sum()) for h in hits])
        assert any(h.all() for h in hits)


CONVERGED = [(k, 1e-7) for k in HC.converged_keys()] + [(k, 1e-4) for k in HC.converged_keys("float32")]


@pytest.mark.parametrize("key,eps", CONVERGED, ids=lambda v: cid(v) + "-" + v[7] if isinstance(v, tuple) else None)
def test_reference_converges_within_the_cap(key, eps):
    """Grade 0, control-only boxes, admm_rho = 10: the reference converges within CONVERGED_CAP iterations at eps 1e-7 on the
    fp64 cells (measured 95, 720, 151, 177) and at eps 1e-4 on the float32-rounded inputs of the fp32 cells (51, 312: both stay
    in the GPU file); its point is optimal for the QP with M to ten times eps and a bound is active."""
    p = HC.problem(*key)
    out = HC.reference(key, eps_abs=eps, eps_rel=eps, admm_rho=XR.ADMM_RHO, max_admm_iters=XR.CONVERGED_CAP)
    print(cid(key), key[7], "iters", out["iters"], "res", out["res_prim"], out["res_dual"])
    assert out["status"] == ref.CONVERGED and out["iters"] <= XR.CONVERGED_CAP, out["iters"]
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], out["x"], out["y"], out["lam"])
    sd = max(np.abs(p["H"] @ out["x"]).max(), np.abs(p["g"]).max(), 1.0)
    assert kk["stat"] <= 10 * eps * sd and kk["eq"] <= 10 * eps * max(np.abs(out["x"]).max(), 1.0) and kk["bound"] <= 10 * eps, kk
    assert np.any(out["y"] != 0)


# ---- wrong on purpose -------------------------------------------------------------------------------------------------------------
def transform_wrong(blocks, M, how):
    """cross_ref.transform's W, Q'', A^' in longdouble with one error.  "diag": the off-diagonals of R_k + rho I dropped before
    the inverse; "RiT": the C x C factor (R_k + rho I)^-1 transposed; "MT": M_k's S x C array read as C x S (the other factor's
    index slip); None: no error - the bits of cross_ref.transform."""
    Q, R, A, B, q, r, M = (np.asarray(t).astype(LD) for t in blocks[:6] + (M,))
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    W, Q2, A2 = np.zeros((K - 1, C, S), LD), Q.copy(), A.copy()
    for k in range(K - 1):
        Rr = R[k] + LD(X.RHO) * np.eye(C, dtype=LD)
        Ri = X.gj_inverse(np.diag(np.diag(Rr)) if how == "diag" else Rr)
        W[k] = (Ri.T if how == "RiT" else Ri) @ (M[k].reshape(C, S) if how == "MT" else M[k].T)
        Q2[k] = Q[k] - M[k] @ W[k]
        A2[k] = A[k] - B[k] @ W[k]
    return dict(W=W, Q2=Q2, A2=A2)


# res_dual is a maximum over all rows: after PARITY_ITERS iterations at eps 0 it is still O(1 .. 10), and where a state row holds
# it and stays above the wrong control rows, the wrong R row does not move it.  Of the 15 parity cells with C > 1 that is this one
# (res_dual 8.54 either way); the other fourteen move by 1.7 to 770.  The converged cells of (f) have no such blind spot: res_dual
# is below 1e-5 there and a wrong control row is O(1).
MAX_ELSEWHERE = {(4, 2, 3)}


def H_without_R_off_diagonals(H, S, C, K):
    """H with the off-diagonal entries of every R_k zeroed: what the control rows of H x would use."""
    out, n = H.copy(), S + C
    for k in range(K - 1):
        u = slice(k * n + S, (k + 1) * n)
        out[u, u] = np.diag(np.diag(H[u, u]))
    return out


@pytest.mark.parametrize("cell", SHAPE_K, ids=cid)
def test_hard_cells_see_what_the_old_cells_cannot(cell):
    """Three restatements wrong on purpose: R_k's off-diagonals dropped before the inverse, M_k read transposed in the product
    that builds W_k, and R's off-diagonals dropped on the control rows of H x.  On every hard cell with C > 1 each misses its GPU
    bar (BLOCK_BAR per block; the res_dual bar 1e-9 max(scale, 1), but for MAX_ELSEWHERE) by a factor of 100 or more.  On the cells of
    cross_ref.batch_cells the two that touch R are exactly the right restatement - R_k is diagonal there.

    Two limits of the mathematics, asserted as they are.  With C = 1 (shape 2/1) R_k is a number: it has no off-diagonal and no
    transpose, and all three wrong restatements are the right one, bit for bit, on any cell.  And the C x C factor of W_k is
    (R_k + rho I)^-1, the inverse of a symmetric matrix: transposing it changes W_k by rounding at the most on ANY input (asserted
    at BLOCK_BAR / 100), so that slip is not an error a test can see or a kernel can make; the transposition that is one is that
    of the other factor, M_k^T, and that is the one held to the factor of 100 here."""
    S, C, K = cell
    for blocks, M, grade in cells_of(S, C, K):
        right = X.transform(*blocks[:6], M, X.RHO, LD)
        same = transform_wrong(blocks, M, None)
        assert all(np.array_equal(same[n], right[n]) for n in same)
        for how in ("diag", "RiT", "MT"):
            wrong = transform_wrong(blocks, M, how)
            e = {n: blockwise(wrong[n], right[n]) for n in wrong}
            if C == 1:
                assert max(e.values()) == 0.0, (how, e)
            elif how == "RiT":
                assert max(e.values()) <= BLOCK_BAR / 100, (how, e)
            else:
                assert min(e["W"], e["Q2"], e["A2"]) >= 100 * BLOCK_BAR, (how, grade, e)
    key = (S, C, K, 0, G64, "full")
    if key in HC.parity_keys():
        p, out = HC.problem(*key), HC.parity_reference(key)
        args = (p["Cm"], p["g"], p["c"], out["x"], out["z"], out["y"], out["lam"])
        (_, rd, _, sd), (_, rd_w, _, _) = ref.residuals(p["H"], *args), ref.residuals(H_without_R_off_diagonals(p["H"], S, C, K), *args)
        print(cid(cell), "res_dual %.3g, without R's off-diagonals %.3g, bar %.3g" % (rd, rd_w, RES_BAR * max(sd, 1.0)))
        assert rd_w == rd if C == 1 or cell in MAX_ELSEWHERE else abs(rd_w - rd) >= 100 * RES_BAR * max(sd, 1.0)
    key = (S, C, K, 0, 0, "controls", False, "float64")
    if key in HC.converged_keys():
        p, out = HC.problem(*key), HC.reference(key, eps_abs=1e-7, eps_rel=1e-7, admm_rho=XR.ADMM_RHO, max_admm_iters=XR.CONVERGED_CAP)
        args = (p["Cm"], p["g"], p["c"], out["x"], out["z"], out["y"], out["lam"])
        (_, rd, _, sd), (_, rd_w, _, _) = ref.residuals(p["H"], *args), ref.residuals(H_without_R_off_diagonals(p["H"], S, C, K), *args)
        print(cid(cell), "converged: res_dual %.3g, without R's off-diagonals %.3g" % (rd, rd_w))
        assert rd_w == rd if C == 1 else abs(rd_w - rd) >= 100 * RES_BAR * max(sd, 1.0)
    # the old cells: diagonal R_k, so the errors that touch R change nothing at all
    for blocks, M in X.batch_cells(S, C, K, 3, seed=K):
        right = X.transform(*blocks[:6], M, X.RHO, LD)
        for how in ("diag", "RiT"):
            wrong = transform_wrong(blocks, M, how)
            assert all(np.array_equal(wrong[n], right[n]) for n in wrong), how
        H = XR.cross_parts(blocks, M)[0]
        assert np.array_equal(H_without_R_off_diagonals(H, S, C, K), H)
