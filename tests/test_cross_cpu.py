"""CPU suite of the stage-cost cross term: the mathematics of the change of variables and of the
gradients on dense solves, the conditioning of every cell the GPU suite (tests/test_gpu_cross.py) uses, and the input checks
of kkt_solve(M=...) that need no GPU."""
import numpy as np
import pytest
import torch

import cross_ref as X
import kkt_grad_ref
from gato_python_amd import synth

GRID = [(S, C, K, dq) for S, C in X.SHAPES for K in (2, 3, 5) for dq in (False, True)]
ids = lambda c: "%d/%d/%d%s" % (c[0], c[1], c[2], "-dense" if c[3] else "")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("case", GRID, ids=ids)
def test_transformed_solve_equals_the_direct_dense_solve(case):
    """Transform, block-diagonal dense solve, finish (all float64) against the dense solve with M and M^T in place: 1e-11."""
    S, C, K, dq = case
    blocks, M = X.cell(S, C, K, seed=3, dense_q=dq)
    dz, lam = X.dense_solve(blocks, M)
    dz_t, lam_t = X.transformed_solve(blocks, M, dtype=np.float64)
    assert rel(dz_t, dz) < 1e-11 and rel(lam_t, lam) < 1e-11, (rel(dz_t, dz), rel(lam_t, lam))
    rng = np.random.default_rng(4)                                      # another right-hand side through the stored W
    g, c = rng.standard_normal(dz.size), rng.standard_normal(lam.size)
    dz2, lam2 = X.dense_solve(blocks, M, g=g, c=c)
    dz2_t, lam2_t = X.transformed_solve(blocks, M, dtype=np.float64, g=g, c=c)
    assert rel(dz2_t, dz2) < 1e-11 and rel(lam2_t, lam2) < 1e-11


@pytest.mark.parametrize("case", GRID, ids=ids)
def test_analytic_gradients_match_central_differences(case):
    """<grad, D> of every input against the central difference of the dense solve, the bar of tests/test_gpu_kkt_grad.py:
    1e-6 max(|an|, 1).  Q and R directions symmetric; M_k and M_k^T move together (M enters the matrix twice)."""
    S, C, K, dq = case
    central_differences_hold(*X.cell(S, C, K, seed=5, dense_q=dq))


def central_differences_hold(blocks, M):
    """The assertion of test_analytic_gradients_match_central_differences on one system (tests/test_cross_hard_cpu.py runs it on
    dense, graded cells)."""
    K, S, C = M.shape[0] + 1, M.shape[1], M.shape[2]
    rng = np.random.default_rng(6)
    N, SK = (S + C) * K - C, S * K
    w1, w2 = rng.standard_normal(N), rng.standard_normal(SK)
    an = X.dense_reference(blocks, M, w1, w2)
    names = ("Q", "R", "A", "B", "q", "r", "c", "M")
    ops = list(blocks) + [M]
    eps = 1e-5
    for i, name in enumerate(names):
        D = rng.standard_normal(ops[i].shape)
        if name in ("Q", "R"):
            D = 0.5 * (D + np.swapaxes(D, 1, 2))

        def L(sign):
            p = [t.copy() for t in ops]
            p[i] = p[i] + sign * eps * D
            dz, lam = X.dense_solve(tuple(p[:7]), p[7])
            return float(dz @ w1 + lam @ w2)
        fd = (L(1) - L(-1)) / (2 * eps)
        got = float((an[name] * D).sum())
        assert abs(fd - got) <= 1e-6 * max(abs(got), 1.0), (name, fd, got)


def gpu_cells():
    """Every (blocks, M, needs the dense KKT) the GPU file builds."""
    out = []
    for S, C in X.SHAPES:
        for K in X.KERNEL_K:
            out += [(b, M, K <= 5) for b, M in X.batch_cells(S, C, K, 3, seed=K)]
        for K in X.GRAD_K:
            out += [(b, M, True) for b, M in X.batch_cells(S, C, K, 3, seed=40 + K)]
    out += [(b, M, False) for b, M in X.batch_cells(*X.STRIDE_CELL, 1, seed=7)]
    for S, C, K in X.SOLVE_CELLS:
        out += [(b, M, True) for b, M in X.batch_cells(S, C, K, 3, seed=20 + K)]
    for S, C, K in X.RESOLVE_CELLS + X.GRADCHECK_CELLS:
        out += [(b, M, True) for b, M in X.batch_cells(S, C, K, 3, seed=30 + K)]
    return out


def test_gpu_cells_are_positive_definite_and_well_conditioned():
    """make_cross keeps every G_k positive definite (and Q_k - M_k R_k^-1 M_k^T >= (1 - scale^2) Q_k); cond(R_k + rho I) <= 1e4 on
    every cell and cond of the dense KKT <= 1e8 on every cell that is solved (the 8197-knot cell only runs the per-knot
    kernels, whose error depends on the blocks alone), so the fp64 bars of the GPU file sit far above the rounding of its
    references: 1e-11 against eps cond(R) ~ 1e-12, 1e-6 against eps cond(KKT) ~ 1e-8."""
    worst_R = worst_K = 0.0
    for blocks, M, solved in gpu_cells():
        Q, R = blocks[0], blocks[1]
        for k in range(M.shape[0]):
            Gk = np.block([[Q[k], M[k]], [M[k].T, R[k]]])
            assert np.linalg.eigvalsh(Gk).min() > 0
            Sch = Q[k] - M[k] @ np.linalg.solve(R[k], M[k].T)
            assert np.linalg.eigvalsh(Sch - 0.75 * Q[k]).min() > -1e-9 * np.abs(Q[k]).max()
            worst_R = max(worst_R, np.linalg.cond(R[k] + X.RHO * np.eye(R.shape[-1])))
        if solved and Q.shape[0] > 1:
            worst_K = max(worst_K, np.linalg.cond(X.dense_kkt(*blocks[:4], M)))
    assert worst_R <= 1e4 and worst_K <= 1e8, (worst_R, worst_K)


def test_make_cross_is_seeded_and_scaled():
    Q, R = synth.make_blocks(6, 3, 4, seed=1, dense_q=True)[:2]
    a, b = synth.make_cross(Q, R, seed=2), synth.make_cross(Q, R, seed=2)
    assert a.shape == (3, 6, 3) and np.array_equal(a, b) and not np.array_equal(a, synth.make_cross(Q, R, seed=3))
    assert np.allclose(synth.make_cross(Q, R, seed=2, scale=0.25), 0.5 * a)
    for k in range(3):                                                     # the spectral norm of L_Q^-1 M L_R^-T is the scale
        Z = np.linalg.solve(np.linalg.cholesky(Q[k]), a[k]) @ np.linalg.inv(np.linalg.cholesky(R[k])).T
        assert abs(np.linalg.norm(Z, 2) - 0.5) < 1e-12


def test_grad_M_is_the_sum_of_both_positions():
    """M_bar = the gradient of the (x, u) block plus the transpose of the gradient of the (u, x) block of -a dz^T (the
    unsymmetrised matrix gradient of a linear solve)."""
    S, C, K = 4, 2, 3
    rng = np.random.default_rng(0)
    N = (S + C) * K - C
    dz, a = rng.standard_normal(N), rng.standard_normal(N)
    full = -np.outer(a, dz)
    got = X.grad_M(dz, a, S, C, K)
    n = S + C
    for k in range(K - 1):
        x, u = slice(k * n, k * n + S), slice(k * n + S, (k + 1) * n)
        assert np.allclose(got[k], full[x, u] + full[u, x].T, rtol=0, atol=1e-15)
    assert kkt_grad_ref.grads_math(dz, np.zeros(S * K), a, np.zeros(S * K), S, C, K)["Q"].shape == (K, S, S)


def test_kkt_solve_checks_M_without_a_gpu():
    from gato_python_amd import autograd
    S, C, K = 4, 2, 3
    blocks, M = X.cell(S, C, K)
    t = [torch.tensor(b) for b in blocks]
    kw = dict(rho=1e-3, exit_tol=1e-10, max_iters=100)
    made = len(autograd._SOLVERS)
    with pytest.raises(ValueError, match="M has shape"):
        autograd.kkt_solve(*t, M=torch.tensor(M[:, :, :1]), **kw)
    with pytest.raises(ValueError, match="M has shape"):
        autograd.kkt_solve(*t, M=torch.tensor(M[1:]), **kw)
    with pytest.raises(ValueError, match="M has shape"):                   # a batch dimension the others lack
        autograd.kkt_solve(*t, M=torch.tensor(M[None]), **kw)
    with pytest.raises(ValueError, match="float32"):
        autograd.kkt_solve(*t, M=torch.tensor(M, dtype=torch.float32), **kw)
    with pytest.raises(ValueError, match="meta"):
        autograd.kkt_solve(*t, M=torch.tensor(M).to("meta"), **kw)
    with pytest.raises(ValueError, match="torch.Tensor"):
        autograd.kkt_solve(*t, M=M, **kw)
    with pytest.raises(ValueError, match="GPU only"):                      # a well-formed M: the values' own device check
        autograd.kkt_solve(*t, M=torch.tensor(M), **kw)
    assert len(autograd._SOLVERS) == made
