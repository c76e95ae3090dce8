"""CPU suite of the forward-mode sensitivities with a cross term: the formulas of
tests/cross_tangent_ref.py against central differences of the dense cross solve, the device's three-step route against the direct
one, the conditioning of every cell the GPU suite (tests/test_gpu_cross_tangent.py) uses, and the input checks of
kkt_solve_tangents(M=...) that need no GPU."""
import numpy as np
import pytest
import torch

import cross_ref as X
import cross_tangent_ref as CT

GRID = [(S, C, K, dq) for S, C in ((2, 1), (4, 2), (6, 3), (14, 7)) for K in (2, 3, 5, 9) for dq in (False, True)]
ids = lambda c: "%d/%d/%d%s" % (c[0], c[1], c[2], "-dense" if c[3] else "")
FD_BAR = 1e-6                                       # x max(1, |want|): the bar of DESIGN.md section 3.13, h = 1e-6


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("case", GRID, ids=ids)
def test_formulas_against_central_differences(case):
    """Each of the eight inputs alone and all together.  M alone at K = 2 moves only lam.: x_0 = c_0 = 0 there, so x. is exactly
    zero and says nothing; from K = 3 on the direction must move x. as well."""
    S, C, K, dq = case
    blocks, M = X.cell(S, C, K, seed=3, dense_q=dq)
    worst = 0.0
    for names in [(n,) for n in CT.NAMES] + [CT.NAMES]:
        dots = CT.random_dots(S, C, K, 11, names)
        _, _, x_dot, lam_dot = CT.dense_tangent(blocks, M, dots)
        x_fd, lam_fd = CT.central_difference(blocks, M, dots)
        for got, want in ((x_dot, x_fd), (lam_dot, lam_fd)):
            e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(e.max()))
            assert e.max() <= FD_BAR, (names, float(e.max()))
        assert np.abs(lam_dot).max() > 0, names
        if K >= 3:
            assert np.abs(x_dot).max() > 0, names
    print("worst |formula - central difference| / max(1, |want|)", worst)


@pytest.mark.parametrize("case", GRID, ids=ids)
def test_three_step_route_equals_the_direct_solve(case):
    """g' = t_g,x - W^T t_g,u, the solve of the transformed system, u. = v. - W x. against the direct dense solve: 1e-11."""
    S, C, K, dq = case
    blocks, M = X.cell(S, C, K, seed=3, dense_q=dq)
    dots = CT.random_dots(S, C, K, 12)
    _, _, x_dot, lam_dot = CT.dense_tangent(blocks, M, dots)
    x3, lam3 = CT.three_step_tangent(blocks, M, dots)
    assert rel(x3, x_dot) < 1e-11 and rel(lam3, lam_dot) < 1e-11, (rel(x3, x_dot), rel(lam3, lam_dot))


def test_scales_bound_the_terms_and_the_transform_is_cross_ref():
    """scale_i is at least |t_i| and the sum over an all-ones restatement; g' with its scale is transform_g of t_g."""
    S, C, K = 4, 2, 3
    blocks, M = X.cell(S, C, K, seed=3)
    x, lam = X.dense_solve(blocks, M)
    dots = CT.random_dots(S, C, K, 13)
    t_g, t_c, s_g, s_c = CT.tangent_rhs(x, lam, S, C, K, dots)
    assert np.all(np.abs(t_g) <= s_g) and np.all(np.abs(t_c) <= s_c) and np.all(s_g > 0)
    W = X.transform(*blocks[:6], M)["W"].astype(np.float64)
    gp, sp = CT.transform_rhs(W, t_g, s_g, S, C, K)
    assert np.array_equal(gp, X.transform_g(W, t_g, S, C, K)) and np.all(sp >= s_g) and np.all(np.abs(gp) <= sp)
    n = S + C
    assert np.array_equal(gp[S:n], t_g[S:n]) and np.array_equal(gp[(K - 1) * n:], t_g[(K - 1) * n:])
    d32 = CT.tangent_rhs(x, lam, S, C, K, dots, np.float32)[0]
    assert d32.dtype == np.float32 and rel(d32, t_g) < 1e-5


def gpu_cells():
    """Every (blocks, M, needs the dense KKT) the GPU file builds."""
    out = []
    for S, C in X.SHAPES:
        for K in CT.KERNEL_K:
            out += [(b, M, False) for b, M in CT.kernel_cells(S, C, K, 3)]
    out += [(b, M, False) for b, M in CT.kernel_cells(*X.STRIDE_CELL, 1)]
    for S, C, K in CT.SOLVE_CELLS:
        out += [(b, M, True) for b, M in CT.solve_cells(S, C, K, 3)]
    return out


def test_gpu_cells_keep_the_conditioning_limits_of_the_cross_suite():
    """tests/test_cross_cpu.py's limits: every G_k positive definite, cond(R_k + rho I) <= 1e4 on every cell, cond of the dense
    KKT <= 1e8 on every cell that is solved."""
    worst_R = worst_K = 0.0
    for blocks, M, solved in gpu_cells():
        Q, R = blocks[0], blocks[1]
        for k in range(R.shape[0]):
            assert np.linalg.eigvalsh(np.block([[Q[k], M[k]], [M[k].T, R[k]]])).min() > 0
            worst_R = max(worst_R, np.linalg.cond(R[k] + X.RHO * np.eye(R.shape[-1])))
        if solved:
            worst_K = max(worst_K, np.linalg.cond(X.dense_kkt(*blocks[:4], M)))
    print("worst cond(R + rho I)", worst_R, "worst cond(KKT)", worst_K)
    assert worst_R <= 1e4 and worst_K <= 1e8, (worst_R, worst_K)


def test_kkt_solve_tangents_checks_M_without_a_gpu():
    from gato_python_amd import autograd
    S, C, K, R = 4, 2, 3, 2
    blocks, M = X.cell(S, C, K)
    t = [torch.tensor(b) for b in blocks]
    kw = dict(rho=1e-3, exit_tol=1e-10, max_iters=100)
    qd = {"q": torch.zeros(R, K, S, dtype=torch.float64)}
    Md = torch.zeros(R, K - 1, S, C, dtype=torch.float64)
    made = len(autograd._SOLVERS)
    call = autograd.kkt_solve_tangents
    for bad in (M[:, :, :1], M[1:], M[None]):
        with pytest.raises(ValueError, match="M has shape"):
            call(*t, qd, M=torch.tensor(bad), **kw)
    with pytest.raises(ValueError, match="float32"):
        call(*t, qd, M=torch.tensor(M, dtype=torch.float32), **kw)
    with pytest.raises(ValueError, match="meta"):
        call(*t, qd, M=torch.tensor(M).to("meta"), **kw)
    with pytest.raises(ValueError, match="torch.Tensor"):
        call(*t, qd, M=M, **kw)
    with pytest.raises(ValueError, match="tangent of M needs"):
        call(*t, dict(qd, M=Md), **kw)
    with pytest.raises(ValueError, match="tangent of M has shape"):
        call(*t, dict(qd, M=Md[:, :, :, :1]), M=torch.tensor(M), **kw)
    with pytest.raises(ValueError, match="tangent of M has shape"):           # the direction axis is missing
        call(*t, dict(qd, M=Md[0]), M=torch.tensor(M), **kw)
    with pytest.raises(ValueError, match="share one R"):
        call(*t, dict(qd, M=Md[:1]), M=torch.tensor(M), **kw)
    with pytest.raises(ValueError, match="GPU only"):                        # well-formed: the values' own device check
        call(*t, dict(qd, M=Md), M=torch.tensor(M), **kw)
    assert len(autograd._SOLVERS) == made
