"""CPU suite of the box QP with a cross term: that the GPU cases (tests/test_gpu_box_qp_cross.py) can
tell an iteration with M from one without, that the reference alone meets the caps the converged cases set, that the shared
problems are what they say, and the refusals of box_qp(M=...) that need no GPU."""
import numpy as np
import pytest
import torch

import box_qp_cross_ref as XR
import box_qp_ref as ref
import cross_ref as X

key_id = lambda k: "%d/%d/%d-%s" % (k[0], k[1], k[2], k[5])


# ---- M must matter -------------------------------------------------------------------------------------------------------------
def moves(key, **admm):
    """|x_M - x_0|inf over max(1, |x_M|inf) of the iterates after PARITY_ITERS x-steps with and without M."""
    a, b = XR.parity_reference(key, True, **admm), XR.parity_reference(key, False, **admm)
    return float(np.abs(a["x"] - b["x"]).max() / max(1.0, np.abs(a["x"]).max()))


@pytest.mark.parametrize("key", [k for k in XR.parity_keys() if k[2] >= 3], ids=key_id)
def test_parity_cells_tell_M_from_no_M(key):
    """The problems of the iterate-parity test, at its settings (full boxes, the default admm_rho): 25 iterations with the cross H
    and with H without M end at least 1e-6 max(1, |x|) apart - a kernel that dropped M would miss the 1e-8 parity bar by two
    orders of magnitude at the least.  (At K = 2 the difference is rounding-size on 2/1: those cells are not counted.)"""
    d = moves(key)
    print(key_id(key), "x moves by", d)
    assert d >= 1e-6, d


@pytest.mark.parametrize("cell", [c for c in XR.PARITY_CELLS if c[2] >= 3], ids=lambda c: "%d/%d/%d" % c)
def test_control_boxes_tell_M_from_no_M(cell):
    """The same on control-only boxes at admm_rho = 10, the converged cases' settings (measured 1.4e-4 .. 8.7e-2)."""
    S, C, K = cell
    d = moves((S, C, K, K, False, "controls"), admm_rho=XR.ADMM_RHO)
    print(cell, "x moves by", d)
    assert d >= 1e-6, d


# ---- the reference converges within the cap ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", XR.converged_keys(), ids=lambda k: key_id(k) + "-seed%d" % k[3])
def test_reference_converges_within_the_cap(key):
    """Control-only boxes, eps 1e-7, admm_rho 10: the reference converges within CONVERGED_CAP iterations on every converged
    cell (measured 32 .. 511), and its point is optimal for the QP with M by the algorithm-free check."""
    p = XR.problem(*key)
    out = XR.reference(key, eps_abs=1e-7, eps_rel=1e-7, admm_rho=XR.ADMM_RHO, max_admm_iters=XR.CONVERGED_CAP)
    print(key_id(key), "iters", out["iters"], "res", out["res_prim"], out["res_dual"])
    assert out["status"] == ref.CONVERGED and out["iters"] <= XR.CONVERGED_CAP, out["iters"]
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], out["x"], out["y"], out["lam"])
    sd = max(np.abs(p["H"] @ out["x"]).max(), np.abs(p["g"]).max(), 1.0)
    assert kk["stat"] <= 1e-6 * sd and kk["eq"] <= 1e-6 and kk["bound"] <= 1e-6, kk
    assert np.any(out["y"] != 0)                                            # a bound is active: the box is not decoration


# ---- the shared problems -----------------------------------------------------------------------------------------------------------
def test_problems_are_what_they_say():
    p = XR.problem(4, 2, 9, 9, False, "full")
    s, n = p["s"], 6
    assert np.array_equal(p["H"], p["H"].T) and not np.array_equal(p["H"], p["H0"])
    assert np.array_equal(p["H"][:4, 4:6], p["M"][0]) and np.array_equal(p["H0"][:4, 4:6], np.zeros((4, 2)))
    H0, Cm, g, c = ref.parts(s)                                             # the device inputs are the blocks without M
    assert np.array_equal(H0, p["H0"]) and np.array_equal(Cm, p["Cm"]) and np.array_equal(g, p["g"]) and np.array_equal(c, p["c"])
    lo, hi = p["lo"], p["hi"]
    idx = np.arange(s.N)
    assert np.isinf(lo[:4]).all() and np.isfinite(lo[(idx % n == 0) & (idx >= n)]).all()     # x_0 free, states clipped
    assert (lo == hi).sum() == 1 and np.all(lo <= hi)
    q = XR.problem(4, 2, 9, 9, False, "controls")
    assert np.isinf(q["lo"][idx % n < 4]).all() and np.isfinite(q["lo"][idx % n >= 4]).all() and not (q["lo"] == q["hi"]).any()
    k2 = XR.problem(2, 1, 2, 2, False, "full")                              # K = 2: the fixed control is knot 0's
    assert k2["lo"][2] == k2["hi"][2]
    z = XR.problem(*XR.batch_keys()[2])
    assert not z["M"].any() and np.array_equal(z["H"], z["H0"])
    assert XR.problem(*XR.batch_keys()[1])["blocks"][0][0, 0, 1] != 0       # dense Q


def test_sparse_cross_parts_equal_the_dense_ones():
    blocks, M = X.cell(4, 2, 5, seed=3)
    from gato_python_amd import synth
    s = synth.blocks_to_csr(*blocks, rho=XR.RHO)
    H, Cm, g, c = XR.cross_parts_sparse(s, M)
    Hd, Cd, gd, cd = XR.cross_parts(blocks, M)
    assert np.array_equal(H.toarray(), Hd) and np.array_equal(Cm.toarray(), Cd) and np.array_equal(g, gd) and np.array_equal(c, cd)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_box_qp_refuses_M_without_a_gpu():
    from gato_python_amd import autograd, qp
    S, C, K = 4, 2, 3
    blocks, M = X.cell(S, C, K)
    t = [torch.tensor(b) for b in blocks]
    kw = dict(rho=1e-3, exit_tol=1e-10, max_iters=100)
    box = (-1.0, 1.0, -1.0, 1.0)
    made = len(autograd._SOLVERS)
    Mt = torch.tensor(M)
    for bad in (dict(polish=True), dict(method="pdas"), dict(method="alm"), dict(method="pdas", x_soft=1.0)):
        with pytest.raises(ValueError, match=r"M needs method='admm' without polish.*DESIGN\.md section 3\.16"):
            qp.box_qp(*t, *box, M=Mt, **bad, **kw)
    with pytest.raises(ValueError, match="M has shape"):
        qp.box_qp(*t, *box, M=torch.tensor(M[:, :, :1]), **kw)
    with pytest.raises(ValueError, match="M has shape"):
        qp.box_qp(*t, *box, M=torch.tensor(M[1:]), **kw)
    with pytest.raises(ValueError, match="M has shape"):                   # a batch dimension the others lack
        qp.box_qp(*t, *box, M=torch.tensor(M[None]), **kw)
    with pytest.raises(ValueError, match="float32"):
        qp.box_qp(*t, *box, M=torch.tensor(M, dtype=torch.float32), **kw)
    with pytest.raises(ValueError, match="meta"):
        qp.box_qp(*t, *box, M=Mt.to("meta"), **kw)
    with pytest.raises(ValueError, match="torch.Tensor"):
        qp.box_qp(*t, *box, M=M, **kw)
    with pytest.raises(ValueError, match="GPU only"):                      # a well-formed M: the values' own device check
        qp.box_qp(*t, *box, M=Mt, **kw)
    assert len(autograd._SOLVERS) == made
