"""CPU suite of the box-constrained QP solve: the numpy reference (tests/box_qp_ref.py) against dense KKT solves and
scipy's SLSQP, and the C entry's presence in the header and the built library."""
import os
import re

import numpy as np
import pytest

import box_qp_ref as ref
from gato_python_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(eps_abs=1e-10, eps_rel=1e-10, max_admm_iters=20000)


@pytest.mark.parametrize("shape,seed", [((2, 1, 5), 0), ((4, 2, 12), 1), ((14, 7, 6), 2)])
def test_free_bounds_is_the_kkt_solve(shape, seed):
    s = synth.make_system(*shape, seed=seed)
    H, Cm, g, c = ref.parts(s)
    inf = np.full(s.N, np.inf)
    dz, lam = synth.dense_kkt_solve(s)
    out = ref.admm(H, Cm, g, c, -inf, inf, sigma=0.0, alpha=1.0)
    assert out["iters"] == 1 and out["status"] == ref.CONVERGED
    assert np.abs(out["x"] - dz).max() <= 1e-10 * np.abs(dz).max()
    assert np.abs(out["lam"] - lam).max() <= 1e-10 * np.abs(lam).max()
    assert not out["y"].any()


def _problems():
    s, lo, hi = ref.pendulum_box(0.2)
    yield "pendulum", s, lo, hi
    s, lo, hi, _ = ref.double_integrator(K=20, u_max=0.5, v_max=0.6)
    yield "double_integrator", s, lo, hi


@pytest.mark.parametrize("name", ["pendulum", "double_integrator"])
def test_active_bounds_reach_kkt(name):
    s, lo, hi = next((s, lo, hi) for n, s, lo, hi in _problems() if n == name)
    H, Cm, g, c = ref.parts(s)
    dz, _ = synth.dense_kkt_solve(s)
    assert np.any((dz < lo) | (dz > hi)), "the unconstrained solution must violate the box"
    out = ref.admm(H, Cm, g, c, lo, hi, **TIGHT)
    assert out["status"] == ref.CONVERGED
    kk = ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, out["z"], out["y"], out["lam"])
    assert max(kk.values()) <= 1e-7, kk
    assert np.any(out["y"] != 0), "some bound must be active"


@pytest.mark.parametrize("name", ["pendulum", "double_integrator"])
def test_objective_matches_slsqp(name):
    from scipy.optimize import minimize
    s, lo, hi = next((s, lo, hi) for n, s, lo, hi in _problems() if n == name)
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, **TIGHT)
    bounds = [(None if np.isinf(a) else a, None if np.isinf(b) else b) for a, b in zip(lo, hi)]
    res = minimize(lambda x: ref.objective(H, g, x), np.clip(np.zeros(s.N), lo, hi), jac=lambda x: H @ x - g,
                   method="SLSQP", bounds=bounds, options=dict(maxiter=2000, ftol=1e-14),
                   constraints=[dict(type="eq", fun=lambda x: Cm @ x - c, jac=lambda x: Cm)])
    assert res.success, res.message
    f_admm, f_ref = ref.objective(H, g, out["z"]), res.fun
    assert abs(f_admm - f_ref) <= 1e-6 * abs(f_ref), (f_admm, f_ref)


def test_residual_formula_and_penalties():
    lo = np.array([-np.inf, -1.0, 2.0, -np.inf, 0.0])
    hi = np.array([np.inf, 1.0, 2.0, 3.0, np.inf])
    assert np.array_equal(ref.penalties(lo, hi, 0.1), [0.0, 0.1, 100.0, 0.1, 0.1])
    s, lo, hi = ref.pendulum_box(0.2)
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, eps_abs=0.0, eps_rel=0.0, max_admm_iters=7)
    assert out["status"] == ref.MAX_ITERS and out["iters"] == 7
    rp, rd, _, _ = ref.residuals(H, Cm, g, c, out["x"], out["z"], out["y"], out["lam"])
    assert (rp, rd) == (out["res_prim"], out["res_dual"])


def test_trivial_qp_and_infeasible_box():
    s = synth.make_system(2, 1, 4, seed=3)
    H, Cm, _, _ = ref.parts(s)
    zero_g, zero_c = np.zeros(s.N), np.zeros(s.S * s.K)
    lo, hi = np.full(s.N, -1.0), np.full(s.N, 1.0)
    with np.errstate(all="ignore"):
        out = ref.admm(H, Cm, zero_g, zero_c, lo, hi)
    assert out["status"] == ref.CONVERGED and not out["x"].any()
    # x_0 pinned to c_0 = 5 outside the box [-1, 1]: no feasible point, the iteration runs out with finite values
    c = zero_c.copy()
    c[:s.S] = 5.0
    out = ref.admm(H, Cm, zero_g, c, lo, hi, max_admm_iters=200)
    assert out["status"] == ref.MAX_ITERS and all(np.isfinite(out[k]).all() for k in ("x", "z", "y", "lam"))


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("shape", [(2, 1, 5), (4, 2, 9), (14, 7, 12)])
def test_sparse_parts_are_the_dense_parts(shape):
    s = synth.make_system(*shape, seed=4, dense_q=True)
    H, Cm, g, c = ref.parts(s)
    Hs, Cs, gs, cs = ref.sparse_parts(s)
    assert ref.is_sparse(Hs) and ref.is_sparse(Cs) and not ref.is_sparse(H)
    assert np.array_equal(Hs.toarray(), H) and np.array_equal(Cs.toarray(), Cm)
    assert np.array_equal(gs, g) and np.array_equal(cs, c)


@pytest.mark.parametrize("shape", [(4, 2, 9), (14, 7, 12)])
def test_sparse_functions_equal_dense(shape):
    """residuals, qp_kkt_residuals and admm on scipy.sparse H, C against the dense path: 1e-12 relative to the larger of 1
    and the vector's infinity norm (two LU factorisations of the same matrix, ten iterations)."""
    from box_qp_polish_ref import boxes
    s = synth.make_system(*shape, seed=4, dense_q=True)
    lo, hi = boxes(s, 5)
    dense, sparse = ref.parts(s), ref.sparse_parts(s)
    kw = dict(admm_rho=10.0, eps_abs=0.0, eps_rel=0.0, max_admm_iters=10)
    a, b = ref.admm(*dense, lo, hi, **kw), ref.admm(*sparse, lo, hi, **kw)
    assert a["iters"] == b["iters"] == 10 and a["status"] == b["status"] == ref.MAX_ITERS
    for k in ("x", "z", "y", "lam"):
        assert _close(b[k], a[k]), (k, np.abs(a[k] - b[k]).max())
    pt = (a["x"], a["z"], a["y"], a["lam"])
    assert _close(ref.residuals(*sparse, *pt), ref.residuals(*dense, *pt))
    kd = ref.qp_kkt_residuals(*dense, lo, hi, a["z"], a["y"], a["lam"])
    ks = ref.qp_kkt_residuals(*sparse, lo, hi, a["z"], a["y"], a["lam"])
    assert _close([ks[k] for k in sorted(ks)], [kd[k] for k in sorted(kd)])


def test_entry_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gato_hip.h")).read()
    assert re.search(r"int\s+gato_box_qp_solve\s*\(", hdr)
    assert re.search(r"void\s+gato_box_qp_default_params\s*\(", hdr)
    assert "gato_box_qp_params" in hdr
    from gato_python_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "gato_box_qp_solve") and hasattr(L, "gato_box_qp_default_params")
    p = _lib.BoxQpParams()
    L.gato_box_qp_default_params(p)
    assert (p.admm_rho, p.sigma, p.alpha, p.eps_abs, p.eps_rel, p.max_admm_iters, p.check_every, p.warm) == \
        (0.1, 1e-6, 1.6, 1e-6, 1e-6, 4000, 25, 0)


def test_box_qp_refuses_cpu_tensors():
    import torch
    import gato_python_amd
    K, S, C = 3, 2, 1
    t = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU only"):
        gato_python_amd.box_qp(t(K, S, S), t(K - 1, C, C), t(K - 1, S, S), t(K - 1, S, C), t(K, S), t(K - 1, C), t(K, S),
                               -1.0, 1.0, -1.0, 1.0, rho=1e-3, exit_tol=1e-8, max_iters=50)
