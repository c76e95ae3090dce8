"""CPU suite of the box-QP polish: the numpy reference tests/box_qp_polish_ref.py against algorithm-free
optimality checks, scipy's SLSQP and central finite differences of the dense QP solution, and the C entries' presence in the
header and the built library."""
import os
import re

import numpy as np
import pytest

import box_qp_polish_ref as P
import box_qp_ref as ref
import kkt_grad_ref as kgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def exact(name):
    if name not in _CACHE:
        _CACHE[name] = P.exact_active(name)
    return _CACHE[name]


def test_active_set_rule():
    lo = np.array([-np.inf, -np.inf, -1.0, -1.0, -1.0, 0.5, -1.0, -np.inf])
    hi = np.array([np.inf, np.inf, 1.0, 1.0, 1.0, 0.5, 1.0, np.inf])
    z = np.array([9.0, 0.0, 1.0, -1.0, 0.2, 0.5, 0.99, 3.0])
    y = np.array([5.0, 0.0, 0.3, -0.3, 0.0, 0.0, 0.001, -7.0])
    # S = 1: coordinate 0 is the state of x_0 - never active whatever z, y say
    assert P.active_set(z, y, lo, hi, 1).tolist() == [0, 0, 1, -1, 0, -1, 0, 0]
    assert P.active_set(z, y, lo, hi, 1).dtype == np.int8


@pytest.mark.parametrize("name", P.PROBLEMS)
def test_reduced_solve_is_optimal(name):
    """The reference's reduced solve from the exact active set is a KKT point (the bar of test_box_qp_cpu's
    test_active_bounds_reach_kkt) whose objective matches SLSQP to 1e-6 relative (that of test_objective_matches_slsqp).
    SLSQP stops at ftol 1e-12: on the 1043 variables of 14/7/50 its line search cannot resolve 1e-14 and ends in
    "Positive directional derivative"; 1e-12 is still six orders below the bar."""
    from scipy.optimize import minimize
    act, H, Cm, g, c, lo, hi = exact(name)
    x, y, lam = P.reduced_solve(H, Cm, g, c, lo, hi, act)
    kk = ref.qp_kkt_residuals(H, Cm, g, c, lo, hi, x, y, lam)
    print(name, kk)
    assert max(kk.values()) <= 1e-7, kk
    A = act != 0
    assert A.any() and np.array_equal(x[A], P.bound_values(act, lo, hi)[A])
    bounds = [(None if np.isinf(a) else a, None if np.isinf(b) else b) for a, b in zip(lo, hi)]
    res = minimize(lambda v: ref.objective(H, g, v), np.clip(np.zeros(len(g)), lo, hi), jac=lambda v: H @ v - g,
                   method="SLSQP", bounds=bounds, options=dict(maxiter=2000, ftol=1e-12),
                   constraints=[dict(type="eq", fun=lambda v: Cm @ v - c, jac=lambda v: Cm)])
    assert res.success, res.message
    f_pol, f_ref = ref.objective(H, g, x), res.fun
    print(name, f_pol, f_ref)
    assert abs(f_pol - f_ref) <= 1e-6 * abs(f_ref), (f_pol, f_ref)


@pytest.mark.parametrize("name,its,decision", [
    ("pendulum", 1, P.REJECTED), ("pendulum", 5, P.REJECTED), ("pendulum", 10, P.ACCEPTED), ("pendulum", 25, P.ACCEPTED),
    ("pendulum", 50, P.ACCEPTED), ("6_3_20", 100, P.REJECTED), ("6_3_20", 1200, P.ACCEPTED)])
def test_reference_decisions(name, its, decision):
    """The polish decisions the GPU tests rely on: the pendulum's early guesses are rejected on the multiplier sign alone
    (their polished residuals are at rounding level), 6/3/20 after 100 iterations on the bound violation."""
    s, lo, hi, arho = P.problem(name)
    H, Cm, g, c = ref.parts(s)
    out = ref.admm(H, Cm, g, c, lo, hi, admm_rho=arho, eps_abs=0.0, eps_rel=0.0, max_admm_iters=its)
    p = P.polish(H, Cm, g, c, lo, hi, out["z"], out["y"], s.S)
    print(name, its, p["decision"], p["res_prim"], p["res_dual"])
    assert p["decision"] == decision
    if name == "pendulum" and decision == P.REJECTED:
        assert max(p["res_prim"], p["res_dual"]) <= 1e-12
    if name == "6_3_20" and decision == P.REJECTED:
        assert p["res_prim"] > 1e-2


def _inputs(name):
    """Math-shaped inputs of a problem (blocks without rho, bounds split into states and controls) and rho."""
    s, lo, hi, _ = P.problem(name)
    Q, R, A, B, q, r, c = kgr.blocks_of(s)
    xl, ul = P.split_states_controls(lo, s.S, s.C, s.K)
    xh, uh = P.split_states_controls(hi, s.S, s.C, s.K)
    return dict(Q=Q, R=R, A=A, B=B, q=q, r=r, c=c, x_lo=xl, x_hi=xh, u_lo=ul, u_hi=uh), s


def _solve(inp, rho, act):
    H, Cm, g, c = P.dense_from_blocks(inp["Q"], inp["R"], inp["A"], inp["B"], inp["q"], inp["r"], inp["c"], rho)
    S, C, K = inp["Q"].shape[1], inp["R"].shape[-1], inp["Q"].shape[0]
    lo = ref.dz_layout(inp["x_lo"], inp["u_lo"], S, C, K)
    hi = ref.dz_layout(inp["x_hi"], inp["u_hi"], S, C, K)
    x, y, lam = P.reduced_solve(H, Cm, g, c, lo, hi, act)
    return x, y, lam, lo, hi


def _same_active_set(x, y, lo, hi, act):
    """act is the exact active set of the solved problem: free coordinates strictly inside their bounds, every active
    multiplier strictly of its sign (lo == hi: any sign)."""
    F, eq = act == 0, lo == hi
    inside = np.all((x[F] > lo[F]) & (x[F] < hi[F]))
    signs = np.all(y[(act > 0) & ~eq] > 0) and np.all(y[(act < 0) & ~eq] < 0)
    return bool(inside and signs)


FD_STEP = 1e-6
# relative accuracy of an fp64 dense solve of these KKT systems (fp64 rounding times condition numbers up to ~1e3): each evaluation of L carries
# an error of about FD_ROUND |xbar| . |x| + |lambar| . |lam|, which a central difference divides by the step
FD_ROUND = 1e-13


@pytest.mark.parametrize("name", P.PROBLEMS)
def test_gradients_match_finite_differences(name):
    """The reference gradients of L = xbar . x + lambar . lam for all eleven inputs against central differences along a
    random direction per input (Q, R symmetric: their gradients are for symmetric perturbations).  Every perturbed problem
    must keep the active set - a condition on the inputs, asserted.  The bound: 1e-6 relative to the directional
    derivative's scale (the truncation error of a step of 1e-6 is far below it) plus the rounding error of the two
    evaluations divided by the step (FD_ROUND)."""
    inp, s = _inputs(name)
    act, H0, C0, g0, c0, lo0, hi0 = exact(name)
    H, Cm, g, c = P.dense_from_blocks(*(inp[k] for k in ("Q", "R", "A", "B", "q", "r", "c")), s.rho)
    assert np.abs(H - H0).max() <= 1e-12 * np.abs(H0).max() and np.array_equal(Cm, C0)
    assert np.array_equal(g, g0) and np.array_equal(c, c0)
    rng = np.random.default_rng(7)
    x, y, lam, lo, hi = _solve(inp, s.rho, act)
    assert _same_active_set(x, y, lo, hi, act)
    xbar, lambar = rng.standard_normal(len(x)), rng.standard_normal(len(lam))
    gr = P.grads(H, Cm, act, x, lam, xbar, lambar, s.S, s.C, s.K)
    assert not gr["a"][act != 0].any()
    L = lambda xx, ll: float(xbar @ xx + lambar @ ll)
    lmag = float(np.abs(xbar) @ np.abs(x) + np.abs(lambar) @ np.abs(lam))
    for key in ("Q", "R", "A", "B", "q", "r", "c", "x_lo", "x_hi", "u_lo", "u_hi"):
        V = rng.standard_normal(inp[key].shape)
        if key in ("Q", "R"):
            V = 0.5 * (V + np.swapaxes(V, -1, -2))
        partner = None
        if key in ("x_lo", "x_hi", "u_lo", "u_hi"):
            V = np.where(np.isfinite(inp[key]), V, 0.0)
            eq = inp[key[0] + "_lo"] == inp[key[0] + "_hi"]
            if key.endswith("_hi"):
                V = np.where(eq, 0.0, V)                 # where lo == hi the gradient goes to lo ...
            else:
                partner = (key[0] + "_hi", np.where(eq, V, 0.0))   # ... for a shift of both bounds together
        vals = []
        for sgn in (1.0, -1.0):
            pert = dict(inp)
            pert[key] = inp[key] + sgn * FD_STEP * V
            if partner is not None:
                pert[partner[0]] = inp[partner[0]] + sgn * FD_STEP * partner[1]
            xp, yp, lp, lop, hip = _solve(pert, s.rho, act)
            assert _same_active_set(xp, yp, lop, hip, act), (key, sgn)
            vals.append(L(xp, lp))
        fd = (vals[0] - vals[1]) / (2 * FD_STEP)
        an = float(np.sum(gr[key] * V))
        tol = 1e-6 * max(1.0, float(np.sum(np.abs(gr[key] * V)))) + FD_ROUND * lmag / FD_STEP
        print(name, key, an, fd, abs(an - fd), tol)
        assert abs(an - fd) <= tol, (key, an, fd, tol)


# ---- sparse references, constructed problems and the reduced stage path (tests/test_gpu_qp_kernel_sweep.py) ---------------
def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("shape", [(4, 2, 9), (14, 7, 12)])
def test_sparse_functions_equal_dense(shape):
    """reduced_solve, polish, adjoint and bound_grads on scipy.sparse H, C against the dense path, on a constructed problem
    (active states included): 1e-12 relative to the larger of 1 and the vector's infinity norm."""
    p = P.constructed(*shape)[0]
    dense = (p["H"], p["Cm"], p["g"], p["c"])
    sparse = ref.sparse_parts(p["s"])
    lo, hi, act = p["lo"], p["hi"], p["act"]
    rd, rs = P.reduced_solve(*dense, lo, hi, act), P.reduced_solve(*sparse, lo, hi, act)
    for a, b in zip(rs, rd):
        assert _close(a, b, 1e-12)
    assert np.array_equal(rs[0][act != 0], rd[0][act != 0])
    zero = np.zeros(len(act))
    pd, ps = (P.polish(*parts, lo, hi, zero, zero, p["s"].S, act=act) for parts in (dense, sparse))
    assert pd["decision"] == ps["decision"] == P.ACCEPTED
    rng = np.random.default_rng(1)
    xbar, lbar = rng.standard_normal(len(act)), rng.standard_normal(len(p["c"]))
    ad, as_ = P.adjoint(dense[0], dense[1], act, xbar, lbar), P.adjoint(sparse[0], sparse[1], act, xbar, lbar)
    for a, b in zip(as_, ad):
        assert _close(a, b, 1e-12)
    assert not ad[0][act != 0].any() and not as_[0][act != 0].any()
    bd, bs = P.bound_grads(dense[0], dense[1], act, xbar, *ad), P.bound_grads(sparse[0], sparse[1], act, xbar, *ad)
    for a, b in zip(bs, bd):
        assert _close(a, b, 1e-12)


def _sweep_cases():
    short = [(S, C, K, "f64") for S, C in P.SWEEP_SHAPES for K in P.SWEEP_SHORT_K]
    return short + [(S, C, K, "f32") for S, C, K in P.SWEEP_F32]


def _check_constructed(p):
    """A constructed problem against its own conditions: the seed rule, the reference's polish, a KKT point of the QP to
    1e-9, and the shape of its active set."""
    s, act, lo, hi = p["s"], p["act"], p["lo"], p["hi"]
    ok, fig = P.meets_seed_rule(p, cond=not ref.is_sparse(p["H"]))
    assert ok, fig
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], lo, hi, p["x"], p["y"], p["lam"])
    assert max(kk.values()) <= 1e-9, kk
    n = s.S + s.C
    knot, var = np.arange(s.N) // n, np.arange(s.N) % n
    on = act != 0
    assert on.any() and not on[:s.S].any()
    assert np.all(np.isfinite(P.bound_values(act, lo, hi)[on]))
    assert np.array_equal(act[lo == hi], np.full(int((lo == hi).sum()), -1))
    if s.K >= 3 and not ref.is_sparse(p["H"]):
        assert (on & (var < s.S) & (knot == 1)).any() and (on & (var < s.S) & (knot == s.K - 1)).any()
        assert (lo == hi).sum() == (1 if s.C >= 2 else 0)
    return fig


@pytest.mark.parametrize("S,C,K,kind", _sweep_cases())
def test_constructed_problem_meets_its_conditions(S, C, K, kind):
    """The seed rule finds a seed below 20 for every case of the GPU sweep (printed), and the problem of that seed is what
    it claims to be.  The fp32 cases add the condition that the fp32 restatement of the rounded problem is accepted."""
    found = P.constructed(S, C, K, extra=P.f32_ok, tag="f32") if kind == "f32" else P.constructed(S, C, K)
    assert len(found) == 1, "no seed below 20 meets the rule"
    p = found[0]
    print("seed", (S, C, K, kind), p["seed"], p["figures"])
    _check_constructed(p)
    if kind == "f32":
        q = P.rounded(p)
        assert P.f32_ok(p) and P.restatement_accepted(q, np.float32, P.F32_EPS)[0]
        assert max(ref.qp_kkt_residuals(q["H"], q["Cm"], q["g"], q["c"], q["lo"], q["hi"], q["x"], q["y"], q["lam"]).values()) <= 1e-9


def test_constructed_batch_and_long_horizon_seeds():
    S, C, K, B = P.SWEEP_BATCH
    found = P.constructed(S, C, K, count=B)
    assert len(found) == B and len({p["seed"] for p in found}) == B
    print("batch seeds", [p["seed"] for p in found])
    for p in found:
        _check_constructed(p)
    found = P.constructed(*P.SWEEP_LONG, **P.LONG_KNOBS)
    assert len(found) == 1
    p = found[0]
    print("long-horizon seed", p["seed"], p["figures"], "active", int((p["act"] != 0).sum()))
    _check_constructed(p)
    n = P.SWEEP_LONG[0] + P.SWEEP_LONG[1]
    assert (np.flatnonzero(p["act"]) // n >= 8192).any()


@pytest.mark.parametrize("S,C", P.SWEEP_SHAPES)
def test_wrong_sign_is_rejected_by_the_reference(S, C):
    p = P.constructed(S, C, 9)[0]
    flipped, j = P.wrong_sign(p)
    assert j % (S + C) >= S and p["lo"][j] != p["hi"][j] and flipped[j] == -p["act"][j] != 0
    zero = np.zeros(len(flipped))
    dec = P.polish(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], zero, zero, S, act=flipped)
    print((S, C), j, dec["decision"], dec["res_prim"], dec["res_dual"])
    assert dec["decision"] == P.REJECTED


@pytest.mark.parametrize("S,C,K,kind", [c for c in _sweep_cases() if c[3] == "f64"])
def test_reduced_stage_path_is_the_reduced_solve(S, C, K, kind):
    """reduced_stage_solve in fp64 - masked Gauss-Jordan inverses, shifted right-hand sides, Schur complement, PCG, dz -
    against the dense LU of the reduced matrix: two different routes to one point.  Bar: 1e-9 of the larger of 1 and the
    vector's infinity norm (the multipliers of these problems reach 5e3; the matrices' condition numbers 1e8)."""
    p = P.constructed(S, C, K)[0]
    x, lam, iters = P.reduced_stage_solve(p["s"], p["lo"], p["hi"], p["act"], np.float64, exit_tol=1e-30)
    ex = np.abs(x - p["x"]).max() / max(1.0, np.abs(p["x"]).max())
    el = np.abs(lam - p["lam"]).max() / max(1.0, np.abs(p["lam"]).max())
    print((S, C, K), "pcg iterations", iters, "x", ex, "lam", el)
    assert ex <= 1e-9 and el <= 1e-9
    on = p["act"] != 0
    assert np.array_equal(x[on], P.bound_values(p["act"], p["lo"], p["hi"])[on])


def test_form_schur_takes_given_inverses():
    """form_schur(inverses=...) with the Gauss-Jordan inverses it would compute itself returns the bits of the default path."""
    from gato_python_amd import synth
    from oracle import gato_oracle as o
    s = P.constructed_system(6, 3, 5, 1)
    for dt in (np.float64, np.float32):
        Gd, Cd = o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, 6, 3, 5, s.rho, dt)
        Q, R = o.unpack_G(Gd, 6, 3, 5)
        want = o.form_schur(Gd, Cd, s.g.astype(dt), s.c.astype(dt), 6, 3, 5)
        got = o.form_schur(Gd, Cd, s.g.astype(dt), s.c.astype(dt), 6, 3, 5,
                           inverses=(o.gauss_jordan_inverse(Q), o.gauss_jordan_inverse(R)))
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gato_hip.h")).read()
    for name in ("gato_box_qp_active_set", "gato_box_qp_polish", "gato_box_qp_bound_grad"):
        assert re.search(r"int\s+%s\s*\(" % name, hdr), name
    for i, code in enumerate(("ACCEPTED", "REJECTED", "NONFINITE", "BAD_ACTIVE")):
        assert re.search(r"#define\s+GATO_QP_POLISH_%s\s+%d\b" % (code, i), hdr), code
    from gato_python_amd import _lib
    L = _lib.lib()
    for name in ("gato_box_qp_active_set", "gato_box_qp_polish", "gato_box_qp_bound_grad"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert (_lib.POLISH_ACCEPTED, _lib.POLISH_REJECTED, _lib.POLISH_NONFINITE, _lib.POLISH_BAD_ACTIVE) == (0, 1, 2, 3)


def test_layer_refuses_cpu_tensors():
    import torch
    import gato_python_amd
    K, S, C = 3, 2, 1
    t = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU only"):
        gato_python_amd.box_qp_layer(t(K, S, S), t(K - 1, C, C), t(K - 1, S, S), t(K - 1, S, C), t(K, S), t(K - 1, C),
                                     t(K, S), -1.0, 1.0, -1.0, 1.0, rho=1e-3, exit_tol=1e-8, max_iters=50)
