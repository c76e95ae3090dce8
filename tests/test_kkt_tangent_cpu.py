"""The forward-mode reference (tests/kkt_tangent_ref.py) against central differences of the dense forward
solves, without a GPU: kkt_solve's tangents against kkt_grad_ref.dense_solve_and_adjoint's forward, the layer's against the reduced
solve of box_qp_polish_ref (the one the soft and capped references share) at fixed act - for every named input, one at a time and
all together - and that the problems the GPU tests use exist."""
import numpy as np
import pytest

import box_qp_polish_ref as P
import kkt_grad_ref as kgr
import kkt_tangent_ref as T
from gato_python_amd import synth

H_FD = 1e-6
BAR = 1e-6


def close(got, want, what):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(what, "max err", err.max())
    assert err.max() <= BAR, (what, err.max())


def central(forward, math, dots):
    plus = {n: v + H_FD * dots[n] if n in dots else v for n, v in math.items()}
    minus = {n: v - H_FD * dots[n] if n in dots else v for n, v in math.items()}
    (xp, lp), (xm, lm) = forward(plus), forward(minus)
    return (xp - xm) / (2 * H_FD), (lp - lm) / (2 * H_FD)


KKT_CASES = [(2, 1, 5), (6, 3, 3), (14, 7, 9)]


def kkt_blocks(S, C, K):
    """Seeded synthetic blocks at the three shapes of the GPU tests.  (The pendulum literals themselves are no case here: with
    |lam| = 240 and cond(M) = 4e4 the rounding noise of a central difference at h = 1e-6, about eps |lam| cond / h, is 8e-6 - the
    difference, not the formula, misses the bar; at h = 1e-4 the two agree to 5e-9.)"""
    return dict(zip(T.BLOCKS, synth.make_blocks(S, C, K, seed=7, dense_q=True))), 1e-3


@pytest.mark.parametrize("shape", KKT_CASES, ids=lambda s: "%d/%d/%d" % s)
def test_kkt_solve_tangents_against_central_differences(shape):
    math, rho = kkt_blocks(*shape)

    def forward(m):
        s = synth.blocks_to_csr(*(m[n] for n in T.BLOCKS), rho=rho, dense_q=True)
        dz, lam, _, _ = kgr.dense_solve_and_adjoint(s, np.zeros(s.N), np.zeros(s.S * s.K))
        return dz, lam
    for names in [(n,) for n in T.BLOCKS] + [T.BLOCKS]:
        dots = T.random_math_tangents(math, 3, names)
        x, lam, x_dot, lam_dot = T.reference_tangents(math, rho, **dots)
        x0, lam0 = forward(math)
        assert np.abs(x - x0).max() < 1e-9 and np.abs(lam - lam0).max() < 1e-8
        fx, fl = central(forward, math, dots)
        close(x_dot, fx, "dz. " + "+".join(names))
        close(lam_dot, fl, "lam. " + "+".join(names))


@pytest.mark.parametrize("case", T.FD_CASES)
def test_layer_tangents_against_central_differences_at_fixed_act(case):
    p = T.layer_problem(case)
    assert p is not None, "the seed walk of %s found no problem" % case
    math, act, rho = T.math_of(p), T.act_of(p), p["s"].rho
    hard, soft, sat = T.sets(act, p.get("w"))
    print(case, "hard", int(hard.sum()), "soft", int(soft.sum()), "sat", int(sat.sum()))
    assert hard.any() and (soft.any() or "w" not in p) and (sat.any() or "m" not in p)
    forward = lambda m: T.forward_at_fixed_act(m, rho, act)
    for names in [(n,) for n in math] + [tuple(math)]:
        dots = T.random_math_tangents(math, 5, names)
        _, _, x_dot, lam_dot = T.reference_tangents(math, rho, act, **dots)
        fx, fl = central(forward, math, dots)
        close(x_dot, fx, "x. " + "+".join(names))
        close(lam_dot, fl, "lam. " + "+".join(names))


def test_the_reference_point_is_the_problems():
    """Every problem the GPU tests use exists (its seed walk finds it), reference_tangents' point is the problem's own reduced
    solution, and zero tangents give zero."""
    for case in T.LAYER_CASES:
        p = T.layer_problem(case)
        assert p is not None, case
        x, lam, x_dot, lam_dot = T.reference_tangents(T.math_of(p), p["s"].rho, T.act_of(p))
        want = p["run"] if "run" in p else p
        assert np.abs(x - want["x"]).max() < 1e-9 and np.abs(lam - want["lam"]).max() < 1e-8
        assert not x_dot.any() and not lam_dot.any()


def test_bound_tangent_on_the_hard_active_set_moves_the_point_with_the_bound():
    p = T.layer_problem("constructed 6/3/9")
    math, act = T.math_of(p), T.act_of(p)
    dots = T.random_math_tangents(math, 1, ("x_lo", "x_hi", "u_lo", "u_hi"))
    d = T.dots_from_math(p["s"].S, p["s"].C, p["s"].K, **dots)
    _, _, x_dot, _ = T.reference_tangents(math, p["s"].rho, act, **dots)
    on = act != 0
    assert np.array_equal(x_dot[on], T.b_dot_of(act, d["lo_dot"], d["hi_dot"])[on])


def test_device_layout_helpers_invert_the_packing():
    from oracle import gato_oracle as o
    S, C, K = 4, 2, 3
    Q, R, A, B, q, r, c = synth.make_blocks(S, C, K, seed=1, dense_q=True)
    H, Cm, _, _ = P.dense_from_blocks(Q, R, A, B, q, r, c, 0.0)
    assert np.array_equal(T.dense_G(o.pack_G(Q, R), S, C, K), H)
    assert np.array_equal(T.dense_C(kgr.pack_C(A, B), S, C, K, True), Cm)
    noid = T.dense_C(kgr.pack_C(A, B), S, C, K, False)
    assert np.array_equal(noid + T.dense_C(0 * kgr.pack_C(A, B), S, C, K, True), Cm) and not noid[:S].any()
