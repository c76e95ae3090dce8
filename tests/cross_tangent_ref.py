"""numpy reference of the forward-mode sensitivities of a KKT solve with a cross term, for the tests.

With (x, lam) the point of the solve in the original variables, a dot an input tangent (a missing one is zero), G_k = [[Q_k, M_k],
[M_k^T, R_k]] for k < K-1 and A, B the raw values of C:
    t_g,x,k = q._k - Q._k x_k - M._k u_k - A._k^T lam_k+1        t_g,u,k = r._k - R._k u_k - M._k^T x_k - B._k^T lam_k+1
    t_c,k+1 = c._k+1 - A._k x_k - B._k u_k,  t_c,0 = c._0        (the last knot has no M, no R and no C block of its own)
    [x.; lam.] = KKT^-1 [t_g; t_c]                               (the cross KKT matrix: cross_ref.dense_kkt)
M. is used as given: M_k and M_k^T are perturbed together.  tangent_rhs() is the formulas per row in a dtype, with scale_i = the
sum of the absolute values of the row's terms; transform_rhs() the change of variables of the right-hand side from a given W with
scale'_i = scale_i + sum_c |W_ci| scale_S+c on state rows; dense_tangent() the direct dense solve; three_step_tangent() the route
of the device (transform, block-diagonal solve, finish) in float64; restatement32() the same route in float32 around the
oracle's float32 solve.  Tangents are math-shaped dicts by input name (NAMES); vectors in the solver's layouts."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cross_ref as X                             # noqa: E402
from gato_python_amd import synth                 # noqa: E402

NAMES = ("Q", "R", "A", "B", "q", "r", "c", "M")

# ---- the cells of tests/test_gpu_cross_tangent.py; tests/test_cross_tangent_cpu.py asserts their conditioning ----------------------
KERNEL_K = (2, 3, 9)                              # the kernel alone: all X.SHAPES x these x two precisions, B = 1 / R = 1 and B = 3 / R = 3
SOLVE_CELLS = [(2, 1, 5), (4, 2, 3), (14, 7, 9), (32, 16, 3)]
PAIR_CELLS = [(4, 2, 3), (14, 7, 9)]              # the pairing with the backward pass, and fp32


def kernel_cells(S, C, K, B):
    return X.batch_cells(S, C, K, B, seed=50 + K)


def solve_cells(S, C, K, B):
    return X.batch_cells(S, C, K, B, seed=60 + K)


def shapes_of(S, C, K):
    return dict(Q=(K, S, S), R=(K - 1, C, C), A=(K - 1, S, S), B=(K - 1, S, C), q=(K, S), r=(K - 1, C), c=(K, S), M=(K - 1, S, C))


def random_dots(S, C, K, seed, names=NAMES, symmetric=True):
    """A standard-normal tangent per named input; Q and R symmetric unless told otherwise (the kernel takes them as given)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in shapes_of(S, C, K).items():
        d = rng.standard_normal(shape)                                    # drawn for every name: a subset keeps the others' values
        if symmetric and name in ("Q", "R"):
            d = 0.5 * (d + np.swapaxes(d, -1, -2))
        if name in names:
            out[name] = d
    return out


def pack_dots(dots, S, C, K, dtype=np.float64):
    """Math-shaped tangents -> the device layouts by the kernel's names (G_dot, M_dot, C_dot, g_dot, c_dot); a pair (Q, R), (A, B)
    or (q, r) neither of which is given, c and M likewise, is left out (a NULL pointer)."""
    full = {n: np.asarray(dots.get(n, np.zeros(s)), np.float64) for n, s in shapes_of(S, C, K).items()}
    Gd, Cd, g, c, Mb = X.pack(*(full[n] for n in NAMES[:7]), full["M"])
    have = lambda *names: any(n in dots for n in names)
    out = {}
    for key, arr, names in (("G_dot", Gd, ("Q", "R")), ("M_dot", Mb, ("M",)), ("C_dot", Cd, ("A", "B")), ("g_dot", g, ("q", "r")),
                            ("c_dot", c, ("c",))):
        if have(*names):
            out[key] = arr.astype(dtype)
    return out


def tangent_rhs(x, lam, S, C, K, dots, dtype=np.float64):
    """-> (t_g [N], t_c [S K], scale_g, scale_c): the formulas per knot with every product and sum in `dtype`; the scales in
    float64."""
    n, N = S + C, (S + C) * K - C
    d = {name: np.asarray(dots.get(name, np.zeros(s)), np.float64).astype(dtype) for name, s in shapes_of(S, C, K).items()}
    x, lam = np.asarray(x).astype(dtype), np.asarray(lam).astype(dtype).reshape(K, S)
    a = lambda v: np.abs(np.asarray(v, np.float64))
    t_g, s_g = np.zeros(N, dtype), np.zeros(N)
    t_c, s_c = d["c"].copy(), a(d["c"])
    for k in range(K):
        xs = slice(k * n, k * n + S)
        xk = x[xs]
        tx, sx = d["q"][k] - d["Q"][k] @ xk, a(d["q"][k]) + a(d["Q"][k]) @ a(xk)
        if k < K - 1:
            us = slice(k * n + S, (k + 1) * n)
            uk, ln = x[us], lam[k + 1]
            tx = tx - d["M"][k] @ uk - d["A"][k].T @ ln
            sx = sx + a(d["M"][k]) @ a(uk) + a(d["A"][k]).T @ a(ln)
            t_g[us] = d["r"][k] - d["R"][k] @ uk - d["M"][k].T @ xk - d["B"][k].T @ ln
            s_g[us] = a(d["r"][k]) + a(d["R"][k]) @ a(uk) + a(d["M"][k]).T @ a(xk) + a(d["B"][k]).T @ a(ln)
            t_c[k + 1] = t_c[k + 1] - d["A"][k] @ xk - d["B"][k] @ uk
            s_c[k + 1] = s_c[k + 1] + a(d["A"][k]) @ a(xk) + a(d["B"][k]) @ a(uk)
        t_g[xs], s_g[xs] = tx, sx
    return t_g, t_c.reshape(-1), s_g, s_c.reshape(-1)


def transform_rhs(W, t_g, s_g, S, C, K):
    """(g', scale') from W [K-1, C, S] in the dtype of W: g'_x = t_g,x - W^T t_g,u with scale'_x = scale_x + |W|^T scale_u."""
    n = S + C
    gp, sp = X.transform_g(W, t_g, S, C, K), np.asarray(s_g, np.float64).copy()
    for k in range(K - 1):
        sp[k * n:k * n + S] += np.abs(np.asarray(W[k], np.float64)).T @ sp[k * n + S:(k + 1) * n]
    return gp, sp


def dense_tangent(blocks, M, dots, rho=X.RHO):
    """(x, lam, x_dot, lam_dot) by two direct dense solves of the cross KKT, refined (cross_ref.dense_solve)."""
    Q, R = blocks[0], blocks[1]
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    x, lam = X.dense_solve(blocks, M, rho=rho)
    t_g, t_c, _, _ = tangent_rhs(x, lam, S, C, K, dots)
    x_dot, lam_dot = X.dense_solve(blocks, M, g=t_g, c=t_c, rho=rho)
    return x, lam, x_dot, lam_dot


def three_step_tangent(blocks, M, dots, rho=X.RHO):
    """(x_dot, lam_dot) by the device's route in float64: g' = t_g,x - W^T t_g,u, the block-diagonal solve of the transformed
    system, u. = v. - W x.  (cross_ref.transformed_solve with the right-hand side (t_g, t_c).)"""
    Q, R = blocks[0], blocks[1]
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    x, lam = X.dense_solve(blocks, M, rho=rho)
    t_g, t_c, _, _ = tangent_rhs(x, lam, S, C, K, dots)
    return X.transformed_solve(blocks, M, rho, np.float64, g=t_g, c=t_c)


def central_difference(blocks, M, dots, h=1e-6, rho=X.RHO):
    """(x_dot, lam_dot) by central differences of cross_ref.dense_solve along the direction dots."""
    ops = dict(zip(NAMES, list(blocks) + [M]))

    def at(sign):
        p = {n: v + sign * h * np.asarray(dots[n]) if n in dots else v for n, v in ops.items()}
        return X.dense_solve(tuple(p[n] for n in NAMES[:7]), p["M"], rho=rho)
    (xp, lp), (xm, lm) = at(1.0), at(-1.0)
    return (xp - xm) / (2 * h), (lp - lm) / (2 * h)


def restatement32(blocks, M, dots, tol, max_iters, rho=X.RHO):
    """(x_dot, lam_dot) of the float32 restatement: its point (cross_ref.oracle32_solve), the right-hand side in float32 from
    that point, g' from the float32 W, the transformed system with that right-hand side through the oracle's float32 solve (the
    device's exit_tol and max_iters), the finish in float32."""
    from oracle import gato_oracle as o
    Q, R, A, B, q, r, cc = blocks
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    x32, lam32 = X.oracle32_solve(blocks, M, tol, max_iters, rho)
    t_g, t_c, _, _ = tangent_rhs(x32, lam32, S, C, K, dots, np.float32)
    t = X.transform(Q, R, A, B, q, r, M, rho, np.float32)
    gp = X.transform_g(t["W"], t_g, S, C, K)
    s = synth.blocks_to_csr(*(np.asarray(v, np.float64) for v in (t["Q2"], R, t["A2"], B, t["q2"], r, cc)), rho=rho)
    lam_d, xp_d, _ = o.linsys_solve(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, gp.astype(np.float32), t_c.astype(np.float32),
                                    S, C, K, tol, max_iters, rho, dtype=np.float32)
    return X.finish(t["W"], np.asarray(xp_d, np.float32), S, C, K), np.asarray(lam_d)
