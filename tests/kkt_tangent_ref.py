"""numpy fp64 reference of the forward-mode sensitivities, for the tests.

With (x, lam) the point of a KKT solve or of a converged box QP on its act, a dot an input tangent, A the hard-active set (act
!= 0 and w_i = 0 or no weights), "soft" act = +-1 with w_i > 0 and "sat" act = +-2, b_i = hi_i (act_i > 0) or lo_i (act_i < 0):
    1. t_g = g. - G. x - C.^T lam,  t_c = c. - C. x                  (C's identity blocks carry no tangent; rho drops out)
    2. soft i: t_g,i += w._i (b_i - x_i) + w_i b._i;  sat i: t_g,i -= sign(act_i) m._i
    3. t_g -= G b._A,  t_c -= C b._A                                 (b._A = b. on A, 0 elsewhere; C's identity blocks included)
and [x.'; lam.] solves the reduced system of the act for (t_g, t_c); x. = x.' off A and b. on A.
tangent_rhs() is the three steps per row with scale_i = the sum of the absolute values of the row's terms; tangent_solve() the
dense reduced solve.  Everything is in the dz layout with dense matrices; the helpers convert from the device layouts and from
math-shaped tangents."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_polish_ref as P                     # noqa: E402
from oracle import gato_oracle as o               # noqa: E402

BLOCKS = ("Q", "R", "A", "B", "q", "r", "c")
BOUNDS = ("x_lo", "x_hi", "u_lo", "u_hi")
LAYER_NAMES = BLOCKS + BOUNDS + ("x_soft", "u_soft", "x_soft_max", "u_soft_max")
DOTS = ("G_dot", "C_dot", "g_dot", "c_dot", "lo_dot", "hi_dot", "w_dot", "m_dot")


def dense_G(Gd, S, C, K, sparse=False):
    """G_dense layout -> the block-diagonal N x N matrix (sparse: scipy CSR, for horizons whose dense matrix is out of reach)."""
    from scipy import sparse as sp
    n, N = S + C, (S + C) * K - C
    Q, R = o.unpack_G(np.asarray(Gd, np.float64), S, C, K)

    def coo(blocks, first, size):
        k = (np.arange(blocks.shape[0]) * n + first)[:, None, None]
        rows = k + np.arange(size)[None, :, None] + 0 * np.arange(size)[None, None, :]
        cols = k + 0 * np.arange(size)[None, :, None] + np.arange(size)[None, None, :]
        return sp.csr_matrix((blocks.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(N, N))
    M = coo(Q, 0, S) + coo(R, S, C)
    return M if sparse else M.toarray()


def dense_C(Cd, S, C, K, identity, sparse=False):
    """C_dense layout -> the S K x N matrix, with or without C's identity blocks."""
    from scipy import sparse as sp
    n, N = S + C, (S + C) * K - C
    A, B = o.unpack_C(np.asarray(Cd, np.float64), S, C, K)
    AB = np.concatenate([A, B], axis=2)                                   # [K-1, S, n]
    rows = ((np.arange(K - 1) + 1) * S)[:, None, None] + np.arange(S)[None, :, None] + 0 * np.arange(n)[None, None, :]
    cols = (np.arange(K - 1) * n)[:, None, None] + 0 * np.arange(S)[None, :, None] + np.arange(n)[None, None, :]
    M = sp.csr_matrix((AB.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(S * K, N))
    if identity:
        ir = np.arange(S * K)
        M = M + sp.csr_matrix((np.ones(S * K), (ir, (ir // S) * n + ir % S)), shape=(S * K, N))
    return M if sparse else M.toarray()


def sets(act, w):
    """(hard, soft, sat) of an act and weights (None: all hard)."""
    act = np.asarray(act)
    sa = P.soft_set(act, w)
    sat = P.sat_set(act) & sa
    return P.hard_set(act, w), sa & ~sat, sat


def b_dot_of(act, lo_dot, hi_dot):
    return np.where(np.asarray(act) > 0, hi_dot, np.where(np.asarray(act) < 0, lo_dot, 0.0))


def tangent_rhs(G, Cm, x, lam, act=None, w=None, lo=None, hi=None, G_dot=None, C_dot=None, g_dot=None, c_dot=None, lo_dot=None,
                hi_dot=None, w_dot=None, m_dot=None):
    """-> (t_g, t_c, scale_g, scale_c).  G [N, N] without rho, Cm [S K, N] with its identity blocks; G_dot [N, N], C_dot [S K, N]
    (zero on the identity blocks), dense or scipy.sparse; the vectors in the dz layout; None: zero.  act None: nothing active."""
    x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
    N, SK = len(x), len(lam)
    zero = lambda v, n: np.zeros(n) if v is None else np.asarray(v, np.float64)
    if G_dot is None:
        G_dot = 0.0 * G
    if C_dot is None:
        C_dot = 0.0 * Cm
    g_dot, c_dot, lo_dot, hi_dot, w_dot, m_dot = zero(g_dot, N), zero(c_dot, SK), zero(lo_dot, N), zero(hi_dot, N), zero(w_dot, N), zero(m_dot, N)
    t_g = g_dot - G_dot @ x - C_dot.T @ lam
    s_g = np.abs(g_dot) + abs(G_dot) @ np.abs(x) + abs(C_dot).T @ np.abs(lam)
    t_c = c_dot - C_dot @ x
    s_c = np.abs(c_dot) + abs(C_dot) @ np.abs(x)
    if act is not None:
        act = np.asarray(act, np.int8)
        hard, soft, sat = sets(act, w)
        b_dot = b_dot_of(act, lo_dot, hi_dot)
        if soft.any():
            b = P.bound_values(act, lo, hi)
            add = w_dot * (b - x) + w * b_dot
            t_g = t_g + np.where(soft, add, 0.0)
            s_g = s_g + np.where(soft, np.abs(w_dot * (b - x)) + np.abs(w * b_dot), 0.0)
        t_g = t_g - np.where(sat, np.sign(act) * m_dot, 0.0)
        s_g = s_g + np.where(sat, np.abs(m_dot), 0.0)
        bA = np.where(hard, b_dot, 0.0)
        t_g, s_g = t_g - G @ bA, s_g + abs(G) @ np.abs(bA)
        t_c, s_c = t_c - Cm @ bA, s_c + abs(Cm) @ np.abs(bA)
    return t_g, t_c, s_g, s_c


def tangent_solve(H, Cm, t_g, t_c, act=None, w=None, lo_dot=None, hi_dot=None):
    """(x_dot, lam_dot): the dense reduced solve of the act (H with rho) for (t_g, t_c); x_dot = b_dot on the hard-active set."""
    N = len(t_g)
    act = np.zeros(N, np.int8) if act is None else np.asarray(act, np.int8)
    solve, F = P._reduced_solver(H, Cm, act, w)
    sol = solve(np.concatenate([np.asarray(t_g, np.float64)[F], np.asarray(t_c, np.float64)]))
    zero = lambda v: np.zeros(N) if v is None else np.asarray(v, np.float64)
    x_dot = np.where(P.hard_set(act, w), b_dot_of(act, zero(lo_dot), zero(hi_dot)), 0.0)
    x_dot[F] = sol[:len(F)]
    return x_dot, sol[len(F):]


def dots_from_math(S, C, K, **t):
    """Math-shaped tangents by input name (LAYER_NAMES; missing: zero) -> tangent_rhs's keyword arguments."""
    z = lambda *shape: np.zeros(shape)
    get = lambda name, *shape: np.asarray(t[name], np.float64) if name in t else z(*shape)
    Hd, Cd, gd, cd = P.dense_from_blocks(get("Q", K, S, S), get("R", K - 1, C, C), get("A", K - 1, S, S), get("B", K - 1, S, C),
                                         get("q", K, S), get("r", K - 1, C), get("c", K, S), 0.0)
    Cd = Cd - P.dense_from_blocks(z(K, S, S), z(K - 1, C, C), z(K - 1, S, S), z(K - 1, S, C), z(K, S), z(K - 1, C), z(K, S), 0.0)[1]
    lay = lambda xn, un: P.ref.dz_layout(get(xn, K, S), get(un, K - 1, C), S, C, K)
    return dict(G_dot=Hd, C_dot=Cd, g_dot=gd, c_dot=cd, lo_dot=lay("x_lo", "u_lo"), hi_dot=lay("x_hi", "u_hi"),
                w_dot=lay("x_soft", "u_soft"), m_dot=lay("x_soft_max", "u_soft_max"))


def reference_tangents(math, rho, act=None, **t):
    """(x, lam, x_dot, lam_dot) of the problem with the math-shaped inputs `math` (a dict by LAYER_NAMES: the seven blocks, and
    with an act the four bounds and, where soft, the weights and caps) at fixed act, along the math-shaped tangents t."""
    Q = math["Q"]
    K, S, C = Q.shape[0], Q.shape[1], math["R"].shape[-1]
    H, Cm, g, c = P.dense_from_blocks(*(math[n] for n in BLOCKS), rho)
    N = len(g)
    lo = hi = w = m = None
    if act is not None:
        lay = lambda xn, un: P.ref.dz_layout(math[xn], math[un], S, C, K)
        lo, hi = lay("x_lo", "u_lo"), lay("x_hi", "u_hi")
        w = lay("x_soft", "u_soft") if "x_soft" in math else None
        m = lay("x_soft_max", "u_soft_max") if "x_soft_max" in math else None
        x, _, lam = P.reduced_solve(H, Cm, g, c, lo, hi, act, w, m)
    else:
        x, _, lam = P.reduced_solve(H, Cm, g, c, np.full(N, -np.inf), np.full(N, np.inf), np.zeros(N, np.int8))
    d = dots_from_math(S, C, K, **t)
    t_g, t_c, _, _ = tangent_rhs(H - rho * np.eye(N), Cm, x, lam, act, w, lo, hi, **d)
    x_dot, lam_dot = tangent_solve(H, Cm, t_g, t_c, act, w, d["lo_dot"], d["hi_dot"])
    return x, lam, x_dot, lam_dot


def forward_at_fixed_act(math, rho, act=None):
    """(x, lam) of reference_tangents alone: what central differences perturb."""
    return reference_tangents(math, rho, act)[:2]


def random_math_tangents(math, seed, names=None):
    """A random tangent per named input (all of `math` by default), Q and R symmetric, zero where a bound, weight or cap is not
    finite or a weight is 0 (the tangent of a hard bound's weight would make it soft)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in (names or list(math)):
        v = np.asarray(math[name], np.float64)
        d = rng.standard_normal(v.shape)
        if name in ("Q", "R"):
            d = 0.5 * (d + np.swapaxes(d, -1, -2))
        if name not in BLOCKS:
            d = np.where(np.isfinite(v), d, 0.0)
        if name in ("x_soft", "u_soft"):
            d = np.where(v > 0, d, 0.0)
        out[name] = d
    return out


# ---- the problems of the tests: the walked and constructed ones of the box-QP suites -----------------------------------------------
LAYER_CASES = ("constructed 6/3/9", "mixed 6/3/9", "mixed 14/7/3", "huber 6/3/9")
# the cases central differences at h = 1e-6 can judge at 1e-6: the difference quotient's own rounding noise grows as eps cond(M)
# |lam| / h, and at mixed 14/7/3 (cond 3.9e6, |lam| = 120) it is 8e-6 for the direction Q alone - falling as 1 / h to 4e-8 at h =
# 1e-4, where the all-inputs direction's truncation error is 3e-2.  That case is held to the device pairing test instead.
FD_CASES = ("constructed 6/3/9", "mixed 6/3/9", "huber 6/3/9")


def layer_problem(case):
    """One of LAYER_CASES as a problem dict (s, H, Cm, g, c, lo, hi, "w" / "m" where soft / capped), or None if its seed walk
    finds nothing: hard bounds with active states (box_qp_pdas_ref.constructed_cold), hard and soft bounds in one act
    (box_qp_soft_ref.mixed_box), capped bounds with a saturated variable (box_qp_huber_ref.huber_box / mixed_box)."""
    import box_qp_huber_ref as HR
    import box_qp_soft_ref as SR
    kind, shape = case.rsplit(" ", 1)
    S, C, K = (int(v) for v in shape.split("/"))
    if kind == "constructed":
        import box_qp_pdas_ref as D
        ps = D.constructed_cold(S, C, K)
    elif kind == "mixed":
        ps = SR.mixed_box(S, C, K)
    elif kind == "huber":
        ps = HR.huber_box(S, C, K)
    else:
        ps = [HR.mixed_box(S, C, K)]
    return ps[0] if ps and ps[0] is not None else None


def act_of(p):
    return np.asarray(p["run"]["act"] if "run" in p else p["act"], np.int8)


def math_of(p):
    """The math-shaped inputs of problem p by name: the seven blocks and four bounds, x_soft / u_soft with "w", x_soft_max /
    u_soft_max with "m"."""
    import box_qp_huber_ref as HR
    import box_qp_soft_ref as SR
    if "m" in p:
        return dict(zip(HR.HUBER_KEYS, HR.huber_math_arrays(p)))
    arrs = SR.soft_math_arrays(p)
    return dict(zip(SR.SOFT_KEYS, arrs)) if "w" in p else dict(zip(SR.SOFT_KEYS[:11], arrs[:11]))
