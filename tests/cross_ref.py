"""numpy reference of KKT solves with a state-control cross term, for the tests.

The stage Hessian is G_k = [[Q_k, M_k], [M_k^T, R_k]] (k < K-1; the last knot is Q_{K-1}), H = G + rho I.  Three restatements:
  * the dense KKT matrix with the cross blocks inserted, solved in float64 and refined once with a longdouble residual;
  * the per-knot change of variables u = v - W x, W = (R + rho I)^-1 M^T, in a given dtype (longdouble: what the device's fp64
    blocks are held to; float32: what its fp32 blocks are measured beside);
  * the gradient formulas on (dz, lambda, a, beta): kkt_grad_ref.grads_math and M_bar_k = -(a_x dz_u^T + dz_x a_u^T).
Blocks are math-shaped (Q [K,S,S], R [K-1,C,C], A, B the raw values of C, M [K-1,S,C]); vectors in the solver's layouts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gato_python_amd import synth                 # noqa: E402

LD = np.longdouble
RHO = 1e-3
SHAPES = [(2, 1), (4, 2), (6, 3), (12, 6), (14, 7), (32, 16)]


# ---- the cells of the GPU tests (tests/test_gpu_cross.py); test_cross_cpu.py asserts their conditioning --------------------------
def cell(S, C, K, seed=0, dense_q=False, scale=0.5):
    """Blocks (Q, R, A, B, q, r, c) of synth.make_blocks and M of synth.make_cross for one system."""
    blocks = synth.make_blocks(S, C, K, seed=seed, dense_q=dense_q)
    return blocks, synth.make_cross(blocks[0], blocks[1], seed=seed + 1000, scale=scale)


def batch_cells(S, C, K, B, seed=0):
    """B different systems of one shape: system 1 has dense Q blocks, the others diagonal ones.  R_k is diagonal in every system
    (synth.make_blocks), A_k = -(I + 1 % noise), c_0 = 0 and every knot has the same O(1) scale; tests/cross_hard_cells.py has
    the cells without these."""
    return [cell(S, C, K, seed=seed + 17 * b, dense_q=(b == 1)) for b in range(B)]


KERNEL_K = (1, 2, 3, 5)                           # kernels alone: all SHAPES x these, B = 3
STRIDE_CELL = (2, 1, 8197)                        # the second pass of the knot stride (grid.x = 8192)
SOLVE_CELLS = [(S, C, K) for S, C in SHAPES for K in (2, 3, 9)] + [(14, 7, 50)]
RESOLVE_CELLS = [(4, 2, 3), (14, 7, 9), (32, 16, 3)]
GRADCHECK_CELLS = [(2, 1, 3), (4, 2, 3)]
GRAD_K = (2, 3)                                   # grad_cross_kernel: all SHAPES x these


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def pack(Q, R, A, B, q, r, c, M=None):
    """-> (G_dense, C_dense, g, c[, M_blocks]) flat, per knot column-major, in the dtype of Q."""
    K = Q.shape[0]
    Gd = np.concatenate([np.concatenate([Q[k].T.reshape(-1), R[k].T.reshape(-1)]) for k in range(K - 1)] + [Q[K - 1].T.reshape(-1)])
    Cd = np.concatenate([np.concatenate([A[k].T.reshape(-1), B[k].T.reshape(-1)]) for k in range(K - 1)]) if K > 1 else np.zeros(0, Q.dtype)
    g = np.concatenate([np.concatenate([q[k], r[k]]) for k in range(K - 1)] + [q[K - 1]])
    out = (Gd, Cd, g, np.asarray(c).reshape(-1).copy())
    return out if M is None else out + (pack_M(M),)


def pack_M(M):
    """M [K-1,S,C] -> M_blocks: per knot S x C column-major (W [K-1,C,S] -> the W layout likewise)."""
    return np.concatenate([M[k].T.reshape(-1) for k in range(M.shape[0])]) if M.shape[0] else np.zeros(0, M.dtype)


def unpack_M(flat, S, C, K):
    return np.stack([flat[k * S * C:(k + 1) * S * C].reshape(C, S).T for k in range(K - 1)]) if K > 1 else np.zeros((0, S, C), flat.dtype)


def unpack_W(flat, S, C, K):
    return np.stack([flat[k * S * C:(k + 1) * S * C].reshape(S, C).T for k in range(K - 1)]) if K > 1 else np.zeros((0, C, S), flat.dtype)


# ---- the dense KKT with the cross blocks ------------------------------------------------------------------------------------
def dense_kkt(Q, R, A, B, M=None, rho=RHO, dtype=np.float64):
    """[[G + rho I, C^T], [C, 0]] with M_k, M_k^T between the Q_k and R_k blocks (M None: none); C's identity blocks included."""
    K, S = Q.shape[0], Q.shape[1]
    C = R.shape[-1] if K > 1 else 0
    n, N, SK = S + C, (S + C) * K - C, S * K
    G = np.zeros((N, N), dtype)
    Cm = np.zeros((SK, N), dtype)
    Cm[:S, :S] = np.eye(S)
    for k in range(K):
        x = slice(k * n, k * n + S)
        G[x, x] = Q[k]
        if k < K - 1:
            u = slice(k * n + S, (k + 1) * n)
            G[u, u] = R[k]
            if M is not None:
                G[x, u] = M[k]
                G[u, x] = M[k].T
            rows = slice((k + 1) * S, (k + 2) * S)
            Cm[rows, x] = A[k]
            Cm[rows, u] = B[k]
            Cm[rows, (k + 1) * n:(k + 1) * n + S] = np.eye(S)
    G = G + rho * np.eye(N, dtype=dtype)
    return np.block([[G, Cm.T], [Cm, np.zeros((SK, SK), dtype)]])


def solve_refined(Mat, rhs):
    """Mat^-1 rhs (rhs [n] or [n, R]): the float64 LU solve and one refinement with the residual in longdouble."""
    Mat64, rhs = np.asarray(Mat, np.float64), np.asarray(rhs, np.float64)
    x = np.linalg.solve(Mat64, rhs)
    res = (rhs.astype(LD) - Mat64.astype(LD) @ x.astype(LD)).astype(np.float64)
    return x + np.linalg.solve(Mat64, res)


def dense_solve(blocks, M, g=None, c=None, rho=RHO):
    """(dz, lam) of the dense cross KKT; g [N] or [R, N] and c likewise replace the blocks' own right-hand side."""
    Q, R, A, B, q, r, cc = blocks
    Mat = dense_kkt(Q, R, A, B, M, rho)
    if g is None:
        _, _, g, c = pack(Q, R, A, B, q, r, cc)
    rhs = np.concatenate([np.asarray(g, np.float64), np.asarray(c, np.float64)], axis=-1)
    x = solve_refined(Mat, rhs.T).T
    N = Mat.shape[0] - Q.shape[0] * Q.shape[1]
    return x[..., :N], x[..., N:]


# ---- the change of variables, per block, in a dtype ----------------------------------------------------------------------------
def gj_inverse(Aa):
    """Gauss-Jordan without pivoting in the dtype of Aa (numpy has no longdouble LAPACK): pivot row *= 1 / pivot, the other rows
    -= their multiplier x that row - the elimination the device's inverse does."""
    n = Aa.shape[0]
    W = np.concatenate([Aa.copy(), np.eye(n, dtype=Aa.dtype)], 1)
    for p in range(n):
        W[p] = W[p] * (Aa.dtype.type(1) / W[p, p])
        for r in range(n):
            if r != p:
                W[r] = W[r] - W[r, p] * W[p]
    return W[:, n:]


def transform(Q, R, A, B, q, r, M, rho=RHO, dtype=LD):
    """-> dict W [K-1,C,S], Q2 [K,S,S] (Q'', rho not added), A2 [K-1,S,S], q2 [K,S]; R, B, r are unchanged."""
    Q, R, A, B, q, r, M = (np.asarray(t).astype(dtype) for t in (Q, R, A, B, q, r, M))
    K = Q.shape[0]
    Q2, q2 = Q.copy(), q.copy()
    W = np.zeros((K - 1,) + M.shape[1:][::-1], dtype)
    A2 = A.copy()
    for k in range(K - 1):
        Rr = R[k] + dtype(rho) * np.eye(R.shape[-1], dtype=dtype)
        W[k] = gj_inverse(Rr) @ M[k].T
        Q2[k] = Q[k] - M[k] @ W[k]
        A2[k] = A[k] - B[k] @ W[k]
        q2[k] = q[k] - W[k].T @ r[k]
    return dict(W=W, Q2=Q2, A2=A2, q2=q2)


def transform_g(W, g, S, C, K):
    """g [N] -> g' from W [K-1,C,S], in the dtype of W."""
    n = S + C
    out = np.asarray(g).astype(W.dtype).copy()
    for k in range(K - 1):
        out[k * n:k * n + S] -= W[k].T @ out[k * n + S:(k + 1) * n]
    return out


def finish(W, dzp, S, C, K):
    """dz' [N] in (x, v) -> dz in (x, u): u_k = v_k - W_k x_k, in the dtype of W."""
    n = S + C
    out = np.asarray(dzp).astype(W.dtype).copy()
    for k in range(K - 1):
        out[k * n + S:(k + 1) * n] -= W[k] @ out[k * n:k * n + S]
    return out


def transformed_solve(blocks, M, rho=RHO, dtype=np.float64, g=None, c=None):
    """(dz, lam) by the three steps in `dtype`: transform, the dense block-diagonal solve (numpy, float64 or float32), finish."""
    Q, R, A, B, q, r, cc = blocks
    K, S = Q.shape[0], Q.shape[1]
    C = R.shape[-1]
    t = transform(Q, R, A, B, q, r, M, rho, dtype)
    Mat = dense_kkt(t["Q2"], R.astype(dtype), t["A2"], B.astype(dtype), None, rho, dtype)
    if g is None:
        gp = pack(t["Q2"], R.astype(dtype), t["A2"], B.astype(dtype), t["q2"], r.astype(dtype), cc.astype(dtype))[2]
        c = np.asarray(cc).reshape(-1)
    else:
        gp = transform_g(t["W"], g, S, C, K)
    rhs = np.concatenate([gp, np.asarray(c).astype(dtype)])
    x = np.linalg.solve(Mat, rhs) if dtype is not LD else solve_refined(Mat, rhs).astype(LD)
    N = Mat.shape[0] - S * K
    return finish(t["W"], x[:N], S, C, K), x[N:]


def oracle32_solve(blocks, M, tol, max_iters, rho=RHO, iters=False):
    """The float32 restatement of a whole cross solve: the transform per block in float32, the oracle's float32 solve (the
    reference's algorithm in its own order of the sums, same exit_tol and max_iters as the device) of the transformed system,
    the finish in float32.  -> (dz, lam), with iters also the oracle's iteration count."""
    from oracle import gato_oracle as o
    Q, R, A, B, q, r, cc = blocks
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    t = transform(Q, R, A, B, q, r, M, rho, np.float32)
    s = synth.blocks_to_csr(*(np.asarray(x, np.float64) for x in (t["Q2"], R, t["A2"], B, t["q2"], r, cc)), rho=rho)
    lam, dzp, it = o.linsys_solve(*s.csr_args(), S, C, K, tol, max_iters, rho, dtype=np.float32)
    out = finish(t["W"], np.asarray(dzp, np.float32), S, C, K), np.asarray(lam)
    return out + (int(it),) if iters else out


# ---- gradients ------------------------------------------------------------------------------------------------------------
def grad_M(dz, a, S, C, K):
    """M_bar [K-1,S,C] = -(a_x dz_u^T + dz_x a_u^T): M_k and M_k^T perturbed together."""
    n = S + C
    dz, a = np.asarray(dz, np.float64), np.asarray(a, np.float64)
    x = lambda v, k: v[k * n:k * n + S]
    u = lambda v, k: v[k * n + S:(k + 1) * n]
    return np.stack([-(np.outer(x(a, k), u(dz, k)) + np.outer(x(dz, k), u(a, k))) for k in range(K - 1)]) if K > 1 else np.zeros((0, S, C))


def dense_reference(blocks, M, dz_bar, lam_bar, rho=RHO):
    """Every gradient of L (dL/ddz = dz_bar, dL/dlam = lam_bar) from the dense forward and adjoint solves: kkt_grad_ref's
    formulas for Q, R, A, B, q, r, c and grad_M for M; also dz, lam, a, beta."""
    import kkt_grad_ref
    Q, R = blocks[0], blocks[1]
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    dz, lam = dense_solve(blocks, M, rho=rho)
    a, beta = dense_solve(blocks, M, g=dz_bar, c=lam_bar, rho=rho)
    out = kkt_grad_ref.grads_math(dz, lam, a, beta, S, C, K)
    out.update(M=grad_M(dz, a, S, C, K), dz=dz, lam=lam, a=a, beta=beta)
    return out
