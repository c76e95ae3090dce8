"""numpy reference of the KKT-solve gradients, for the tests.

The solve is M x = b, M = [[G + rho I, C^T], [C, 0]], x = [dz; lambda], b = [g; c].  With upstream gradients (dz_bar, lam_bar)
the adjoint is [a; beta] = M^-1 [dz_bar; lam_bar] (M is symmetric) and
    g_bar = a,  c_bar = beta,
    Q_bar_k = -1/2 (a_x,k dz_x,k^T + dz_x,k a_x,k^T),  R_bar_k the same on the u-parts      (symmetric perturbations)
    A_bar_k = -(beta_k+1 dz_x,k^T + lambda_k+1 a_x,k^T),  B_bar_k = -(beta_k+1 dz_u,k^T + lambda_k+1 a_u,k^T)
with A_k, B_k the raw values stored in C (-A, -B of the dynamics).  The identity blocks of C get no gradient: the solver
never reads them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gato_python_amd import synth                 # noqa: E402
from oracle import gato_oracle as o               # noqa: E402


def grads_math(dz, lam, a, beta, S, C, K):
    """-> dict Q [K,S,S], R [K-1,C,C], A [K-1,S,S], B [K-1,S,C], q [K,S], r [K-1,C], c [K,S] of the gradient."""
    n = S + C
    dz, lam, a, beta = (np.asarray(v, np.float64) for v in (dz, lam, a, beta))
    x = lambda v, k: v[k * n: k * n + S]
    u = lambda v, k: v[k * n + S: (k + 1) * n]
    blk = lambda v, k: v[k * S: (k + 1) * S]
    Q = np.stack([-0.5 * (np.outer(x(a, k), x(dz, k)) + np.outer(x(dz, k), x(a, k))) for k in range(K)])
    R = np.zeros((K - 1, C, C))
    A = np.zeros((K - 1, S, S))
    B = np.zeros((K - 1, S, C))
    for k in range(K - 1):
        R[k] = -0.5 * (np.outer(u(a, k), u(dz, k)) + np.outer(u(dz, k), u(a, k)))
        A[k] = -(np.outer(blk(beta, k + 1), x(dz, k)) + np.outer(blk(lam, k + 1), x(a, k)))
        B[k] = -(np.outer(blk(beta, k + 1), u(dz, k)) + np.outer(blk(lam, k + 1), u(a, k)))
    q = np.stack([x(a, k) for k in range(K)])
    r = np.stack([u(a, k) for k in range(K - 1)]) if K > 1 else np.zeros((0, C))
    return dict(Q=Q, R=R, A=A, B=B, q=q, r=r, c=beta.reshape(K, S).copy())


def pack_C(A, B):
    """A [K-1,S,S], B [K-1,S,C] -> C_dense (per knot [A_k | B_k] column-major; inverse of oracle.unpack_C)."""
    return np.concatenate([np.concatenate([A[k].T.reshape(-1), B[k].T.reshape(-1)]) for k in range(A.shape[0])]) \
        if A.shape[0] else np.zeros(0)


def grads_dense_layout(dz, lam, a, beta, S, C, K):
    """-> (G_bar in the G_dense layout, C_bar in the C_dense layout)."""
    m = grads_math(dz, lam, a, beta, S, C, K)
    return o.pack_G(m["Q"], m["R"]), pack_C(m["A"], m["B"])


def csr_slot_map(G_row, G_col, C_row, C_col, S, C, K):
    """Restates oracle.convert's loops: CSR entry -> index into G_dense / C_dense it is written into, or -1.  Within a row the
    last entry wins a slot, so an earlier entry of the same slot maps to -1.  A G entry between the Q and R parts (state row,
    control column or the reverse) lies outside every block: the device scatter drops it, so it maps to -1 here too."""
    n = S + C
    N = n * K - C
    slotG = np.full(len(G_col), -1, np.int64)
    slotC = np.full(len(C_col), -1, np.int64)
    for row in range(N):
        isr, off, owner = row % n, (row // n) * (S * S + C * C), {}
        for it in range(G_row[row], G_row[row + 1]):
            isc = int(G_col[it]) % n
            if (isr < S) != (isc < S):
                continue
            d = off + isc * S + isr if isc < S else off + S * S + (isc - S) * C + (isr - S)
            if d in owner:
                slotG[owner[d]] = -1
            owner[d] = it
            slotG[it] = d
    for row in range(S, S * K):
        br, owner = row // S - 1, {}
        for it in range(C_row[row], C_row[row + 1]):
            col = int(C_col[it])
            if col // n > br:
                continue
            d = br * (S * S + S * C) + (col % n) * S + row % S
            if d in owner:
                slotC[owner[d]] = -1
            owner[d] = it
            slotC[it] = d
    return slotG, slotC


def gather(dense, slots):
    out = np.zeros(len(slots), np.float64)
    m = slots >= 0
    out[m] = np.asarray(dense, np.float64)[slots[m]]
    return out


def scatter_kkt(s):
    """Dense [[G + rho I, C^T], [C, 0]] and [g; c] of the system the scatter builds (oracle.convert: the last entry of a slot
    wins, dropped entries are ignored, C's identity blocks implied) - synth.dense_kkt sums duplicates instead."""
    S, C, K = s.S, s.C, s.K
    Gd, Cd = o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, S, C, K, s.rho)
    Q, R = o.unpack_G(Gd, S, C, K)
    A, B = o.unpack_C(Cd, S, C, K)
    n, N = S + C, s.N
    G = np.zeros((N, N))
    Cm = np.zeros((S * K, N))
    Cm[:S, :S] = np.eye(S)
    for k in range(K):
        G[k * n: k * n + S, k * n: k * n + S] = Q[k]
        if k < K - 1:
            G[k * n + S: (k + 1) * n, k * n + S: (k + 1) * n] = R[k]
            Cm[(k + 1) * S: (k + 2) * S, k * n: k * n + S] = A[k]
            Cm[(k + 1) * S: (k + 2) * S, k * n + S: (k + 1) * n] = B[k]
            Cm[(k + 1) * S: (k + 2) * S, (k + 1) * n: (k + 1) * n + S] = np.eye(S)
    M = np.block([[G, Cm.T], [Cm, np.zeros((S * K, S * K))]])
    return M, np.concatenate([np.asarray(s.g, np.float64), np.asarray(s.c, np.float64)])


def dense_solve_and_adjoint(s, dz_bar, lam_bar, scatter=False):
    """fp64 dense forward (dz, lam) and adjoint (a, beta) of the system s (scipy via synth.dense_kkt; scatter=True:
    scatter_kkt, for patterns with duplicate or dropped entries)."""
    M, rhs = scatter_kkt(s) if scatter else synth.dense_kkt(s)
    x = np.linalg.solve(M, rhs)
    y = np.linalg.solve(M.T, np.concatenate([np.asarray(dz_bar, np.float64), np.asarray(lam_bar, np.float64)]))
    return x[: s.N], x[s.N:], y[: s.N], y[s.N:]


def dense_reference(s, dz_bar, lam_bar, scatter=False):
    """Full gradient of L with dL/ddz = dz_bar, dL/dlam = lam_bar from the dense solves: grads_math + the CSR value gradients."""
    dz, lam, a, beta = dense_solve_and_adjoint(s, dz_bar, lam_bar, scatter)
    out = grads_math(dz, lam, a, beta, s.S, s.C, s.K)
    Gd, Cd = grads_dense_layout(dz, lam, a, beta, s.S, s.C, s.K)
    sg, sc = csr_slot_map(s.G_row, s.G_col, s.C_row, s.C_col, s.S, s.C, s.K)
    out.update(G_dense=Gd, C_dense=Cd, G_val=gather(Gd, sg), C_val=gather(Cd, sc), g=a, dz=dz, lam=lam, a=a, beta=beta)
    return out


def blocks_of(s):
    """Math blocks (Q, R, A, B, q, r, c) of a CSR system (rho not added)."""
    Gd, Cd = o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, s.S, s.C, s.K, 0.0)
    Q, R = o.unpack_G(Gd, s.S, s.C, s.K)
    A, B = o.unpack_C(Cd, s.S, s.C, s.K)
    n = s.S + s.C
    g = np.asarray(s.g, np.float64)
    q = np.stack([g[k * n: k * n + s.S] for k in range(s.K)])
    r = np.stack([g[k * n + s.S: (k + 1) * n] for k in range(s.K - 1)])
    return Q, R, A, B, q, r, np.asarray(s.c, np.float64).reshape(s.K, s.S)
