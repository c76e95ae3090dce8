"""What the CPU and GPU tests of the box QP with a cross term share: the problems and their references.

A problem is a cell of cross_ref (blocks of synth.make_blocks, M of synth.make_cross) with a box.  Its reference is
box_qp_ref.admm on the dense H = G + rho I with M_k, M_k^T in place (cross_ref.dense_kkt) - the reference iteration takes any H,
so it needs no new algorithm.  Every problem and every reference run is computed once (lru_cache) and must not be written."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import cross_ref as X                             # noqa: E402
from gato_python_amd import synth                 # noqa: E402

RHO = X.RHO
ADMM_RHO = 10.0                                   # the synthetic systems' scale (Q up to 1e3) wants a stiffer penalty than 0.1
PARITY_ITERS = 25
PARITY_CELLS = [(S, C, K) for S, C in X.SHAPES for K in (2, 3, 9)]
CONVERGED_CELLS = [(2, 1, 3), (4, 2, 9), (14, 7, 9), (14, 7, 50), (32, 16, 3)]
CONVERGED_CAP = 1000                              # ADMM iterations the reference may take on a converged cell
STRIDE_CELL = (2, 1, 8197)                        # the second pass of the knot stride (grid.x = 8192)
STRIDE_ITERS = 3
BATCH_CELL = (4, 2, 9)                            # the B = 3 parity batch: system 1 dense Q, system 2 M = 0


def cross_parts(blocks, M, rho=RHO):
    """(H, C, g, c) dense, H = G + rho I with the cross blocks in place (M None: none)."""
    Q, R, A, B, q, r, c = blocks
    N = (Q.shape[1] + R.shape[-1]) * Q.shape[0] - R.shape[-1]
    Mat = X.dense_kkt(Q, R, A, B, M, rho)
    _, _, g, cc = X.pack(Q, R, A, B, q, r, c)
    return Mat[:N, :N].copy(), Mat[N:, :N].copy(), g, cc


def cross_parts_sparse(s, M):
    """(H, C, g, c) as scipy.sparse CSR matrices from the system's CSR arrays, H with M_k and M_k^T added: the long horizons."""
    from scipy import sparse
    H, Cm, g, c = ref.sparse_parts(s)
    K1, S, C = M.shape
    n = S + C
    rows = (np.arange(K1)[:, None, None] * n + np.arange(S)[None, :, None] + np.zeros((1, 1, C), np.int64)).reshape(-1)
    cols = (np.arange(K1)[:, None, None] * n + S + np.arange(C)[None, None, :] + np.zeros((1, S, 1), np.int64)).reshape(-1)
    X_ = sparse.coo_matrix((M.reshape(-1), (rows, cols)), shape=H.shape)
    return (H + X_ + X_.T).tocsr(), Cm, g, c


def full_box(s, seed, dz):
    """A box in the manner of box_qp_polish_ref.boxes around the unconstrained solution dz: the controls and every other state
    bounded (x_0 free), and one control fixed (lo == hi) - on knot K // 2, or on the last knot that has a control."""
    lo, hi = P.boxes(s, seed, eq=False, dz=dz)
    j = s.S + (s.S + s.C) * min(s.K // 2, s.K - 2)
    lo[j] = hi[j] = 0.25 * dz[j]
    return lo, hi


def control_box(s, seed, dz):
    """The same with every state free and no fixed control: the box under which ADMM converges within CONVERGED_CAP."""
    return P.boxes(s, seed, eq=False, states=False, dz=dz)


@functools.lru_cache(maxsize=None)
def problem(S, C, K, seed=0, dense_q=False, box="full", zero_M=False, sparse=False):
    """One problem as a dict: blocks, M [K-1,S,C], s (the KKTSystem of the blocks, without M, for the device inputs), H, Cm, g, c
    (H with M; H0 without), lo, hi.  box: "full" or "controls".  zero_M: M = 0.  sparse: H, Cm are scipy.sparse."""
    blocks, M = X.cell(S, C, K, seed=seed, dense_q=dense_q)
    if zero_M:
        M = np.zeros_like(M)
    s = synth.blocks_to_csr(*blocks, rho=RHO, dense_q=dense_q)
    if sparse:
        H, Cm, g, c = cross_parts_sparse(s, M)
        H0 = ref.sparse_parts(s)[0]
    else:
        H, Cm, g, c = cross_parts(blocks, M)
        H0 = cross_parts(blocks, None)[0]
    inf = np.full(s.N, np.inf)
    dz = ref.kkt_solver(H, Cm)(np.concatenate([g, c]))[:s.N]               # the unconstrained solution with M
    lo, hi = (full_box if box == "full" else control_box)(s, seed + 500, dz)
    assert inf.shape == lo.shape
    return dict(blocks=blocks, M=M, s=s, H=H, H0=H0, Cm=Cm, g=g, c=c, lo=lo, hi=hi)


@functools.lru_cache(maxsize=None)
def reference(key, with_M=True, **admm):
    """box_qp_ref.admm on problem(*key) with the cross H (with_M False: without M), admm given as keyword settings."""
    p = problem(*key)
    return ref.admm(p["H"] if with_M else p["H0"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], **admm)


def parity_reference(key, with_M=True, iters=PARITY_ITERS, **admm):
    """The iterate after `iters` x-steps: eps 0, so the test never passes."""
    return reference(key, with_M, eps_abs=0.0, eps_rel=0.0, max_admm_iters=iters, **admm)


def parity_keys():
    """The keys of problem() of the iterate-parity test: the six shapes at K = 2, 3, 9 with full boxes."""
    return [(S, C, K, K, False, "full") for S, C, K in PARITY_CELLS]


def batch_keys():
    """The B = 3 parity batch: three systems of one shape, system 1 with dense Q, system 2 with M = 0."""
    S, C, K = BATCH_CELL
    return [(S, C, K, 60, False, "full"), (S, C, K, 77, True, "full"), (S, C, K, 94, False, "full", True)]


def converged_keys(seeds=(0, 17)):
    """The converged-solve problems: CONVERGED_CELLS with control-only boxes."""
    return [(S, C, K, seed, False, "controls") for S, C, K in CONVERGED_CELLS for seed in seeds]
