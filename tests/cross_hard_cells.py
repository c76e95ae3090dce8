"""The hard cells of the cross-term suites (tests/test_cross_hard_cpu.py, tests/test_gpu_cross_hard.py; DESIGN.md sections 3.15 to
3.17): asm_ref.hard_blocks - dense SPD Q_k and R_k of condition 100, every block on its own power-of-two scale, A_k far from the
identity, c_0 != 0 - with the M of synth.make_cross on them.  Everything cross_ref.cell leaves out: there R_k is diagonal (the
Gauss-Jordan of cross_prepare inverts a diagonal matrix, the control rows of H x have no off-diagonal term), A_k is nearly -I and
every knot has the same scale (W_k-1 for W_k costs little).

The box QPs on them are box_qp_cross_ref's boxes around the dense solution of the hard cell; every problem and every reference
run is computed once (lru_cache) and must not be written.  A plain module: the lists below are the cells of the GPU file, and
the CPU file asserts the conditioning, the convergence and the references' own agreement on every one of them."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import asm_ref                                    # noqa: E402
import box_qp_cross_ref as XR                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
import cross_ref as X                             # noqa: E402
from gato_python_amd import synth                 # noqa: E402

RHO = X.RHO
GRADE = asm_ref.GRADE
SHAPES = X.SHAPES


def hard_cell(S, C, K, seed, grade):
    """(blocks, M) of one system: asm_ref.hard_blocks at condition 100 and the given grade, M of synth.make_cross at scale 0.5."""
    blocks = asm_ref.hard_blocks(S, C, K, seed, asm_ref.COND, grade)
    return blocks, synth.make_cross(blocks[0], blocks[1], seed=seed + 1000, scale=0.5)


def hard_batch(S, C, K, B, grade):
    """B different systems of one shape: seeds 0 .. B-1."""
    return [hard_cell(S, C, K, b, grade) for b in range(B)]


def grade_of(dt):
    return GRADE[np.dtype(dt).name]


# ---- the cells of tests/test_gpu_cross_hard.py -------------------------------------------------------------------------------
KERNEL_K = (2, 3, 5)                              # (a), (b): all SHAPES x these, B = 3
SOLVE_K, SOLVE_B = (2, 9), (1, 3)                 # (c): all SHAPES x these
SOLVE_CELLS = [(S, C, K) for S, C in SHAPES for K in SOLVE_K]
RESOLVE_CELLS = [(4, 2, 3), (14, 7, 9), (32, 16, 3)]         # (c) solve_rhs_cross and (g) tangents
GRAD_CELLS = [(6, 3, 5), (14, 7, 9), (32, 16, 3)]            # (d), B = 3
FD_CELLS = [(4, 2, 3), (6, 3, 5)]                 # the CPU suite's central differences, grade 0
PARITY_CELLS = [(S, C, K) for S, C in SHAPES for K in (2, 3, 9)]   # (e), seed 0, grade 4
BATCH_CELL = (4, 2, 9)                            # (e) B = 3: seed 1 has M = 0, seed 2 a control-only box
CONVERGED_CELLS = [(2, 1, 3), (4, 2, 9), (12, 6, 3), (32, 16, 3)]  # (f), seed 0, grade 0, control-only boxes
CONVERGED_F32 = CONVERGED_CELLS[:2]               # (f) in fp32, eps 1e-4


# ---- box QPs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(S, C, K, seed=0, grade=4, box="full", zero_M=False, dt="float64"):
    """box_qp_cross_ref.problem on a hard cell: blocks, M, s (the KKTSystem of the blocks without M, for the device inputs), H with
    M and H0 without, Cm, g, c, lo, hi.  The box is box_qp_cross_ref.full_box ("full") or control_box ("controls") around the
    dense solution with M.  dt = "float32": every value of the blocks and M rounded to float32 first (what an fp32 device is
    given; the box is rounded by the device helper)."""
    blocks, M = hard_cell(S, C, K, seed, grade)
    if zero_M:
        M = np.zeros_like(M)
    if dt == "float32":
        r32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
        blocks, M = tuple(r32(b) for b in blocks), r32(M)
    s = synth.blocks_to_csr(*blocks, rho=RHO, dense_q=True)
    H, Cm, g, c = XR.cross_parts(blocks, M)
    H0 = XR.cross_parts(blocks, None)[0]
    dz = ref.kkt_solver(H, Cm)(np.concatenate([g, c]))[:s.N]
    lo, hi = (XR.full_box if box == "full" else XR.control_box)(s, seed + 500, dz)
    return dict(blocks=blocks, M=M, s=s, H=H, H0=H0, Cm=Cm, g=g, c=c, lo=lo, hi=hi)


@functools.lru_cache(maxsize=None)
def reference(key, with_M=True, **admm):
    """box_qp_ref.admm on problem(*key), with the cross H or (with_M False) the H without M."""
    p = problem(*key)
    return ref.admm(p["H"] if with_M else p["H0"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], **admm)


def parity_reference(key, with_M=True):
    """The iterate after PARITY_ITERS x-steps at eps 0 and admm_rho = 10."""
    return reference(key, with_M, eps_abs=0.0, eps_rel=0.0, max_admm_iters=XR.PARITY_ITERS, admm_rho=XR.ADMM_RHO)


def parity_keys():
    return [(S, C, K, 0, GRADE["float64"], "full") for S, C, K in PARITY_CELLS]


def batch_keys():
    S, C, K = BATCH_CELL
    g = GRADE["float64"]
    return [(S, C, K, 0, g, "full"), (S, C, K, 1, g, "full", True), (S, C, K, 2, g, "controls")]


def converged_keys(dt="float64"):
    return [(S, C, K, 0, 0, "controls", False, dt) for S, C, K in (CONVERGED_CELLS if dt == "float64" else CONVERGED_F32)]


def at_bound(out, p):
    """Per variable: the reference's z sits on a finite bound."""
    return (out["z"] == p["lo"]) | (out["z"] == p["hi"])


def knots_with_a_control_at_a_bound(out, p):
    """[K-1] bools: some control of full knot k has z on a bound."""
    s = p["s"]
    n = s.S + s.C
    hit = at_bound(out, p)
    return np.array([hit[k * n + s.S:(k + 1) * n].any() for k in range(s.K - 1)])
