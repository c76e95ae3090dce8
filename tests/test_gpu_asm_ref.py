"""gather_kernel, invert_G_kernel, schur_kernel, ss_kernel, dz_kernel and the fused assemble_kernel against the dense longdouble
reference of tests/asm_ref.py, on inputs with dense graded Q_k and R_k, A_k far from the identity and c_0 != 0: every compiled
shape, the knot edges K = 1, 2, 3, 5, both dtypes, per block, beside the two CPU orders' own errors (the bar and where its factor
and floor come from: tests/asm_ref.py; that it holds between the CPU orders and that a subtly wrong assembly breaks it:
tests/test_asm_ref_cpu.py).  Every test prints the per-buffer errors and ratios (pytest -s; tools/asm_accuracy.py records them).

Measured on the MI355X over all cases below (profiles/asm_accuracy.json): device / max(worse CPU order, floor) is at most 1.83
(gamma, 4/2/5 fp32) where both CPU orders set the bar, and 3.71 in one buffer of the long horizon, where the C order alone does
(block-Jacobi Pinv, fp32: 120 eps against the C order's 32; in fp64 the same buffer is at 0.35).  The factor stays the 4 of the
CPU measurement."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import asm_ref as ar                               # noqa: E402  (tests/asm_ref.py)
from gato_python_amd import _lib                   # noqa: E402
from gato_python_amd.solver import Solver         # noqa: E402
from oracle import gato_oracle as o                # noqa: E402

STAGE = ar.stage_cases()
sid = lambda c: ar.case_id(*c)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()                                    # the HIP library must be the thing that runs


@pytest.mark.parametrize("case", STAGE, ids=sid)
def test_stage_entries(case):
    """convert bit for bit; form_schur (its own inversions), form_ss and compute_dz each on the rounded reference outputs of the
    stage before it: Ginv, S, block-Jacobi Pinv, gamma, stair Pinv, dz."""
    S, C, K, dt = case
    got, e_dev, e_or = ar.device_stage_case(S, C, K, dt)
    Gd, Cd = ar.expected_dense(ar.blocks_of(S, C, K, dt), ar.RHO, dt)
    assert np.array_equal(got["G_dense"], Gd) and np.array_equal(got["C_dense"], Cd)
    assert ar.pinv0_is_minus_q0(got["Pinv_bj"], Gd, S)
    assert ar.judge(f"stages {sid(case)}", dt, e_dev, e_or, ar.STAGE_BUFFERS) == []


@pytest.mark.parametrize("case", STAGE, ids=sid)
def test_whole_calls(case):
    """linsys through the stage launches (asm_mode 1) and through the fused launch (asm_mode 2), one PCG iteration: the solver's
    own Ginv, S, Pinv, gamma.  fp64: a converged solve against the longdouble KKT solution at BASELINE's bar."""
    S, C, K, dt = case
    s, ref = ar.system_of(S, C, K, dt), ar.reference_of(S, C, K, dt)
    Gd, _ = ar.expected_dense(ar.blocks_of(S, C, K, dt), ar.RHO, dt)
    e_or = ar.oracle_chain_errors(S, C, K, dt)
    for mode in (1, 2):
        sol = Solver(S, C, K, np.dtype(dt))
        got = ar.whole_call(sol, s, mode)
        assert got["fused"] == mode - 1
        assert ar.pinv0_is_minus_q0(got["Pinv"], Gd, S)
        bad = ar.judge(f"linsys asm_mode {mode} {sid(case)}", dt, ar.errors(got, ref.buf, S, C, K, ar.WHOLE_BUFFERS), e_or, ar.WHOLE_BUFFERS)
        if dt == "float64":
            conv = ar.whole_call(sol, s, mode, ar.EXIT_TOL, ar.MAX_ITERS)
            ez = float(np.abs(conv["dz"] - ref.dz_kkt).max())
            el = float(np.abs(conv["lam"] - ref.lam_kkt).max() / np.abs(ref.lam_kkt).max())
            print(f"converged solve asm_mode {mode} {sid(case)}: |dz - dz_ref|_inf {ez:.1e}, lambda {el:.1e} relative")
            assert ez < 1e-6 and el < 1e-6
        sol.close()
        assert bad == []


@pytest.mark.parametrize("dt", ar.DTYPES)
@pytest.mark.parametrize("S,C,K", ar.BLOCKS_CASES)
def test_linsys_blocks(S, C, K, dt):
    """Direct block input (rho not yet added): asm_mode 1, 2 and 3 (a value the fused launch does not claim: the stage launches)."""
    s, ref = ar.system_of(S, C, K, dt), ar.reference_of(S, C, K, dt)
    Gd, Cd = ar.expected_dense(ar.blocks_of(S, C, K, dt), 0.0, dt)
    Gd_rho, _ = ar.expected_dense(ar.blocks_of(S, C, K, dt), ar.RHO, dt)
    e_or = ar.oracle_chain_errors(S, C, K, dt)
    for mode in (1, 2, 3):
        sol = Solver(S, C, K, np.dtype(dt))
        got = ar.whole_call(sol, s, mode, blocks=(Gd, Cd))
        assert got["fused"] == (mode == 2)
        assert np.array_equal(sol.read_buffer("G_dense"), Gd_rho) and ar.pinv0_is_minus_q0(got["Pinv"], Gd_rho, S)
        sol.close()
        assert ar.judge(f"linsys_blocks asm_mode {mode} {S}-{C}-{K}-{dt}", dt, ar.errors(got, ref.buf, S, C, K, ar.WHOLE_BUFFERS), e_or,
                        ar.WHOLE_BUFFERS) == []


@pytest.mark.parametrize("dt", ar.DTYPES)
@pytest.mark.parametrize("S,C,K", ar.BATCH_CASES)
def test_batches_of_different_systems(S, C, K, dt):
    """B = 3 different hard systems in one linsys_batched call, stage launches and fused launch: each system's share of every
    work buffer against that system's own reference (a wrong batch stride reads a neighbour's blocks)."""
    bad = []
    for mode in (1, 2):
        fused, per_system = ar.device_batch_case(S, C, K, dt, mode)
        assert fused == mode - 1
        for b, (e, e_or) in enumerate(per_system):
            bad += ar.judge(f"batch asm_mode {mode} system {b} {S}-{C}-{K}-{dt}", dt, e, e_or, ar.WHOLE_BUFFERS)
    assert bad == []


@pytest.mark.parametrize("dt", ar.DTYPES)
def test_stage_entries_past_the_grid_caps(dt):
    """2/1/16400: the Schur, stair and dz launches wrap their 8192 workgroups twice, the inversion launch once; ten knots around
    each wrap and the last ten against each window's dense reference, the whole horizon finite, convert bit for bit."""
    S, C, K = ar.LONG
    got, want, e_dev, e_or, (Gd, Cd) = ar.long_horizon_case(dt)
    assert np.array_equal(got["G_dense"], Gd) and np.array_equal(got["C_dense"], Cd)
    assert all(np.all(np.isfinite(got[n])) for n in ar.STAGE_BUFFERS)
    assert ar.judge(f"stages {S}-{C}-{K}-{dt}, windows at {ar.LONG_WINDOWS}", dt, e_dev, e_or, ar.STAGE_BUFFERS) == []


@pytest.mark.parametrize("dt", ar.DTYPES)
@pytest.mark.parametrize("S,C,K", [(4, 2, 3), (14, 7, 5), (32, 16, 2)])
def test_precon_modes(S, C, K, dt):
    """Block-Jacobi: the off-diagonal blocks of Pinv exactly zero, the main blocks against the reference.  Point-Jacobi: 1 / S_ii
    of the device's own S, bit for bit, zeros elsewhere."""
    s, ref = ar.system_of(S, C, K, dt), ar.reference_of(S, C, K, dt)
    e_or = ar.oracle_chain_errors(S, C, K, dt)
    sol = Solver(S, C, K, np.dtype(dt))
    sol.set_option("precon_mode", _lib.PRECON_BLOCK_JACOBI)
    got = ar.whole_call(sol, s, 0)
    assert got["fused"] == 0
    P = got["Pinv"].reshape(K, 3, S * S)
    assert not P[:, 0].any() and not P[:, 2].any()
    e = ar.errors(dict(got, Pinv_bj=got["Pinv"]), ref.buf, S, C, K, ("S", "Pinv_bj"))
    bad = ar.judge(f"block-Jacobi {S}-{C}-{K}-{dt}", dt, e, e_or, ("S", "Pinv_bj"))
    sol.set_option("precon_mode", _lib.PRECON_POINT_JACOBI)
    got = ar.whole_call(sol, s, 0)
    sol.close()
    assert got["fused"] == 0
    assert np.array_equal(got["Pinv"], o.point_jacobi(got["S"], S, K))
    assert bad == []
