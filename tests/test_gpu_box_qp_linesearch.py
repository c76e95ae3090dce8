"""The exact line search of the soft active-set iteration on the device (gato_box_qp_pdas_ls, gato_box_qp_line_search,
Solver.box_qp_pdas(line_search=True), Solver.box_qp_line_search, box_qp / box_qp_layer(method="pdas", line_search=True); DESIGN.md
section 3.12) against the numpy reference of tests/box_qp_linesearch_ref.py (tests/test_box_qp_linesearch_cpu.py asserts that
every case here has a seed).  The kernels alone: the step length on the reference's linear piece and the reference's slope at
it within SLACK N eps scale, the summation bound.  End to end: the reference's solves, acts and full steps, fp64 parity 1e-6 in
the infinity norm, penalised KKT residuals <= 1e-7, the same bits on a repeat."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_linesearch_ref as L                 # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import (CAP, F64, SENTINEL, check_point, check_search, dev_inputs, ls_bits, ls_converges_case, ls_fp32_case,  # noqa: E402
                           ls_layer_gradients_case, ls_run, math_inputs, sentinels, solver)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


# ---- 1. the two kernels alone --------------------------------------------------------------------------------------------------
KERNEL = [(S, C, K, dt, form) for S, C, K in L.CAPPED_CASES for dt in (np.float64, np.float32) for form in (L.CAPPED, L.UNCAPPED)]


@pytest.mark.parametrize("S,C,K,dt,form", KERNEL, ids=["%d-%d-%d-%s-%s" % (S, C, K, np.dtype(dt).name, "capped" if f[1] else "uncapped")
                                                       for S, C, K, dt, f in KERNEL])
def test_line_search_kernels(S, C, K, dt, form):
    """A damped search, a full step and a second damped search, alone (B = 1) and as a batch of three systems."""
    batch = L.kernel_batch(S, C, K, form, dt)
    assert batch, "no inputs at %d/%d/%d" % (S, C, K)
    one = check_search(solver(S, C, K, dt), batch[:1], dt, with_caps=form[1] is not None)
    full = check_search(solver(S, C, K, dt), batch[1:2], dt, with_caps=form[1] is not None)
    three = check_search(solver(S, C, K, dt, batch=3), batch, dt)
    print("largest slope / (N eps scale)", max(one, full, three))


def test_line_search_kernels_past_the_grid_cap():
    """2/1/8197, inputs from the sparse reference's second solve: the knot kernel's second grid pass and the system kernel's
    strided passes (N = 24590 over 256 threads).  Among 24590 variables some x_i always lies within 1e-5 of a bound (seed 3: the
    margins of its first twelve solves are 2e-8 to 7e-6), so no decision margin is asked of the solve: this test checks the
    step length and the slope, which read no act, and search_inputs still keeps the root off the ends of its linear piece."""
    cases = L.kernel_inputs(*D.LONG, L.CAPPED, np.float64, True, sparse=True)
    assert cases and D.LONG[2] > CAP
    print("largest slope / (N eps scale)", check_search(solver(*D.LONG, np.float64), cases, np.float64))


# ---- 2. end to end, fp64 -------------------------------------------------------------------------------------------------------
E2E = [(c, L.CAPPED) for c in L.CAPPED_CASES] + [(c, L.UNCAPPED) for c in L.UNCAPPED_CASES]


@pytest.mark.parametrize("case,form", E2E, ids=["%d-%d-%d-%s" % (c + ("capped" if f[1] else "uncapped",)) for c, f in E2E])
def test_line_search_converges_where_the_undamped_iteration_does_not(case, form):
    """The reference's number of solves over the reference's act sequence (the act of solve j is that of a run stopped after j
    solves), alpha exactly 1 where the reference's is and inside (0, 1) elsewhere, x and lambda within 1e-6, the penalised KKT
    residuals <= 1e-7, the same bits again; without the option MAX_ITERS and nothing written."""
    S, C, K = case
    ps = L.ls_box(S, C, K, form)
    assert ps, "the walk finds no seed"
    ls_converges_case(ps[0])


@pytest.mark.parametrize("S,C,K", L.F32_CASES, ids=["%d-%d-%d" % c for c in L.F32_CASES])
def test_fp32_follows_the_reference(S, C, K):
    """fp32 at eps = F32_EPS and the PCG exit tolerance F32_EXIT_TOL, where the fp32 restatement follows the reference's acts:
    the reference's solves, final act and full steps."""
    ps = L.ls_box(S, C, K, L.CAPPED, f32=True)
    assert ps, "the walk finds no seed"
    ls_fp32_case(ps[0])


# ---- 3. batches, warm starts, refusals -----------------------------------------------------------------------------------------
BATCH = (6, 3, 9)


def test_batch_of_five_with_a_bad_cap_and_a_hard_bound():
    """Two line-search problems that freeze at different solves (0, 1), one that takes full steps throughout (2), one with a NaN
    cap (3) and one with a finite hard bound (4): the call raises, marks 3 and 4 BAD_BOUNDS and writes nothing.  With the two
    made valid, every system has the bits of its solo run."""
    S, C, K = BATCH
    found = L.ls_box(S, C, K, L.CAPPED, count=4)
    a = found[0]
    b = next(p for p in found[1:] if p["run"]["iters"] != a["run"]["iters"])
    full = L.full_step_box(S, C, K)
    c, d = [p for p in found if p is not a and p is not b][:2]
    n, N = S + C, a["s"].N
    bad_cap = dict(c, m=np.where(np.arange(N) == n, np.nan, c["m"]))
    hard = dict(d, w=np.where(np.arange(N) == n + S, 0.0, d["w"]))
    assert np.isfinite(d["lo"][n + S]) or np.isfinite(d["hi"][n + S])
    sol = solver(S, C, K, np.float64, batch=5)
    outs = sentinels(sol)
    with pytest.raises(ValueError, match=r"systems \[3, 4\].*soft bounds only.*BAD_BOUNDS"):
        ls_run(sol, [a, b, full, bad_cap, hard], outs=outs)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs.values()) and sol.get_option("assembly_valid") == 0
    ps = [a, b, full, c, d]
    r = ls_run(sol, ps, outs=outs)
    print("status", r.status.tolist(), "iters", r.iters.tolist())
    for i, p in enumerate(ps):
        one = solver(S, C, K, np.float64)
        solo = ls_run(one, [p], outs=sentinels(one))
        assert int(r.status[i]) == _lib.QP_CONVERGED and int(r.iters[i]) == p["run"]["iters"]
        assert ls_bits(r, i, sol) == ls_bits(solo, 0, one), i
        check_point(sol, r, i, p, p["run"])
    assert set(r.alpha[2, :full["run"]["iters"] - 1].tolist()) == {1.0}


def test_warm_start_from_the_converged_act():
    p = L.ls_box(*BATCH, L.CAPPED)[0]
    sol = solver(*BATCH, np.float64)
    warm = ls_run(sol, [p], act=p["run"]["act"])
    assert int(warm.iters[0]) == 1 and warm.alpha[0].tolist() == [0.0] * 30
    check_point(sol, warm, 0, p, dict(p["run"], iters=1))


def test_python_entries():
    """box_qp(line_search=True) is the solver call; the refusals that need the device."""
    import gato_python_amd
    p = L.ls_box(*BATCH, L.CAPPED)[0]
    s = p["s"]
    ts = math_inputs(p)
    r = gato_python_amd.box_qp(*ts[:11], rho=s.rho, method="pdas", x_soft=ts[11], u_soft=ts[12], x_soft_max=ts[13], u_soft_max=ts[14],
                               line_search=True, **F64)
    sol = solver(*BATCH, np.float64)
    want = ls_run(sol, [p])
    assert int(r.status) == _lib.QP_CONVERGED and r.alpha.shape == (30,)
    assert torch.equal(r.x, want.x) and torch.equal(r.lam, want.lam) and torch.equal(r.alpha, want.alpha[0])
    with pytest.raises(ValueError, match="soft bounds only"):        # the controls keep their hard bounds
        gato_python_amd.box_qp(*ts[:11], rho=s.rho, method="pdas", x_soft=ts[11], line_search=True, **F64)
    with pytest.raises(ValueError, match="soft bounds only"):
        gato_python_amd.box_qp_layer(*ts[:11], rho=s.rho, method="pdas", x_soft=ts[11], line_search=True, **F64)
    with pytest.raises(ValueError, match="line_search=True needs soft_weight"):
        sol.box_qp_pdas(*dev_inputs(sol, [s], [(p["lo"], p["hi"])]), rho=s.rho, line_search=True, **F64)


# ---- 4. the layer --------------------------------------------------------------------------------------------------------------
LAYER = [c + (st,) for c in L.LAYER_CASES for st in (False, True)]


@pytest.mark.parametrize("S,C,K,stale", LAYER, ids=["%d-%d-%d-%s" % (S, C, K, "stale" if st else "fresh") for S, C, K, st in LAYER])
def test_layer_gradients(S, C, K, stale):
    """box_qp_layer(line_search=True): all fifteen gradients against the reference through the final act, err < 1e-6 max(1,
    |want|).  stale: another solve on the cached solver between the passes; the backward pass rebuilds its assembly with one
    solve on the saved act, without the option."""
    ls_layer_gradients_case(L.ls_box(S, C, K, L.CAPPED)[0], stale, D.control_box(S, C, K)[0])
