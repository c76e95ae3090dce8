"""The one-workgroup fp64 solve (pcg_single_f64m_kernel), bit for bit against the commit before its launch was shortened OUTSIDE
the PCG loop.

The kernel loads gamma (and lambda0 of a warm start) ahead of the matrices and hands lambda to the dz helper blocks without
fences (write-through stores, drained, then the flag; pcg_single_f32x2_kernel does the same).  None of that - and no other
order or route of the loads outside the loop - may change lambda, dz or the iteration count of any solve:
tests/golden/f64m_outside_loop_parent.json holds SHA-256
digests recorded from the parent commit's library (tools/record_f64m_bits.py); cases in tests/f64m_outside_loop_cases.py.
Every solve starts from lambda and dz filled with NaN, so a helper block that read lambda before it was complete, a dz row
that no helper wrote, or a leftover in LDS that reached a result shows as a digest that differs."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import f64m_outside_loop_cases as fc               # noqa: E402  (tests/f64m_outside_loop_cases.py)

CASES = fc.all_cases()
IDS = [c[0] for c in CASES]
DEFAULT_ROUTE = dict(pair=2, image=1, dz_fused=2)       # mixed-rows kernel, transposed images, dz in the helper blocks
REPEATS = 6


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    with open(fc.GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("cid", IDS)
def test_default_route_has_the_parents_bits(golden, cid):
    got, route = fc.run_case(dict(CASES)[cid])
    print(cid, route, got["iters"], "iterations; differs from the parent's:", [k for k in got if got[k] != golden[cid][k]] or "nothing")
    assert route == DEFAULT_ROUTE, route
    assert got == golden[cid], cid


@pytest.mark.parametrize("cid", IDS)
def test_block_row_loads_and_dz_launch_have_the_parents_bits(golden, cid):
    """no_image = 1 (the block-row load path) with no_fuse_dz = 1 (dz in a launch of its own): the same bits."""
    got, route = fc.run_case(dict(CASES)[cid], no_image=1, no_fuse_dz=1)
    print(cid, route, got["iters"], "iterations")
    assert route == dict(pair=2, image=0, dz_fused=0), route
    assert got == golden[cid], cid


@pytest.mark.parametrize("cid", IDS)
def test_repeats_from_nan_filled_outputs(golden, cid):
    """Six solves on one solver, lambda and dz refilled with NaN before each: a helper that read lambda too early shows here."""
    case = dict(CASES)[cid]
    sv = fc.Solve(case["K"])
    runs = [sv.run(case["tol"], case["iters"]) for _ in range(REPEATS)]
    assert sv.route() == DEFAULT_ROUTE
    sv.close()
    bad = [i for i, r in enumerate(runs) if r != golden[cid]]
    print(cid, "repeats that differ from the parent's:", bad or "none")
    assert not bad, (cid, bad)


def test_small_solve_after_a_large_one(golden):
    """K = 50 then K = 33 on a second solver, three times: at K = 33 more than half of the two-row lanes own no rows, and LDS keeps
    what the K = 50 launch left there (the lanes without rows must read zeros, not leftovers)."""
    big, small = fc.Solve(50), fc.Solve(33)
    for rnd in range(3):
        for sv in (big, small):
            for tol, it in fc.STOPS:
                got = sv.run(tol, it)
                assert got == golden[fc.case_id(sv.K, tol, it)], (rnd, sv.K, tol, it)
    assert big.route() == DEFAULT_ROUTE and small.route() == DEFAULT_ROUTE
    big.close()
    small.close()


@pytest.mark.parametrize("K", [33, 50])
def test_true_warm_start_against_the_block_row_loads(K):
    """true_warm_start = 1 (the first product is S lambda0, so every load is waited for in front of it): images against no_image = 1."""
    lam0 = np.random.default_rng(K).standard_normal(fc.S * K)
    img, blk = fc.Solve(K, true_warm_start=1), fc.Solve(K, true_warm_start=1, no_image=1)
    for tol, it in fc.STOPS:
        runs = [img.run(tol, it, lam0) for _ in range(3)]
        want = blk.run(tol, it, lam0)
        print(K, tol, it, "iterations", want["iters"])
        assert all(r == want for r in runs), (K, tol, it)
    assert img.route() == DEFAULT_ROUTE and blk.route() == dict(pair=2, image=0, dz_fused=2)
    cold = fc.Solve(K)
    assert cold.run(*fc.STOPS[0]) != img.run(*fc.STOPS[0], lam0), "the guess must matter"
    for sv in (img, blk, cold):
        sv.close()


@pytest.mark.parametrize("K", [50, 33])
def test_under_uneven_load(golden, K):
    """The default route and its six repeats once more while a second stream copies a 1 GB buffer over and over: hand-offs between
    workgroups must hold when the memory system is busy with somebody else's traffic."""
    side = torch.cuda.Stream()
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    sv = fc.Solve(K)
    overlapped = 0
    for tol, it in fc.STOPS:
        for rep in range(1 + REPEATS):
            with torch.cuda.stream(side):
                for _ in range(3):                      # ~1 ms of copies per solve (a solve takes 0.2 - 0.5 ms)
                    dst.copy_(src, non_blocking=True)
                copied = torch.cuda.Event(enable_timing=True)
                copied.record(side)
            # (Solver launches on torch's CURRENT stream - Solver._stream() - which is where Event.record() records: the event
            #  completes behind the solve's last launch)
            solved = torch.cuda.Event(enable_timing=True)
            got = sv.run(tol, it, launched=solved.record)
            overlapped += solved.elapsed_time(copied) > 0       # the copies ended after the solve
            assert got == golden[fc.case_id(K, tol, it)], (K, tol, it, rep)
    print(K, "solves that ended while the copies were still running:", overlapped, "of", 2 * (1 + REPEATS))
    assert overlapped > 0, "no solve ran beside the copies: the test checked nothing under load"
    assert sv.route() == DEFAULT_ROUTE
    sv.close()


@pytest.mark.parametrize("K", [9, 50, 73])
def test_fp32_helper_blocks_against_the_dz_launch(K):
    """pcg_single_f32x2_kernel hands lambda to the same helper blocks: dz from them against no_fuse_dz = 1, six repeats from NaN."""
    fused, plain = fc.Solve(K, np.float32), fc.Solve(K, np.float32, no_fuse_dz=1)
    for tol, it in ((0.0, 30), (1e-5, 100)):
        want = plain.run(tol, it)
        runs = [fused.run(tol, it) for _ in range(REPEATS)]
        bad = [i for i, r in enumerate(runs) if r != want]
        print(K, tol, it, "iterations", want["iters"], "repeats that differ:", bad or "none")
        assert not bad, (K, tol, it, bad)
    assert fused.route() == dict(pair=1, image=fused.route()["image"], dz_fused=2), fused.route()
    assert plain.route()["pair"] == 1 and plain.route()["dz_fused"] == 0, plain.route()
    fused.close()
    plain.close()
