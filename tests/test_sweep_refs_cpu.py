"""CPU suite: what the GPU sweeps (tests/test_gpu_resolve_sweep.py, tests/test_gpu_kkt_grad_sweep.py) lean on.

- Every named re-solve case is one the reference can carry: at its recorded seed the C oracle and the numpy oracle stop at the
  same iteration and agree to 1e-9 in lambda and dz for every (system, right-hand side), and no earlier seed does (the seed is
  the first of ten that passes; none needed the fixed-count fallback exit_tol = 0, max_iters = 8).
- Every case can tell two systems apart: the oracle's solutions of system b and of system (b + 1) % B on the same (g, c) are more
  than 1e-3 apart, so a kernel that reads another system's matrices is off at order 1, not at a rounding.
- The warm-start guesses are worth iterations in the oracle.
- csr_slot_map restates the scatter on every pattern of tests/csr_patterns.py."""
import numpy as np
import pytest

import csr_patterns as cp
import kkt_grad_ref as ref
import resolve_sweep_ref as R
from box_qp_polish_ref import SWEEP_SHAPES
from oracle import c_oracle as co
from oracle import gato_oracle as o

names = lambda cases: [c.name for c in cases]


def test_case_names_are_unique_and_one_per_route():
    assert len(R.BY_NAME) == len(R.ALL)
    assert all(c.B in (2, 3) and c.R in (2, 3) for c in R.ALL)
    assert set(R.DZ_LAUNCH) <= set(names(R.ROUTES))
    for shape in [(14, 7), (4, 2), (12, 6), (32, 16), (2, 1), (6, 3)]:          # the shapes the re-solve had not run at, and 14/7
        assert any((c.S, c.C) == shape for c in R.ROUTES), shape


@pytest.mark.parametrize("case", R.ALL, ids=names(R.ALL))
def test_the_two_oracles_agree_on_every_right_hand_side(case):
    for seed in range(case.seed):                                             # the recorded seed is the first that passes
        assert not R.carries(case, seed)[0], seed
    ok, rows = R.carries(case, case.seed)
    print(case.name, rows)
    assert ok, rows
    assert len(rows) == case.B * case.R
    assert all(row[2] > 0 for row in rows)                                     # no right-hand side is solved before the first iteration


@pytest.mark.parametrize("case", R.ALL, ids=names(R.ALL))
def test_two_systems_of_a_case_are_far_apart(case):
    d = R.distinct(case)
    print(case.name, "closest pair of systems on one right-hand side", d)
    assert d > R.DISTINCT


@pytest.mark.parametrize("case", R.WARM, ids=names(R.WARM))
def test_warm_guesses_save_iterations_in_the_oracle(case):
    S, C, K = case.S, case.C, case.K
    seen = set()
    for i, s2 in enumerate(s2 for per in case.inputs()[1] for s2 in per):
        n = o.linsys_solve(*s2.csr_args(), S, C, K, case.tol, case.mi, s2.rho, dtype=case.dt, return_all=True)
        lam0 = R.warm_guess(n["lam"].astype(np.float64), i).astype(case.dt)
        _, it = o.pcg(n["S"], n["Pinv"], n["gamma"], S, K, case.tol, case.mi, lam0=lam0)
        assert 0 < it < n["iters"], (i, it, n["iters"])
        seen.add(lam0.tobytes())
    assert len(seen) == case.B * case.R                                        # another guess per (b, r)


# ---- the slot map on the patterns of the gradient sweep -----------------------------------------------------------------------------
PATTERN_CASES = [(S, C, K, name) for (S, C), K in (((2, 1), 60), ((4, 2), 8), ((4, 2), 4), ((6, 3), 6), ((12, 6), 4), ((14, 7), 4),
                                                    ((32, 16), 4)) for name in sorted(cp.PATTERNS)]


def test_pattern_cases_cover_every_shape():
    assert {(S, C) for S, C, _, _ in PATTERN_CASES} == set(SWEEP_SHAPES)


@pytest.mark.parametrize("S,C,K,name", PATTERN_CASES, ids=["%d-%d-%d-%s" % c for c in PATTERN_CASES])
def test_slot_map_restates_the_scatter_on_every_pattern(S, C, K, name):
    """Every entry a distinct non-zero value, scattered by the C oracle at rho = 0: an entry with a slot put its value there, and
    the dense arrays hold as many non-zeros as there are slots - nothing else was written anywhere."""
    s = cp.pattern_system(name, S, C, K)
    assert np.all(np.diff(s.G_row) >= 0) and np.all(np.diff(s.C_row) >= 0) and s.G_row[-1] == len(s.G_col) and s.C_row[-1] == len(s.C_col)
    assert s.G_col.min() >= 0 and s.G_col.max() < s.N and s.C_col.min() >= 0 and s.C_col.max() < s.N
    assert np.all(np.diff(s.C_row)[:S] == 1)                                   # block row 0 as kkt_solve_csr reads S off it
    sg, sc = ref.csr_slot_map(s.G_row, s.G_col, s.C_row, s.C_col, S, C, K)
    Gv, Cv = 1.0 + np.arange(len(s.G_col)), -1.0 - np.arange(len(s.C_col))
    Gd, Cd = co.convert(s.G_row, s.G_col, Gv, s.C_row, s.C_col, Cv, S, C, K, 0.0, np.float64)
    Gd_n, Cd_n = o.convert(s.G_row, s.G_col, Gv, s.C_row, s.C_col, Cv, S, C, K, 0.0, np.float64)
    assert np.array_equal(Gd, Gd_n) and np.array_equal(Cd, Cd_n)
    assert np.array_equal(Gd[sg[sg >= 0]], Gv[sg >= 0]) and np.array_equal(Cd[sc[sc >= 0]], Cv[sc >= 0])
    assert np.count_nonzero(Gd) == len(set(sg[sg >= 0])) == (sg >= 0).sum()
    assert np.count_nonzero(Cd) == len(set(sc[sc >= 0])) == (sc >= 0).sum()
    k = cp.kinds(s, sg, sc)
    print(name, (S, C, K), k)
    assert k["block_row_0"] == S and k["identity"] > 0
    if name in ("duplicates", "combined"):
        assert k["overwritten_G"] > 0 and k["overwritten_C"] > 0
        # a duplicate far from its original: an overwritten entry whose winner is not the next entry of the row
        far = [e for e in np.flatnonzero(sg < 0) if s.G_col[e + 1] != s.G_col[e]]
        assert far
    if name in ("empty", "combined"):
        assert s.C_row[S] == s.C_row[S + 1] and s.C_row[-2] == s.C_row[-1]     # the first row of block row 1 and the last row: empty
        assert k["empty_C_rows"] >= 2 and k["diagonal_only_G_rows"] > 0
