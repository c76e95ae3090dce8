"""GPU suite: the opt-in true warm start (solver option true_warm_start = 1: lambda is also the initial guess, r0 = gamma - S lambda0)
on every one-GPU entry that holds it, against the numpy oracle started from the SAME lambda0 (oracle.gato_oracle.pcg / linsys_solve
with lam0, pinned on the CPU by tests/test_oracle.py).  The reference has no such option (D5), so these comparisons are its only pin.

fp64: the oracle's exit iteration and rel < 1e-9.  fp32: iterations within 2 of the fp32 oracle's, lambda / dz judged by check_f32
against the fp64 run on the fp32-rounded system from the same lambda0 - after the same fixed number of iterations (exit_tol = 0),
where both recurrences are still far from rounding level.  Every case also checks that lambda0 = 0 with the option on gives the
bits of the cold solve (r0 = gamma - S 0 = gamma exactly), and which kernel ran (last_pair / last_groups / last_mode)."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from gato_python_amd import _lib, synth                 # noqa: E402
from oracle import gato_oracle as o                     # noqa: E402
from f32_parity import check_f32                        # noqa: E402

F64_BAR = 1e-9
FIXED = 12                                              # fp32: iterations of the fixed-count comparison


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def rel(a, b, floor=1e-300):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def system(S, C, K, seed):
    if K == 1:
        return synth.blocks_to_csr(*synth.make_blocks(S, C, 1, seed, False))
    return synth.make_system(S, C, K, seed=seed)


def solver(S, C, K, dt, batch=1, **opts):
    from gato_python_amd.solver import Solver
    sol = Solver(S, C, K, dt, batch=batch)
    for k, v in opts.items():
        sol.set_option(k, v)
    return sol


def tol_mi(dt):
    return (1e-10, 300) if dt == np.float64 else (1e-5, 100)


def read_iters(sol, n=1):
    buf = (ct.c_int * n)()
    torch.cuda.synchronize()
    assert ct.CDLL("libamdhip64.so").hipMemcpy(buf, ct.c_void_p(sol.buffer_ptr(8)), 4 * n, 2) == 0
    return list(buf)


def oracle_solve(s, dt, tol, mi, lam0, rounded=False):
    """The numpy oracle's whole solve from lam0: in dt, or (rounded) in fp64 on the fp32-rounded system and guess."""
    if rounded:
        s64 = s.astype(np.float32).astype(np.float64)
        return o.linsys_solve(*s64.csr_args(), s.S, s.C, s.K, tol, mi, float(np.float32(s.rho)), dtype=np.float64,
                              lam0=np.asarray(lam0, np.float32).astype(np.float64))
    return o.linsys_solve(*s.csr_args(), s.S, s.C, s.K, tol, mi, s.rho, dtype=dt, lam0=np.asarray(lam0, dt))


def guesses(s, n, seed):
    """n initial guesses near the solution (0.9 x it + noise), in fp64; guess 0 is the converged solution itself."""
    lam_x = o.linsys_solve(*s.csr_args(), s.S, s.C, s.K, 1e-20, 2000, s.rho, dtype=np.float64)[0]
    rng = np.random.default_rng(seed)
    sc = np.abs(lam_x).max()
    return [lam_x] + [0.9 * lam_x + 0.05 * sc * rng.standard_normal(lam_x.size) for _ in range(n - 1)]


def judge(tag, s, dt, tol, mi, lam0, lam, dz, it, run_fixed=None):
    """One warm solve (lam, dz, it) against the oracle from the same lam0.  run_fixed(n) -> (lam, dz): the same solve with
    exit_tol = 0 and n iterations (fp32 only)."""
    lam_o, dz_o, it_o = oracle_solve(s, dt, tol, mi, lam0)
    if dt == np.float64:
        # dz relative to max(|dz|, 1): at K = 1 the solution's dz is rounding noise (~1e-18).  K = 2 (28 unknowns) is
        # ill-conditioned enough that the iterate stopped at exit_tol depends on the summation order: the numpy and the C oracle,
        # same recurrence, differ by 3.6e-6 in dz there - held to the bar of the one-knot-per-rank cluster tests instead.
        bl, bz = (1e-5, 1e-4) if s.K == 2 else (F64_BAR, F64_BAR)
        assert it == it_o, (tag, it, it_o)
        assert rel(lam, lam_o) < bl and rel(dz, dz_o, 1.0) < bz, (tag, rel(lam, lam_o), rel(dz, dz_o, 1.0))
        return it_o
    assert abs(it - it_o) <= 2, (tag, it, it_o)
    if run_fixed is not None:
        n = min(FIXED, mi)
        lam_f, dz_f = run_fixed(n)
        lam_of, dz_of, _ = oracle_solve(s, dt, 0.0, n, lam0)
        lam_tf, dz_tf, _ = oracle_solve(s, dt, 0.0, n, lam0, rounded=True)
        check_f32(f"warm start, lambda after {n} iterations {tag}", lam_f, lam_of, lam_tf)
        check_f32(f"warm start, dz after {n} iterations {tag}", dz_f, dz_of, dz_tf)
    lam_t, dz_t, _ = oracle_solve(s, dt, 1e-14, 2000, lam0, rounded=True)        # converged: what the stopped runs approach
    check_f32(f"warm start, lambda {tag}", lam, lam_o, lam_t)
    check_f32(f"warm start, dz {tag}", dz, dz_o, dz_t)
    return it_o


# (S, C, K, dtype, options, expected (last_pair, groups > 1, last_mode)): every family the planner picks for a whole solve
WHOLE = [
    (2, 1, 5, np.float64, {}, (0, False, 1)),
    (2, 1, 5, np.float32, {}, (1, False, 1)),
    (32, 16, 7, np.float64, {}, (0, False, 1)),
    (14, 7, 50, np.float64, {}, (2, False, 1)),             # mixed-rows single workgroup (two rows per lane in part of the waves)
    (14, 7, 50, np.float32, {}, (1, False, 1)),             # private windows (two rows per lane)
    (14, 7, 49, np.float32, {}, (1, False, 1)),
    (14, 7, 10, np.float32, {}, (1, False, 1)),
    (14, 7, 512, np.float32, {}, (0, True, 1)),             # multi-workgroup persistent launch
    (14, 7, 300, np.float64, dict(pcg_mode=2), (0, False, 2)),   # streaming kernels
    (14, 7, 1, np.float64, {}, (0, False, 1)),
    (14, 7, 2, np.float64, {}, (0, False, 1)),
    (14, 7, 2, np.float32, {}, (1, False, 1)),
]


@pytest.mark.parametrize("S,C,K,dt,opts,family", WHOLE)
def test_warm_whole_solve(S, C, K, dt, opts, family):
    """Solver.linsys (gato_linsys_device) with true_warm_start: lambda and dz against oracle.linsys_solve(lam0=...)."""
    s = system(S, C, K, seed=K + 3)
    tol, mi = tol_mi(dt)
    sol = solver(S, C, K, dt, true_warm_start=1, **opts)
    dev = sol.upload_system(s)
    lam0 = guesses(s, 2, seed=K)[1].astype(dt)
    lam, dz = sol.new(S * K), sol.new(sol.N)

    def run(t, m, guess):
        lam.copy_(torch.from_numpy(np.ascontiguousarray(guess, dt)))
        sol.linsys(*dev, t, m, s.rho, lam, dz)
        sol.check_status()
        return host(lam).copy(), host(dz).copy()

    got_l, got_d = run(tol, mi, lam0)
    it = read_iters(sol)[0]
    pair, multi, mode = family
    assert (sol.get_option("last_pair"), sol.get_option("last_groups") > 1, sol.get_option("last_mode")) == (pair, multi, mode)
    tag = f"{S}/{C}/{K} {np.dtype(dt).name} {opts}"
    judge(tag, s, dt, tol, mi, lam0, got_l, got_d, it,
          run_fixed=(lambda n: run(0.0, n, lam0)) if K > 2 else None)     # (K <= 2 in fp32: 28 unknowns, exact within a few steps)
    # lambda0 = 0 with the option on: the cold solve's bits (r0 = gamma - S 0 = gamma exactly; the hand-offs move the same values)
    warm0 = run(tol, mi, np.zeros(S * K)) + (read_iters(sol)[0],)
    sol.set_option("true_warm_start", 0)
    cold = run(tol, mi, np.full(S * K, np.nan)) + (read_iters(sol)[0],)  # (the cold solve never reads lambda)
    assert warm0[2] == cold[2] and np.array_equal(warm0[0], cold[0]) and np.array_equal(warm0[1], cold[1]), tag
    sol.close()


@pytest.mark.parametrize("S,C,K,B,dt", [(14, 7, 50, 5, np.float64), (14, 7, 50, 7, np.float64), (14, 7, 50, 5, np.float32),
                                        (14, 7, 50, 7, np.float32), (2, 1, 5, 33, np.float64)])
def test_warm_batch_with_a_guess_per_system(S, C, K, B, dt):
    """linsys_batched: B different systems, each with its OWN lambda0 at lambda + b S K; system 1 starts from its converged
    solution, so the per-system iteration counts differ (a wrong system offset or a shared lambda0 cannot pass)."""
    systems = [synth.make_system(S, C, K, seed=40 + b) for b in range(B)]
    tol, mi = tol_mi(dt)
    sol = solver(S, C, K, dt, batch=B, true_warm_start=1)
    dev = sol.upload_batch(systems)
    lam0s = [guesses(x, 2, seed=b)[1] for b, x in enumerate(systems)]
    lam0s[1] = guesses(systems[1], 1, seed=0)[0]
    lam0 = np.concatenate(lam0s).astype(dt)
    lam, dz, it = sol.new(B * S * K), sol.new(B * sol.N), sol.new(B, torch.int32)

    def run(t, m, guess):
        lam.copy_(torch.from_numpy(np.ascontiguousarray(guess, dt)))
        sol.linsys_batched(*dev, t, m, systems[0].rho, lam, dz, it)
        sol.check_status()
        return host(lam).copy(), host(dz).copy(), host(it).copy()

    L, Z, I = run(tol, mi, lam0)
    assert sol.get_option("last_groups") == 1
    sk, N = S * K, sol.N
    its_o = []
    for b, x in enumerate(systems):
        tag = f"batch {S}/{C}/{K} x{B} system {b} {np.dtype(dt).name}"
        its_o.append(judge(tag, x, dt, tol, mi, lam0[b * sk:(b + 1) * sk], L[b * sk:(b + 1) * sk], Z[b * N:(b + 1) * N], int(I[b])))
    assert I[1] <= 1 and max(I) > 1 and its_o[1] <= 1, (list(I), its_o)
    if dt == np.float32:                # fixed count: every system after FIXED iterations from its own guess
        Lf, Zf, _ = run(0.0, FIXED, lam0)
        for b, x in enumerate(systems):
            if b == 1:
                continue                # (from the solution: the fixed iterations run on rounding noise)
            g = lam0[b * sk:(b + 1) * sk]
            lo, zo, _ = oracle_solve(x, dt, 0.0, FIXED, g)
            lt, zt, _ = oracle_solve(x, dt, 0.0, FIXED, g, rounded=True)
            check_f32(f"warm batch, lambda after {FIXED} iterations system {b} x{B}", Lf[b * sk:(b + 1) * sk], lo, lt)
            check_f32(f"warm batch, dz after {FIXED} iterations system {b} x{B}", Zf[b * N:(b + 1) * N], zo, zt)
    W0 = run(tol, mi, np.zeros(B * sk))
    sol.set_option("true_warm_start", 0)
    C0 = run(tol, mi, np.full(B * sk, np.nan))
    assert all(np.array_equal(a, b) for a, b in zip(W0, C0))
    sol.close()


def new_rhs(s, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(s.g.shape) * max(np.abs(s.g).max(), 1.0)
    c = rng.standard_normal(s.c.shape) * max(np.abs(s.c).max(), 1.0)
    return synth.KKTSystem(s.S, s.C, s.K, s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val,
                           g.astype(s.g.dtype), c.astype(s.c.dtype), s.rho)


@pytest.mark.parametrize("S,C,K,dt", [(14, 7, 50, np.float64), (14, 7, 512, np.float32)])
@pytest.mark.parametrize("B", [1, 4])
def test_warm_resolve_with_a_guess_per_rhs(S, C, K, dt, B):
    """Solver.solve_rhs (gato_solve_rhs) with R = 3 right-hand sides per system, each with its own lambda0 at lambda + (b R + i) S K
    (the index is a right-hand side, not a matrix); the first of every system starts from its converged solution."""
    if B > 1 and K > 100:
        K = 50                          # (a batch needs one workgroup per system)
    R = 3
    base = [synth.make_system(S, C, K, seed=60 + b) for b in range(B)]
    tol, mi = tol_mi(dt)
    sol = solver(S, C, K, dt, batch=B, true_warm_start=1)
    lam_a, dz_a = sol.new(B * S * K), sol.new(B * sol.N)
    lam_a.zero_()                       # (the assembling solve is warm-started too)
    if B > 1:
        sol.linsys_batched(*sol.upload_batch(base), tol, mi, base[0].rho, lam_a, dz_a)
    else:
        sol.linsys(*sol.upload_system(base[0]), tol, mi, base[0].rho, lam_a, dz_a)
    sol.check_status()
    sol.reserve_rhs(R)
    rhs = [[new_rhs(x, 100 * b + i) for i in range(R)] for b, x in enumerate(base)]
    flat = [r for per in rhs for r in per]
    g = sol.to_device(np.concatenate([r.g for r in flat]))
    c = sol.to_device(np.concatenate([r.c for r in flat]))
    lam0s = []
    for j, r in enumerate(flat):
        gs = guesses(r, 2, seed=j)
        lam0s.append(gs[0] if j % R == 0 else gs[1])
    lam0 = np.concatenate(lam0s).astype(dt)
    sk, N = S * K, sol.N

    def run(t, m, guess):
        lam = sol.to_device(np.ascontiguousarray(guess, dt))
        lam, dz, it = sol.solve_rhs(g, c, t, m, lam=lam)
        sol.check_status()
        return host(lam).copy(), host(dz).copy(), host(it).copy()

    L, Z, I = run(tol, mi, lam0)
    if K > 100:
        assert sol.get_option("last_groups") > 1
    for j, r in enumerate(flat):
        judge(f"re-solve {S}/{C}/{K} B={B} rhs {j} {np.dtype(dt).name}", r, dt, tol, mi, lam0[j * sk:(j + 1) * sk],
              L[j * sk:(j + 1) * sk], Z[j * N:(j + 1) * N], int(I[j]))
    assert all(I[j] <= 1 for j in range(0, B * R, R)) and max(I) > 1, list(I)
    if dt == np.float32:
        Lf, Zf, _ = run(0.0, FIXED, lam0)
        for j, r in enumerate(flat):
            if j % R == 0:
                continue
            gj = lam0[j * sk:(j + 1) * sk]
            lo, zo, _ = oracle_solve(r, dt, 0.0, FIXED, gj)
            lt, zt, _ = oracle_solve(r, dt, 0.0, FIXED, gj, rounded=True)
            check_f32(f"warm re-solve, lambda after {FIXED} iterations rhs {j} B={B}", Lf[j * sk:(j + 1) * sk], lo, lt)
            check_f32(f"warm re-solve, dz after {FIXED} iterations rhs {j} B={B}", Zf[j * N:(j + 1) * N], zo, zt)
    W0 = run(tol, mi, np.zeros(B * R * sk))
    sol.set_option("true_warm_start", 0)
    C0 = run(tol, mi, np.full(B * R * sk, np.nan))
    assert all(np.array_equal(a, b) for a, b in zip(W0, C0))
    sol.close()


def test_dropin_ignores_a_stray_warm_start():
    """D5: the drop-in gpu_library.linsys_solve resets lambda as the reference does - input_lambda full of NaN with warm_start = 1
    returns the cold result bit for bit."""
    import gpu_library
    s = synth.make_system(14, 7, 50, seed=0)
    gpu_library.set_problem_size(14, 7, 50)
    try:
        args = (s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, s.g, s.c)
        l0, dz0 = gpu_library.linsys_solve(*args, np.zeros(700), 2, 1e-6, 100, False, s.rho)
        it0 = gpu_library.last_stats()["iters"]
        l1, dz1 = gpu_library.linsys_solve(*args, [float("nan")] * 700, 2, 1e-6, 100, True, s.rho)
        it1 = gpu_library.last_stats()["iters"]
    finally:
        gpu_library.clear_problem_size()
    assert it0 == it1 and np.array_equal(np.asarray(l0), np.asarray(l1)) and np.array_equal(np.asarray(dz0), np.asarray(dz1))
    assert np.isfinite(np.asarray(l1)).all()
