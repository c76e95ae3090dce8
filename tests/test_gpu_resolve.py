"""Re-solve of an assembled system for new right-hand sides (gato_solve_rhs, Solver.solve_rhs, linsys_resolve).

The reference for every re-solve is the oracle's WHOLE solve of the system with the same G / C and the new (g, c)."""
import ctypes as ct
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gato_python_amd import _lib, synth           # noqa: E402
from oracle import c_oracle as co                 # noqa: E402
from oracle import gato_oracle as o               # noqa: E402
from test_gpu_parity import check_solve, host, rel   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def new_rhs(s, seed):
    """The system s with the same G / C and a fresh (g, c)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(s.g.shape) * max(np.abs(s.g).max(), 1.0)
    c = rng.standard_normal(s.c.shape) * max(np.abs(s.c).max(), 1.0)
    return synth.KKTSystem(s.S, s.C, s.K, s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val,
                           g.astype(s.g.dtype), c.astype(s.c.dtype), s.rho)


def solver(S, C, K, dt, batch=1, **opts):
    from gato_python_amd.solver import Solver
    sol = Solver(S, C, K, dt, batch=batch)
    for k, v in opts.items():
        sol.set_option(k, v)
    return sol


def tol_mi(dt):
    return (1e-10, 300) if dt == np.float64 else (1e-5, 100)


def assembled(S, C, K, dt, seed=0, **opts):
    s = synth.make_system(S, C, K, seed=seed)
    sol = solver(S, C, K, dt, **opts)
    dev = sol.upload_system(s)
    tol, mi = tol_mi(dt)
    lam, dz = sol.new(S * K), sol.new(sol.N)
    sol.linsys(*dev, tol, mi, s.rho, lam, dz)
    torch.cuda.synchronize()
    sol.check_status()
    return s, sol, dev, lam, dz


def rhs_dev(sol, systems):
    return (sol.to_device(np.concatenate([x.g for x in systems])), sol.to_device(np.concatenate([x.c for x in systems])))


CASES = [(2, 1, 5, np.float64, {}), (2, 1, 5, np.float32, {}), (14, 7, 1, np.float64, {}), (14, 7, 2, np.float64, {}),
         (14, 7, 50, np.float64, {}), (14, 7, 50, np.float32, {}), (32, 16, 7, np.float64, {}), (32, 16, 7, np.float32, {}),
         (14, 7, 512, np.float32, {}),                                          # multi-workgroup
         (14, 7, 50, np.float64, dict(pcg_mode=2))]                             # streaming kernels


@pytest.mark.parametrize("S,C,K,dt,opts", CASES)
def test_new_rhs_equals_a_full_solve(S, C, K, dt, opts):
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=5, **opts)
    # 14/7/2 at exit_tol 1e-10 is order-chaotic: the C and the numpy oracle differ by 4e-8 there; 8 fixed iterations agree to 1e-11
    tol, mi = (0.0, 8) if (S, C, K) == (14, 7, 2) else tol_mi(dt)
    s2 = new_rhs(s, 1)
    g2, c2 = rhs_dev(sol, [s2])

    def rerun(t, m):
        lam, dz, _ = sol.solve_rhs(g2, c2, t, m)
        torch.cuda.synchronize()
        return host(lam), host(dz)
    lam, dz, it = sol.solve_rhs(g2, c2, tol, mi)
    torch.cuda.synchronize()
    sol.check_status()
    check_solve(f"re-solve {S}/{C}/{K} {opts}", s2, S, C, K, dt, tol, mi, host(lam), host(dz), int(host(it)[0]), rerun=rerun)
    sol.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_new_rhs_under_each_preconditioner(mode):
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=6, precon_mode=mode)
    # block- / point-Jacobi take 100+ iterations here and their exit index moves by one with the summation order: compared at
    # a fixed count, as tests/test_gpu_parity.py::test_preconditioner_modes does
    tol, mi = tol_mi(dt) if mode == 0 else (0.0, 15)
    s2 = new_rhs(s, 2)
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, [s2]), tol, mi)
    torch.cuda.synchronize()
    ref = o.linsys_solve(*s2.csr_args(), S, C, K, tol, mi, s2.rho, dtype=np.float64, return_all=True, precon_mode=mode)
    assert int(host(it)[0]) == ref["iters"]
    assert rel(host(lam), ref["lam"]) < 1e-8 and rel(host(dz), ref["dz"]) < 1e-8
    sol.close()


def test_gamma_of_the_resolve():
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=7)
    s2 = new_rhs(s, 3)
    sol.solve_rhs(*rhs_dev(sol, [s2]), 1e-10, 300)
    ref = o.linsys_solve(*s2.csr_args(), S, C, K, 1e-10, 300, s2.rho, dtype=np.float64, return_all=True)
    assert rel(sol.read_rhs_gamma(1), ref["gamma"]) < 1e-12
    sol.close()


def test_same_rhs_as_the_assembly():
    """Not bit for bit: the re-solve sums gamma in another order than the Schur launch of the assembly."""
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, lam, dz = assembled(S, C, K, dt, seed=8)
    lam0, dz0 = host(lam).copy(), host(dz).copy()
    _, _, it_full = co.linsys_solve(*s.csr_args(), S, C, K, 1e-10, 300, s.rho, dtype=dt)
    lam1, dz1, it1 = sol.solve_rhs(dev[6], dev[7], 1e-10, 300)
    torch.cuda.synchronize()
    assert rel(host(lam1), lam0) < 1e-12 and rel(host(dz1), dz0) < 1e-12
    assert int(host(it1)[0]) == it_full
    sol.close()


@pytest.mark.parametrize("S,C,K,dt", [(14, 7, 50, np.float64), (14, 7, 50, np.float32), (14, 7, 512, np.float32)])
def test_r_at_once_equals_r_calls_bit_for_bit(S, C, K, dt):
    R = 7
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=9)
    tol, mi = tol_mi(dt)
    rs = [new_rhs(s, 20 + r) for r in range(R)]
    lam7, dz7, it7 = sol.solve_rhs(*rhs_dev(sol, rs), tol, mi)
    torch.cuda.synchronize()
    sol.check_status()
    lam7, dz7, it7 = host(lam7).reshape(R, -1), host(dz7).reshape(R, -1), host(it7)
    for r in range(R):
        lam, dz, it = sol.solve_rhs(*rhs_dev(sol, [rs[r]]), tol, mi)
        torch.cuda.synchronize()
        assert np.array_equal(host(lam), lam7[r]) and np.array_equal(host(dz), dz7[r]), r
        assert int(host(it)[0]) == int(it7[r])
    check_solve(f"R=7 rhs 3 {S}/{C}/{K}", rs[3], S, C, K, dt, tol, mi, lam7[3], dz7[3], int(it7[3]))
    sol.close()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_batch_of_systems_times_rhs(dt):
    S, C, K, B, R = 14, 7, 50, 4, 3
    systems = [synth.make_system(S, C, K, seed=100 + b) for b in range(B)]
    sol = solver(S, C, K, dt, batch=B)
    dev = sol.upload_batch(systems)
    tol, mi = tol_mi(dt)
    lam, dz, iters = sol.new(B * S * K), sol.new(B * sol.N), sol.new(B, torch.int32)
    sol.linsys_batched(*dev, tol, mi, systems[0].rho, lam, dz, iters)
    rs = [new_rhs(systems[b], 40 + 3 * b + r) for b in range(B) for r in range(R)]
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, rs), tol, mi)
    torch.cuda.synchronize()
    sol.check_status()
    lam, dz, it = host(lam).reshape(B * R, -1), host(dz).reshape(B * R, -1), host(it)
    for i, s2 in enumerate(rs):
        check_solve(f"batch {i // R} rhs {i % R}", s2, S, C, K, dt, tol, mi, lam[i], dz[i], int(it[i]))
    sol.close()


def test_matrices_untouched_and_a_new_assembly_is_used():
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=10)
    names = ("G_dense", "C_dense", "Ginv", "S", "Pinv")
    before = [sol.read_buffer(n).tobytes() for n in names]
    sol.solve_rhs(*rhs_dev(sol, [new_rhs(s, 4)]), 1e-10, 300)
    after = [sol.read_buffer(n).tobytes() for n in names]
    assert before == after
    s3 = synth.make_system(S, C, K, seed=11)                       # same pattern, other values
    lam, dz = sol.new(S * K), sol.new(sol.N)
    sol.linsys(*sol.upload_system(s3), 1e-10, 300, s3.rho, lam, dz)
    s4 = new_rhs(s3, 5)
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, [s4]), 1e-10, 300)
    torch.cuda.synchronize()
    check_solve("after a new assembly", s4, S, C, K, dt, 1e-10, 300, host(lam), host(dz), int(host(it)[0]))
    sol.close()


def test_true_warm_start():
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=12, true_warm_start=1)
    s2 = new_rhs(s, 6)
    ref = o.linsys_solve(*s2.csr_args(), S, C, K, 1e-10, 300, s2.rho, dtype=np.float64, return_all=True)
    lam0 = ref["lam"] * 0.9 + 0.01
    lam_o, it_o = o.pcg(ref["S"], ref["Pinv"], ref["gamma"], S, K, 1e-10, 300, lam0=lam0)
    lam = sol.to_device(lam0)
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, [s2]), 1e-10, 300, lam=lam)
    torch.cuda.synchronize()
    assert int(host(it)[0]) == it_o
    assert rel(host(lam), lam_o) < 1e-8
    sol.close()


def test_block_input_assembly():
    S, C, K, dt = 14, 7, 50, np.float64
    s = synth.make_system(S, C, K, seed=31)
    Gd0, Cd = co.convert(*s.csr_args()[:6], S, C, K, 0.0, dt)
    sol = solver(S, C, K, dt)
    Cb = sol.to_device(Cd)                                          # must stay unchanged until the next whole solve
    lam, dz = sol.new(S * K), sol.new(sol.N)
    sol.linsys_blocks(sol.to_device(Gd0), Cb, sol.to_device(s.g), sol.to_device(s.c), 1e-10, 300, s.rho, lam, dz)
    s2 = new_rhs(s, 7)
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, [s2]), 1e-10, 300)
    torch.cuda.synchronize()
    check_solve("re-solve after block input", s2, S, C, K, dt, 1e-10, 300, host(lam), host(dz), int(host(it)[0]))
    sol.close()


def _refused(fn, out):
    """fn must raise GatoError(EINVAL) and leave `out` (filled with a sentinel) untouched: nothing was enqueued."""
    out.fill_(7.0)
    torch.cuda.synchronize()
    with pytest.raises(_lib.GatoError) as e:
        fn()
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0


def test_refusals():
    L = _lib.lib()
    S, C, K, dt = 14, 7, 50, np.float64
    s = synth.make_system(S, C, K, seed=13)
    sol = solver(S, C, K, dt)
    g2, c2 = rhs_dev(sol, [new_rhs(s, 8)])
    lam = sol.new(S * K)
    _refused(lambda: sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam), lam)                       # no assembly yet
    dev = sol.upload_system(s)
    sol.linsys(*dev, 1e-10, 300, s.rho, sol.new(S * K), sol.new(sol.N))
    sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam)                                               # valid now
    torch.cuda.synchronize()
    # a stage entry writing into the solver's workspace
    _lib.check(L.gato_form_ss(sol._h, ct.c_void_p(sol.buffer_ptr(3)), ct.c_void_p(sol.buffer_ptr(4)), sol._stream()))
    assert sol.get_option("assembly_valid") == 0
    _refused(lambda: sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam), lam)
    sol.linsys(*dev, 1e-10, 300, s.rho, sol.new(S * K), sol.new(sol.N))
    # R = 0 (the C entry; the Python face infers R from the lengths) and wrong lengths
    dz, its = sol.new(sol.N), sol.new(1, torch.int32)

    def r0():
        _lib.check(L.gato_solve_rhs(sol._h, 0, ct.c_void_p(g2.data_ptr()), ct.c_void_p(c2.data_ptr()), 1e-10, 300,
                                    ct.c_void_p(lam.data_ptr()), ct.c_void_p(dz.data_ptr()), ct.c_void_p(its.data_ptr()),
                                    sol._stream()))
    _refused(r0, lam)
    with pytest.raises(ValueError):
        sol.solve_rhs(g2[:-1], c2, 1e-10, 300, lam=lam)
    with pytest.raises(ValueError):
        sol.solve_rhs(g2, c2[:-1], 1e-10, 300, lam=lam)
    # a cluster rank
    _lib.check(L.gato_cluster_create(sol._h, 0, 1, None))
    _refused(lambda: sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam), lam)
    _lib.check(L.gato_cluster_destroy(sol._h))
    sol.close()
    # a multi-workgroup re-solve under capture: refused, nothing enqueued, the capture itself still valid
    S, C, K, dt = 14, 7, 512, np.float32
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=14)
    assert sol.get_option("last_groups") > 1
    g2, c2 = rhs_dev(sol, [new_rhs(s, 9)])
    lam, dz, its = sol.new(S * K), sol.new(sol.N), sol.new(1, torch.int32)
    sol.reserve_rhs(1)
    st = torch.cuda.Stream()
    lam.fill_(7.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.GatoError):
            with torch.cuda.graph(gr, stream=st):
                sol.solve_rhs(g2, c2, 1e-5, 100, lam=lam, dz=dz, iters=its)
    torch.cuda.synchronize()
    assert float(lam.min()) == 7.0 and float(lam.max()) == 7.0
    # R beyond the reservation under capture (one-workgroup system)
    sol.close()
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=15)
    sol.reserve_rhs(1)
    rs = [new_rhs(s, 30 + r) for r in range(2)]
    g2, c2 = rhs_dev(sol, rs)
    lam = sol.new(2 * S * K).fill_(7.0)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(_lib.GatoError):
            with torch.cuda.graph(gr, stream=st):
                sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam)
    torch.cuda.synchronize()
    assert float(lam.min()) == 7.0
    sol.close()


def test_resolve_is_enqueue_only_and_replays_from_a_graph():
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=16)
    s2 = new_rhs(s, 10)
    g2, c2 = rhs_dev(sol, [s2])
    lam, dz, its = sol.new(S * K), sol.new(sol.N), sol.new(1, torch.int32)
    sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam, dz=dz, iters=its)
    torch.cuda.synchronize()
    ref = host(lam).copy()
    stream = torch.cuda.current_stream()
    t0 = time.perf_counter()
    torch.cuda._sleep(2_000_000)
    torch.cuda.synchronize()
    ticks = int(0.06 / ((time.perf_counter() - t0) / 2_000_000))
    lam.zero_()
    torch.cuda.synchronize()
    torch.cuda._sleep(ticks)
    t0 = time.perf_counter()
    sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam, dz=dz, iters=its)
    dt_call = time.perf_counter() - t0
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy and dt_call < 0.03, (busy, dt_call)
    assert np.array_equal(host(lam), ref)
    # captured once (single stream), replayed with new c values written in place
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            sol.solve_rhs(g2, c2, 1e-10, 300, lam=lam, dz=dz, iters=its)
        for rep in range(3):
            s3 = new_rhs(s, 50 + rep)
            s3 = synth.KKTSystem(S, C, K, s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, s2.g, s3.c, s.rho)
            c2.copy_(sol.to_device(s3.c))
            lam.fill_(float("nan")); dz.fill_(float("nan"))
            gr.replay()
            st.synchronize()
            check_solve(f"graph replay {rep}", s3, S, C, K, dt, 1e-10, 300, host(lam), host(dz), int(host(its)[0]))
    sol.close()


def test_headline_path_and_stage_times():
    S, C, K, dt = 14, 7, 50, np.float64
    s, sol, dev, _, _ = assembled(S, C, K, dt, seed=17)
    sol.set_option("time_stages", 1)
    lam, dz, it = sol.solve_rhs(*rhs_dev(sol, [new_rhs(s, 11)]), 1e-10, 300)
    torch.cuda.synchronize()
    assert sol.get_option("last_image") == 1 and sol.get_option("last_dz_fused") == 2
    ms = sol.last_stage_ms()
    assert ms["assembly"] > 0 and ms["pcg"] > 0
    sol.close()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_list_level_resolve(prec):
    import gato_python_amd as gp
    S, C, K = 14, 7, 50
    dt = np.float64 if prec == "f64" else np.float32
    s = synth.make_system(S, C, K, seed=18)
    s2 = new_rhs(s, 12)
    tol, mi = tol_mi(dt)
    old = os.environ.get("GATO_VERBOSE")
    os.environ["GATO_VERBOSE"] = "0"
    try:
        gp.set_precision(prec)
        gp.clear_problem_size()
        args = lambda x: [a.tolist() for a in x.csr_args()]
        gp.linsys_solve(*args(s), [0.0] * (S * K), 1, tol, mi, 0, s.rho)
        lam_r, dz_r = gp.linsys_resolve(s2.g.tolist(), s2.c.tolist(), tol, mi)
        it_r = gp.last_stats()["iters"]
        lam_f, dz_f = gp.linsys_solve(*args(s2), [0.0] * (S * K), 1, tol, mi, 0, s2.rho)
        it_f = gp.last_stats()["iters"]
    finally:
        gp.set_precision("f32")
        if old is None:
            os.environ.pop("GATO_VERBOSE", None)
        else:
            os.environ["GATO_VERBOSE"] = old
    if prec == "f64":
        assert it_r == it_f and rel(lam_r, lam_f) < 1e-8 and rel(dz_r, dz_f) < 1e-8
    else:
        check_solve("list-level re-solve f32", s2, S, C, K, dt, tol, mi, np.asarray(lam_r), np.asarray(dz_r), it_r)


def test_lti_mpc_example():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lti_mpc.py")], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("largest difference")][-1]
    assert float(last.split()[-1]) < 1e-8, last
