"""Device time of the CSR entry to the cross solve beside two yardsticks that are not the code under
test: Solver.linsys_blocks_cross on pre-scattered blocks (the floor: no gather at all) and plain Solver.linsys / linsys_batched
on the CSR without M (what CSR input costs today).  Also the stage alone - cross_prepare_csr with 256 and with 64 threads per
workgroup - beside its two-launch alternative, convert (the gather of the plain path) followed by cross_prepare, and beside
cross_prepare alone.  One build, one process, every group in alternation over --rounds rounds; median, smallest and largest of
the rounds.  Fixed iteration counts (exit_tol = 0) so that every solve runs the same PCG work.  One JSON line per case.
--threads-sweep measures instead where the library's switch between the two workgroup sizes (CROSS_CSR_WAVE_KNOTS knots per
compute unit, gato_solver.h) belongs: the stage alone with 256 and with 64 threads, in alternation, over batch sizes at one shape.
    python tools/cross_csr_bench.py [--iters 30] [--reps 20] [--rounds 7] [--only CASE] [--out FILE]
    python tools/cross_csr_bench.py --threads-sweep [--shape 14,7,50] [--batches 4,8,...] [--reps 20] [--rounds 7] [--out FILE]"""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import _lib, autograd, synth      # noqa: E402
from gato_python_amd.solver import Solver              # noqa: E402


def timed(fn, reps):
    """median device time (ms) of fn() between two events"""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def case(S, C, K, B, dt, it, reps, rounds):
    tdt = torch.float64 if dt == np.float64 else torch.float32
    per = [synth.make_blocks(S, C, K, seed=300 + b, dense_q=True) for b in range(B)]
    Ms = [synth.make_cross(p[0], p[1], seed=700 + b) for b, p in enumerate(per)]
    dev = lambda a: torch.tensor(a, dtype=tdt, device="cuda:0")
    idev = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda:0")
    blocks = [dev(np.stack([p[i] for p in per])) for i in range(7)]
    Gb, Cb, g, c = autograd._pack(*blocks)
    Mb = dev(np.stack(Ms)).transpose(-1, -2).reshape(B, -1).contiguous()
    # the batch shares the pattern of its first system (dense Q, dense M: every system has the same structure)
    with_M = [synth.blocks_to_csr(*p, dense_q=True, M=m) for p, m in zip(per, Ms)]
    no_M = [synth.blocks_to_csr(*p, dense_q=True) for p in per]
    assert all(np.array_equal(s.G_col, with_M[0].G_col) for s in with_M) and all(np.array_equal(s.G_col, no_M[0].G_col) for s in no_M)
    csr = lambda ss: (idev(ss[0].G_row), idev(ss[0].G_col), dev(np.stack([s.G_val for s in ss])).reshape(-1), idev(ss[0].C_row),
                      idev(ss[0].C_col), dev(np.stack([s.C_val for s in ss])).reshape(-1))
    cm, c0 = csr(with_M), csr(no_M)
    gf, cf = g.reshape(-1), c.reshape(-1)
    # a solver per path, so that no side pays for the other's work area or plan
    names = ("csr_cross", "blocks_cross", "csr_plain", "stage")
    sol = {k: Solver(S, C, K, dt, batch=B) for k in names}
    N, sk = sol["stage"].N, S * K
    lam, dz = sol["stage"].new(B * sk), sol["stage"].new(B * N)
    st = sol["stage"]
    plain = (lambda: sol["csr_plain"].linsys(*c0, gf, cf, 0.0, it, 1e-3, lam, dz)) if B == 1 else \
            (lambda: sol["csr_plain"].linsys_batched(*c0, gf, cf, 0.0, it, 1e-3, lam, dz))
    if B > 1:
        st.set_option("batch_nnz_G", cm[1].numel())
        st.set_option("batch_nnz_C", cm[4].numel())

    def stage(threads):
        def fn():
            st.set_option("cross_csr_threads", threads)
            st.cross_prepare_csr(*cm, gf, 1e-3)
        return fn

    # gato_convert writes the blocks of all B systems: outputs of that size (Solver.convert allocates one system's)
    Gd, Cd = st.new(B * st.sizes["G_dense"]), st.new(B * st.sizes["C_dense"])
    assert Gd.numel() == Gb.numel() and Cd.numel() == Cb.numel()

    def two_launches():
        _lib.check(_lib.lib().gato_convert(st._h, *(ct.c_void_p(t.data_ptr()) for t in cm), 0.0, ct.c_void_p(Gd.data_ptr()),
                                           ct.c_void_p(Cd.data_ptr()), st._stream()))
        st.cross_prepare(Gd, Mb, Cd, gf, 1e-3)

    fns = dict(linsys_cross=lambda: sol["csr_cross"].linsys_cross(*cm, gf, cf, 0.0, it, 1e-3, lam, dz),
               linsys_blocks_cross=lambda: sol["blocks_cross"].linsys_blocks_cross(Gb, Mb, Cb, gf, cf, 0.0, it, 1e-3, lam, dz),
               linsys_plain_csr=plain,
               prepare_csr=stage(0), prepare_csr_256=stage(256), prepare_csr_64=stage(64),      # 0: the library's choice
               convert_then_prepare=two_launches,
               prepare_blocks=lambda: st.cross_prepare(Gb, Mb, Cb, gf, 1e-3))
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps))
    out = dict(S=S, C=C, K=K, B=B, dtype=np.dtype(dt).name, pcg_iters=it, reps=reps, rounds=rounds, nnz_G=int(cm[1].numel()),
               nnz_C=int(cm[4].numel()), knots_per_cu=knots_per_cu(K, B), **{k + "_ms": spread(v) for k, v in ms.items()})
    med = lambda k: out[k + "_ms"]["median"]
    out["linsys_cross_over_blocks_us"] = 1e3 * (med("linsys_cross") - med("linsys_blocks_cross"))
    out["linsys_cross_over_plain_csr_us"] = 1e3 * (med("linsys_cross") - med("linsys_plain_csr"))
    out["fused_over_two_launches_us"] = 1e3 * (med("prepare_csr") - med("convert_then_prepare"))      # as the library launches it
    for s in sol.values():
        s.close()
    return out


def knots_per_cu(K, B):
    """the quantity the library's choice of the workgroup size goes by: workgroups of the stage per compute unit"""
    return B * min(K, 8192) / torch.cuda.get_device_properties(0).multi_processor_count


def threads_sweep(S, C, K, batches, dt, reps, rounds):
    """The stage alone with 256 and with 64 threads per workgroup over batch sizes, the two in alternation over the rounds.  The
    batch repeats eight different systems (the time does not depend on the values); dense Q and M as in case()."""
    tdt = torch.float64 if dt == np.float64 else torch.float32
    per = [synth.make_blocks(S, C, K, seed=300 + b, dense_q=True) for b in range(8)]
    ss = [synth.blocks_to_csr(*p, dense_q=True, M=synth.make_cross(p[0], p[1], seed=700 + b)) for b, p in enumerate(per)]
    assert all(np.array_equal(s.G_col, ss[0].G_col) for s in ss)
    idx = [torch.tensor(a, dtype=torch.int32, device="cuda:0") for a in (ss[0].G_row, ss[0].G_col, ss[0].C_row, ss[0].C_col)]
    tile = lambda f, B: torch.tensor(np.stack([f(ss[b % 8]) for b in range(B)]), dtype=tdt, device="cuda:0").reshape(-1)
    for B in batches:
        sol = Solver(S, C, K, dt, batch=B)
        if B > 1:
            sol.set_option("batch_nnz_G", idx[1].numel())
            sol.set_option("batch_nnz_C", idx[3].numel())
        Gv, Cv, g = tile(lambda s: s.G_val, B), tile(lambda s: s.C_val, B), tile(lambda s: s.g, B)

        def stage(threads):
            sol.set_option("cross_csr_threads", threads)
            sol.cross_prepare_csr(idx[0], idx[1], Gv, idx[2], idx[3], Cv, g, 1e-3)

        us = {256: [], 64: []}
        for t in us:
            stage(t)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for t in us:
                us[t].append(1e3 * timed(lambda: stage(t), reps))
        sol.close()
        yield dict(S=S, C=C, K=K, B=B, dtype=np.dtype(dt).name, reps=reps, rounds=rounds, knots_per_cu=knots_per_cu(K, B),
                   t256_us=spread(us[256]), t64_us=spread(us[64]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", type=int, default=None, help="run case 0, 1 or 2 alone")
    ap.add_argument("--threads-sweep", action="store_true", help="64 against 256 threads per workgroup over batch sizes")
    ap.add_argument("--shape", default="14,7,50", help="S,C,K of --threads-sweep")
    ap.add_argument("--batches", default="4,8,16,32,64,128,256", help="batch sizes of --threads-sweep")
    a = ap.parse_args()
    lines = []
    if a.threads_sweep:
        S, C, K = (int(v) for v in a.shape.split(","))
        for dt in (np.float64, np.float32):
            for line in threads_sweep(S, C, K, [int(v) for v in a.batches.split(",")], dt, a.reps, a.rounds):
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    else:
        cases = ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32))
        for S, C, K, B, dt in cases if a.only is None else cases[a.only:a.only + 1]:
            lines.append(json.dumps(case(S, C, K, B, dt, a.iters, a.reps, a.rounds)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
