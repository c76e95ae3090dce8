"""Device time per call of the re-solve (Solver.solve_rhs) against the whole solve it replaces.  Fixed iteration counts
(exit_tol = 0) so that both sides run the same PCG work.  Prints one JSON line per case.
    python tools/resolve_bench.py [--iters 30] [--reps 50] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import synth                      # noqa: E402
from gato_python_amd.solver import Solver              # noqa: E402


def timed(fn, reps):
    """median device time (ms) of fn() between two events, after warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def rhs_of(s, seed, R):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.standard_normal(s.g.shape) for _ in range(R)]), np.concatenate([rng.standard_normal(s.c.shape) for _ in range(R)])


def one_system(S, C, K, dt, it, reps):
    s = synth.make_system(S, C, K, seed=0)
    sol = Solver(S, C, K, dt)
    dev = sol.upload_system(s)
    lam, dz = sol.new(S * K), sol.new(sol.N)
    full = timed(lambda: sol.linsys(*dev, 0.0, it, s.rho, lam, dz), reps)
    g, c = (sol.to_device(a) for a in rhs_of(s, 1, 1))
    out = sol.new(S * K), sol.new(sol.N), sol.new(1, torch.int32)
    re = timed(lambda: sol.solve_rhs(g, c, 0.0, it, *out), reps)
    r = dict(case=f"{S}/{C}/{K} {np.dtype(dt).name} R=1", full_ms=full, resolve_ms=re, ratio=re / full,
             last_image=sol.get_option("last_image"), last_dz_fused=sol.get_option("last_dz_fused"))
    sol.close()
    return r


def many_rhs(S, C, K, dt, R, it, reps):
    s = synth.make_system(S, C, K, seed=0)
    sol = Solver(S, C, K, dt)
    dev = sol.upload_system(s)
    sol.linsys(*dev, 0.0, it, s.rho, sol.new(S * K), sol.new(sol.N))
    sol.reserve_rhs(R)
    gR, cR = (sol.to_device(a) for a in rhs_of(s, 2, R))
    outR = sol.new(R * S * K), sol.new(R * sol.N), sol.new(R, torch.int32)
    at_once = timed(lambda: sol.solve_rhs(gR, cR, 0.0, it, *outR), reps)
    gs = [gR[r * sol.N:(r + 1) * sol.N] for r in range(R)]
    cs = [cR[r * S * K:(r + 1) * S * K] for r in range(R)]
    outs = [(outR[0][r * S * K:(r + 1) * S * K], outR[1][r * sol.N:(r + 1) * sol.N], outR[2][r:r + 1]) for r in range(R)]

    def singles():
        for r in range(R):
            sol.solve_rhs(gs[r], cs[r], 0.0, it, *outs[r])
    one_by_one = timed(singles, max(3, reps // 10))
    sol.close()
    return dict(case=f"{S}/{C}/{K} {np.dtype(dt).name} R={R} on one matrix", one_call_ms=at_once, r_calls_ms=one_by_one,
                speedup=one_by_one / at_once)


def batch(S, C, K, dt, B, it, reps):
    systems = [synth.make_system(S, C, K, seed=100 + b) for b in range(B)]
    sol = Solver(S, C, K, dt, batch=B)
    dev = sol.upload_batch(systems)
    lam, dz, its = sol.new(B * S * K), sol.new(B * sol.N), sol.new(B, torch.int32)
    full = timed(lambda: sol.linsys_batched(*dev, 0.0, it, systems[0].rho, lam, dz, its), reps)
    g, c = dev[6], dev[7]
    out = sol.new(B * S * K), sol.new(B * sol.N), sol.new(B, torch.int32)
    re = timed(lambda: sol.solve_rhs(g, c, 0.0, it, *out), reps)
    sol.close()
    return dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name} R=1", full_ms=full, resolve_ms=re, ratio=re / full)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = [one_system(14, 7, 50, np.float64, a.iters, a.reps), one_system(14, 7, 512, np.float32, a.iters, a.reps),
            many_rhs(14, 7, 50, np.float64, 64, a.iters, a.reps), batch(14, 7, 50, np.float64, 512, a.iters, a.reps)]
    for r in rows:
        r["pcg_iters"] = a.iters
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
