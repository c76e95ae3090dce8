"""Device time of KKT solves with a state-control cross term beside the same solves with M dropped:
Solver.linsys_blocks_cross against linsys_blocks, solve_rhs_cross against solve_rhs, and the backward stages of kkt_solve with M
(the adjoint through solve_rhs_cross, kkt_grad_blocks, kkt_grad_cross) against those without - on one build in one process, each
pair in alternation over --rounds rounds; median, smallest and largest of the rounds.  Fixed iteration counts (exit_tol = 0) so
that both sides of a pair run the same PCG work.  One JSON line per case.
    python tools/cross_bench.py [--iters 30] [--reps 20] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import autograd, synth            # noqa: E402
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
    per = [synth.make_blocks(S, C, K, seed=300 + b) for b in range(B)]
    Ms = [synth.make_cross(p[0], p[1], seed=700 + b) for b, p in enumerate(per)]
    dev = lambda a: torch.tensor(a, dtype=tdt, device="cuda:0")
    blocks = [dev(np.stack([p[i] for p in per])) for i in range(7)]
    Gb, Cb, g, c = autograd._pack(*blocks)
    Mb = dev(np.stack(Ms)).transpose(-1, -2).reshape(B, -1).contiguous()
    # two solvers, so that each side re-solves its own assembly in the alternation
    plain, cross = Solver(S, C, K, dt, batch=B), Solver(S, C, K, dt, batch=B)
    N, sk = plain.N, S * K
    lam, dz = plain.new(B * sk), plain.new(B * N)
    rng = np.random.default_rng(0)
    w1, w2 = dev(rng.standard_normal((B, N))), dev(rng.standard_normal((B, sk)))
    Gbar, Cbar, Mbar = torch.empty_like(Gb), torch.empty_like(Cb), torch.empty_like(Mb)
    for s in (plain, cross):
        s.reserve_rhs(1)
    plain.linsys_blocks(Gb, Cb, g, c, 0.0, it, 1e-3, lam, dz)
    cross.linsys_blocks_cross(Gb, Mb, Cb, g, c, 0.0, it, 1e-3, lam, dz)
    lam_d, dz_d = lam.view(B, sk), dz.view(B, N)

    def backward(sol, is_cross):
        a, beta = autograd._adjoint(sol, lam_d, dz_d, w2, w1, 0.0, it, cross=is_cross)
        sol.kkt_grad_blocks(dz_d, lam_d, a, beta, Gbar, Cbar)
        if is_cross:
            sol.kkt_grad_cross(dz_d, a, Mbar)

    fns = dict(linsys_blocks=lambda: plain.linsys_blocks(Gb, Cb, g, c, 0.0, it, 1e-3, lam, dz),
               linsys_blocks_cross=lambda: cross.linsys_blocks_cross(Gb, Mb, Cb, g, c, 0.0, it, 1e-3, lam, dz),
               solve_rhs=lambda: plain.solve_rhs(w1, w2, 0.0, it),
               solve_rhs_cross=lambda: cross.solve_rhs_cross(w1, w2, 0.0, it),
               backward_stages=lambda: backward(plain, False),
               backward_stages_cross=lambda: backward(cross, True))
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps))
    out = dict(S=S, C=C, K=K, B=B, dtype=np.dtype(dt).name, pcg_iters=it, reps=reps, rounds=rounds,
               **{k + "_ms": spread(v) for k, v in ms.items()})
    for a, b in (("linsys_blocks_cross", "linsys_blocks"), ("solve_rhs_cross", "solve_rhs"), ("backward_stages_cross", "backward_stages")):
        out[a + "_extra_us"] = 1e3 * (out[a + "_ms"]["median"] - out[b + "_ms"]["median"])
    plain.close()
    cross.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        lines.append(json.dumps(case(S, C, K, B, dt, a.iters, a.reps, a.rounds)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
