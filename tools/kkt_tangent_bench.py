"""Device time of forward-mode sensitivities (Solver.tangents) beside the backward pass of the same call:
one tangent (R = 1) and R = 8 tangents in one call against the stages of kkt_solve's backward (the adjoint re-solve plus the
gradient kernel), on the same build in the same run, the three in alternation over --rounds rounds; median, smallest and largest
of the rounds.  Also the tangent's own stages (the right-hand-side kernel, the re-solve) and L.backward() through torch.  Fixed
iteration counts (exit_tol = 0) so that every re-solve runs the same PCG work per right-hand side.  One JSON line per case.
    python tools/kkt_tangent_bench.py [--iters 30] [--reps 20] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import autograd, synth            # noqa: E402


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
    blocks = [torch.tensor(np.stack([p[i] for p in per]), dtype=tdt, device="cuda:0", requires_grad=True) for i in range(7)]
    kw = dict(rho=1e-3, exit_tol=0.0, max_iters=it)
    rng = np.random.default_rng(0)
    N = (S + C) * K - C
    rand = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=tdt, device="cuda:0")
    w1, w2 = rand(B, N), rand(B, S * K)
    lam, dz = autograd.kkt_solve(*blocks, **kw)
    L = (dz * w1).sum() + (lam * w2).sum()
    sol = autograd._SOLVERS[(S, C, K, B, tdt, 0)]
    lam_d, dz_d = lam.detach(), dz.detach()
    Gb, Cb, _, _ = autograd._pack(*[b.detach() for b in blocks])
    Gbar, Cbar = torch.empty_like(Gb), torch.empty_like(Cb)
    dots = {R: dict(G_dot=rand(B * R * Gb.shape[1]), C_dot=rand(B * R * Cb.shape[1]), g_dot=rand(B * R * N), c_dot=rand(B * R * S * K))
            for R in (1, 8)}

    def backward_stages():
        a, beta = autograd._adjoint(sol, lam_d, dz_d, w2, w1, 0.0, it)
        sol.kkt_grad_blocks(dz_d, lam_d, a, beta, Gbar, Cbar)

    fns = dict(tangent_r1=lambda: sol.tangents(1, dz_d, lam_d, 0.0, it, **dots[1]),
               tangent_r8=lambda: sol.tangents(8, dz_d, lam_d, 0.0, it, **dots[8]),
               backward_stages=backward_stages,
               backward_torch=lambda: L.backward(retain_graph=True),
               rhs_kernel_r1=lambda: sol.kkt_tangent_rhs(1, dz_d, lam_d, **dots[1]),
               rhs_kernel_r8=lambda: sol.kkt_tangent_rhs(8, dz_d, lam_d, **dots[8]),
               resolve_r1=lambda: sol.solve_rhs(dots[1]["g_dot"], dots[1]["c_dot"], 0.0, it),
               resolve_r8=lambda: sol.solve_rhs(dots[8]["g_dot"], dots[8]["c_dot"], 0.0, it))
    for fn in fns.values():                                  # warm-up: the re-solve work area grows to R = 8 here
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps))
    out = dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", pcg_iters=it, rounds=rounds, reps=reps)
    out.update({k + "_ms": spread(v) for k, v in ms.items()})
    med = lambda k: out[k + "_ms"]["median"]
    out["tangent_r1_over_backward_stages"] = med("tangent_r1") / med("backward_stages")
    out["tangent_r8_over_8_tangent_r1"] = med("tangent_r8") / (8 * med("tangent_r1"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = [case(14, 7, 50, 1, np.float64, a.iters, a.reps, a.rounds), case(14, 7, 50, 512, np.float64, a.iters, a.reps, a.rounds),
            case(14, 7, 512, 1, np.float32, a.iters, a.reps, a.rounds)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
