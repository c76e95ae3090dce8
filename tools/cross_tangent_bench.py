"""Device time of forward-mode sensitivities with a cross term (Solver.tangents_cross) beside the call
without M (Solver.tangents), and of cross_tangent_rhs_kernel - staged through LDS and reading the tangent blocks in place (option
cross_tangent_form) - beside kkt_tangent_rhs_kernel on the same G., C., g., c. with M. NULL: the systems of
tools/kkt_tangent_bench.py, R = 1 and R = 8, dense random tangents, fixed iteration counts (exit_tol = 0), on the same build in
the same process, everything in alternation over --rounds rounds; median, smallest and largest of the rounds.  The kernel rows of
one system are launch-bound between events: their device times are those of a rocprofv3 --kernel-trace --stats run of this tool.
One JSON line per case.
    python tools/cross_tangent_bench.py [--iters 30] [--reps 20] [--rounds 7] [--directions 1,8] [--batches 8,32,128] [--out FILE]"""
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


def case(S, C, K, B, dt, it, reps, rounds, Rs=(1, 8)):
    tdt = torch.float64 if dt == np.float64 else torch.float32
    per = [synth.make_blocks(S, C, K, seed=300 + b) for b in range(B)]
    Ms = [synth.make_cross(p[0], p[1], seed=1300 + b) for b, p in enumerate(per)]
    dev = lambda a: torch.tensor(a, dtype=tdt, device="cuda:0")
    Gb, Cb, g, c = autograd._pack(*[dev(np.stack([p[i] for p in per])) for i in range(7)])
    Mb = dev(np.stack(Ms)).transpose(-1, -2).reshape(B, -1).contiguous()
    rng = np.random.default_rng(0)
    N, sk = (S + C) * K - C, S * K
    rand = lambda n: torch.tensor(rng.standard_normal(n), dtype=tdt, device="cuda:0")
    sols = {name: Solver(S, C, K, dt, batch=B) for name in ("plain", "cross", "staged", "in_place")}
    sols["staged"].set_option("cross_tangent_form", 1)       # the kernel rows force a form; tangents_cross runs the entry's own choice
    sols["in_place"].set_option("cross_tangent_form", 2)
    lam, dz = {}, {}
    for name, sol in sols.items():
        lam[name], dz[name] = sol.new(B * sk), sol.new(B * N)
        if name == "plain":
            sol.linsys_blocks(Gb, Cb, g, c, 0.0, it, 1e-3, lam[name], dz[name])
        else:
            sol.linsys_blocks_cross(Gb, Mb, Cb, g, c, 0.0, it, 1e-3, lam[name], dz[name])
    dots = {R: dict(G_dot=rand(B * R * Gb.shape[1]), C_dot=rand(B * R * Cb.shape[1]), g_dot=rand(B * R * N), c_dot=rand(B * R * sk))
            for R in Rs}
    Md = {R: rand(B * R * Mb.shape[1]) for R in Rs}
    outs = {R: dict(tg=rand(B * R * N), gp=rand(B * R * N), tc=rand(B * R * sk)) for R in Rs}
    fns = {}
    for R in Rs:
        o = outs[R]
        fns.update({
            f"tangents_plain_r{R}": lambda R=R: sols["plain"].tangents(R, dz["plain"], lam["plain"], 0.0, it, **dots[R]),
            f"tangents_cross_r{R}": lambda R=R: sols["cross"].tangents_cross(R, dz["cross"], lam["cross"], 0.0, it, M_dot=Md[R], **dots[R]),
            f"kernel_plain_r{R}": lambda R=R, o=o: sols["plain"].kkt_tangent_rhs(R, dz["plain"], lam["plain"], tg=o["tg"], tc=o["tc"], **dots[R]),
            f"kernel_cross_staged_r{R}": lambda R=R, o=o: sols["staged"].kkt_tangent_rhs_cross(R, dz["staged"], lam["staged"], gp=o["gp"], tc=o["tc"], **dots[R]),
            f"kernel_cross_in_place_r{R}": lambda R=R, o=o: sols["in_place"].kkt_tangent_rhs_cross(R, dz["in_place"], lam["in_place"], gp=o["gp"], tc=o["tc"], **dots[R]),
            f"kernel_cross_staged_with_M_dot_r{R}": lambda R=R, o=o: sols["staged"].kkt_tangent_rhs_cross(R, dz["staged"], lam["staged"], gp=o["gp"], tc=o["tc"], M_dot=Md[R], **dots[R]),
            f"kernel_cross_in_place_with_M_dot_r{R}": lambda R=R, o=o: sols["in_place"].kkt_tangent_rhs_cross(R, dz["in_place"], lam["in_place"], gp=o["gp"], tc=o["tc"], M_dot=Md[R], **dots[R]),
            f"cross_finish_r{R}": lambda R=R, o=o: sols["cross"].cross_finish(o["tg"]),
        })
    for fn in fns.values():                                  # warm-up: the re-solve work areas grow to R = 8 here
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    Rl = Rs[-1]
    a = sols["staged"].kkt_tangent_rhs_cross(Rl, dz["cross"], lam["cross"], M_dot=Md[Rl], **dots[Rl])
    b = sols["in_place"].kkt_tangent_rhs_cross(Rl, dz["cross"], lam["cross"], M_dot=Md[Rl], **dots[Rl])
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps))
    out = dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", pcg_iters=it, rounds=rounds, reps=reps, staged_equals_in_place=same)
    out.update({k + "_ms": spread(v) for k, v in ms.items()})
    med = lambda k: out[k + "_ms"]["median"]
    for R in Rs:
        out[f"cross_extra_us_r{R}"] = 1e3 * (med(f"tangents_cross_r{R}") - med(f"tangents_plain_r{R}"))
        out[f"staged_over_in_place_r{R}"] = med(f"kernel_cross_staged_r{R}") / med(f"kernel_cross_in_place_r{R}")
        out[f"staged_over_plain_kernel_r{R}"] = med(f"kernel_cross_staged_r{R}") / med(f"kernel_plain_r{R}")
    for sol in sols.values():
        sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--directions", default="1,8", help="comma-separated R (a profile run separates them by running one)")
    ap.add_argument("--batches", help="comma-separated batch sizes of 14/7/50 fp64 instead of the three cases")
    ap.add_argument("--out")
    a = ap.parse_args()
    Rs = tuple(int(v) for v in a.directions.split(","))
    if a.batches:                                            # where staging starts to pay: 14/7/50 fp64 over the batch size
        rows = [case(14, 7, 50, int(B), np.float64, a.iters, a.reps, a.rounds, Rs) for B in a.batches.split(",")]
    else:
        rows = [case(14, 7, 50, 1, np.float64, a.iters, a.reps, a.rounds, Rs), case(14, 7, 50, 512, np.float64, a.iters, a.reps, a.rounds, Rs),
                case(14, 7, 512, 1, np.float32, a.iters, a.reps, a.rounds, Rs)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
