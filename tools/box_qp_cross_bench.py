"""Time of an ADMM iteration of a box QP with a state-control cross term beside the same iteration with M
dropped and beside its unfused composition, on one build in one process:
    box_qp                 Solver.box_qp on the system without M: a re-solve and qp_update_kernel per iteration;
    box_qp_cross           Solver.box_qp_cross: a re-solve and qp_update_cross_kernel per iteration;
    box_qp_cross_unfused   the same with option qp_cross_unfused = 1: cross_rhs, the re-solve, cross_finish and the update kernel
                           given a W of zeros - four launches per iteration, the same values.
Every call runs a fixed number of ADMM iterations (eps = 0) of a fixed number of PCG iterations (exit_tol = 0) and never reads the
live count, so a call is its launches and one synchronise; the time of an iteration is the difference of a long and a short call
over the difference of their iteration counts, which takes the prepare stages and the whole solve out.  The three in alternation
over --rounds rounds; median, smallest and largest of the rounds.  One JSON line per case.
    python tools/box_qp_cross_bench.py [--pcg 10] [--short 50] [--long 250] [--reps 5] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import _lib, autograd, synth      # noqa: E402
from gato_python_amd.solver import Solver              # noqa: E402


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def case(S, C, K, B, dt, pcg, short, long_, reps, rounds):
    tdt = torch.float64 if dt == np.float64 else torch.float32
    per = [synth.make_blocks(S, C, K, seed=300 + b) for b in range(B)]
    Ms = [synth.make_cross(p[0], p[1], seed=700 + b) for b, p in enumerate(per)]
    dev = lambda a: torch.tensor(a, dtype=tdt, device="cuda:0")
    blocks = [dev(np.stack([p[i] for p in per])) for i in range(7)]
    Gb, Cb, g, c = autograd._pack(*blocks)
    Mb = dev(np.stack(Ms)).transpose(-1, -2).reshape(B, -1).contiguous()
    inf = float("inf")
    xs, us = (lambda v: torch.full((B, K, S), v, dtype=tdt, device="cuda:0")), (lambda v: torch.full((B, K - 1, C), v, dtype=tdt, device="cuda:0"))
    lo, hi = autograd._dz_layout(xs(-inf), us(-0.2)), autograd._dz_layout(xs(inf), us(0.2))               # free states, |u| <= 0.2
    sols = dict(box_qp=Solver(S, C, K, dt, batch=B), box_qp_cross=Solver(S, C, K, dt, batch=B),
                box_qp_cross_unfused=Solver(S, C, K, dt, batch=B))
    sols["box_qp_cross_unfused"].set_option("qp_cross_unfused", 1)
    outs = {k: dict(x=s.new(B * s.N), z=s.new(B * s.N), y=s.new(B * s.N), lam=s.new(B * S * K)) for k, s in sols.items()}
    kw = dict(rho=1e-3, exit_tol=0.0, max_iters=pcg, admm_rho=10.0, eps_abs=0.0, eps_rel=0.0, check_every=1 << 30)

    def run(kind, n):
        s = sols[kind]
        if kind == "box_qp":
            return s.box_qp(Gb, Cb, g, c, lo, hi, max_admm_iters=n, **kw, **outs[kind])
        return s.box_qp_cross(Gb, Mb, Cb, g, c, lo, hi, max_admm_iters=n, **kw, **outs[kind])

    def timed(kind, n):
        """median host time (ms) of a blocking call: it ends in a stream synchronise"""
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(kind, n)
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    ran = {}
    for kind in sols:                                                       # warm-up, and every call must run all its iterations
        r = run(kind, long_)
        ran[kind] = bool((r.iters == long_).all()) and bool((r.status == _lib.QP_MAX_ITERS).all())
    same = all(torch.equal(outs["box_qp_cross"][k], outs["box_qp_cross_unfused"][k]) for k in ("x", "z", "y", "lam"))
    total, each = {k: [] for k in sols}, {k: [] for k in sols}
    for _ in range(rounds):
        for kind in sols:
            t_short, t_long = timed(kind, short), timed(kind, long_)
            total[kind].append(t_long)
            each[kind].append(1e3 * (t_long - t_short) / (long_ - short))
    out = dict(S=S, C=C, K=K, B=B, dtype=np.dtype(dt).name, pcg_iters=pcg, admm_iters=[short, long_], reps=reps, rounds=rounds,
               ran_every_iteration=ran, fused_equals_unfused=same,
               **{k + "_call_ms": spread(v) for k, v in total.items()}, **{k + "_iteration_us": spread(v) for k, v in each.items()})
    med = lambda k: out[k + "_iteration_us"]["median"]
    out["cross_extra_us_per_iteration"] = med("box_qp_cross") - med("box_qp")
    out["unfused_extra_us_per_iteration"] = med("box_qp_cross_unfused") - med("box_qp_cross")
    for s in sols.values():
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pcg", type=int, default=10)
    ap.add_argument("--short", type=int, default=50)
    ap.add_argument("--long", type=int, default=250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        lines.append(json.dumps(case(S, C, K, B, dt, a.pcg, a.short, a.long, a.reps, a.rounds)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
