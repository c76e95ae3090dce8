"""Cost of a capped (Huber) solve of the active-set iteration beside an uncapped soft one (section 3.10), on
the same build in the same run: the three cases of tools/box_qp_soft_bench.py with its soft state boxes.  Per case three calls of
Solver.box_qp_pdas are timed in alternation, round after round: `soft` (gato_box_qp_pdas_soft), `inf` (gato_box_qp_pdas_huber with
every cap +inf: the same solves, bit for bit, through the capped kernels) and `cap` (a finite cap on every soft state: other solves,
so only its time per solve compares).  Per call: the reduced solves, the median wall time (blocking) in total and per solve, and
the spread (min, max) of the per-solve time over the rounds.  Prints one JSON line per case.
    python tools/box_qp_huber_bench.py [--reps 7] [--weight 100] [--cap 1] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch                                           # noqa: E402
from gato_python_amd import _lib                       # noqa: E402
from box_qp_polish_bench import problem                # noqa: E402
from box_qp_soft_bench import state_box                # noqa: E402


def case(S, C, K, B, dt, reps, weight, cap):
    sol, inp, systems, boxes = problem(S, C, K, B, dt)
    rho = systems[0].rho
    f64 = dt == np.float64
    kw = dict(exit_tol=1e-12 if f64 else 1e-8, max_iters=500)
    eps = 1e-6 if f64 else 1e-4
    soft = [state_box(s, *b, weight) for s, b in zip(systems[:len(boxes)], boxes)]
    cat = lambda j: sol.to_device(np.concatenate([soft[b % len(soft)][j] for b in range(B)]).astype(dt))
    sinp = inp[:4] + (cat(0), cat(1))
    w = cat(2)
    inf = torch.full_like(w, float("inf"))
    variants = dict(soft=dict(soft_weight=w), inf=dict(soft_weight=w, soft_cap=inf),
                    cap=dict(soft_weight=w, soft_cap=torch.where(w > 0, float(cap), float("inf")).to(w.dtype)))
    out, times = {}, {name: [] for name in variants}

    def run(name):
        out[name] = sol.box_qp_pdas(*sinp, rho=rho, eps_abs=eps, eps_rel=eps, max_pdas_iters=30, **kw, **variants[name])
        torch.cuda.synchronize()

    for name in variants:                                          # warm-up: every kernel of every variant loaded
        run(name)
    for _ in range(reps):                                          # alternate the variants: the host and the clocks drift
        for name in variants:
            t0 = time.perf_counter()
            run(name)
            times[name].append((time.perf_counter() - t0) * 1e6)
    same = all(torch.equal(getattr(out["soft"], f), getattr(out["inf"], f)) for f in ("x", "z", "y", "lam", "iters", "status", "act"))
    row = dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", systems=B, weight=weight, cap=cap, reps=reps, inf_equals_soft=bool(same))
    for name in variants:
        its, status = out[name].iters.cpu().numpy(), out[name].status.cpu().numpy()
        solves = int(its.max())                                    # the batch runs until its last system froze
        per = np.asarray(times[name]) / solves
        row.update({name + "_solves_max": solves, name + "_converged": int((status == _lib.QP_CONVERGED).sum()),
                    name + "_us_total": float(np.median(times[name])), name + "_us_per_solve": float(np.median(per)),
                    name + "_us_per_solve_min": float(per.min()), name + "_us_per_solve_max": float(per.max())})
    act = out["cap"].act.view(B, -1).cpu().numpy()
    row["cap_saturated_mean"] = float((np.abs(act) == 2).sum(1).mean())
    sol.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--cap", type=float, default=1.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        rows.append(case(S, C, K, B, dt, a.reps, a.weight, a.cap))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
