"""Cost of the exact line search of the active-set iteration beside the undamped iteration, on the same
build in the same run: the three cases of tools/box_qp_pdas_bench.py with the state boxes of tools/box_qp_soft_bench.py, every
bound - the controls' too - soft with one weight and one cap.  Per case two calls of Solver.box_qp_pdas are timed in alternation,
round after round: `undamped` (gato_box_qp_pdas_huber) and `ls` (gato_box_qp_pdas_ls).  Per call: the reduced solves, how many
systems converged, the median wall time (blocking) in total and per solve and the spread (min, max) of the per-solve time over
the rounds.  --undamped-only times the first call alone (it needs no entry of this section: the tool then runs on an older build,
which is how the parent commit's per-solve time is taken).  Prints one JSON line per case.
    python tools/box_qp_linesearch_bench.py [--reps 7] [--weight 100] [--cap 1] [--max-solves 30] [--undamped-only] [--out FILE]"""
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


def case(S, C, K, B, dt, a):
    sol, inp, systems, boxes = problem(S, C, K, B, dt)
    rho = systems[0].rho
    f64 = dt == np.float64
    kw = dict(exit_tol=1e-12 if f64 else 1e-8, max_iters=500)
    eps = 1e-6 if f64 else 1e-4
    soft = [state_box(s, *b, a.weight) for s, b in zip(systems[:len(boxes)], boxes)]
    cat = lambda j: sol.to_device(np.concatenate([soft[b % len(soft)][j] for b in range(B)]).astype(dt))
    lo, hi = cat(0), cat(1)
    sinp = inp[:4] + (lo, hi)
    w = torch.full_like(lo, float(a.weight))           # every bound soft, the controls' too
    m = torch.full_like(lo, float(a.cap))
    variants = dict(undamped=dict(soft_weight=w, soft_cap=m))
    if not a.undamped_only:
        variants["ls"] = dict(soft_weight=w, soft_cap=m, line_search=True)
    out, times = {}, {name: [] for name in variants}

    def run(name):
        out[name] = sol.box_qp_pdas(*sinp, rho=rho, eps_abs=eps, eps_rel=eps, max_pdas_iters=a.max_solves, **kw, **variants[name])
        torch.cuda.synchronize()

    for name in variants:                                          # warm-up: every kernel of every variant loaded
        run(name)
    for _ in range(a.reps):                                        # alternate the variants: the host and the clocks drift
        for name in variants:
            t0 = time.perf_counter()
            run(name)
            times[name].append((time.perf_counter() - t0) * 1e6)
    row = dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", systems=B, weight=a.weight, cap=a.cap, reps=a.reps, max_solves=a.max_solves)
    for name in variants:
        its, status = out[name].iters.cpu().numpy(), out[name].status.cpu().numpy()
        solves = int(its.max())                                    # the batch runs until its last system froze
        per = np.asarray(times[name]) / solves
        row.update({name + "_solves_max": solves, name + "_converged": int((status == _lib.QP_CONVERGED).sum()),
                    name + "_us_total": float(np.median(times[name])), name + "_us_per_solve": float(np.median(per)),
                    name + "_us_per_solve_min": float(per.min()), name + "_us_per_solve_max": float(per.max())})
    if "ls" in out:
        al = out["ls"].alpha.cpu().numpy()
        row["ls_damped_steps_mean"] = float(((al > 0) & (al < 1)).sum(1).mean())
    sol.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--cap", type=float, default=1.0)
    ap.add_argument("--max-solves", type=int, default=30)
    ap.add_argument("--undamped-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        rows.append(case(S, C, K, B, dt, a))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
