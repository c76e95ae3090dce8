"""Cost of the primal-dual active-set iteration for box QPs beside ADMM + polish on the same QP in the
same run.  Per case: the reduced solves a cold Solver.box_qp_pdas call takes, its wall time (blocking) in total and per solve,
how many systems end CONVERGED; and the wall time of Solver.box_qp followed by the active set and one polish, with its ADMM
x-steps and accepted polishes.  The cases and the control-only boxes (half the unconstrained controls) are those of
tools/box_qp_polish_bench.py.  Prints one JSON line per row.
    python tools/box_qp_pdas_bench.py [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gato_python_amd import _lib                       # noqa: E402
from box_qp_polish_bench import problem, wall          # noqa: E402


def case(S, C, K, B, dt, reps):
    sol, inp, systems, boxes = problem(S, C, K, B, dt)
    rho = systems[0].rho
    f64 = dt == np.float64
    kw = dict(exit_tol=1e-12 if f64 else 1e-8, max_iters=500)
    eps = 1e-6 if f64 else 1e-4
    out = {}

    def pdas():
        out["pdas"] = sol.box_qp_pdas(*inp, rho=rho, eps_abs=eps, eps_rel=eps, max_pdas_iters=30, **kw)

    pdas_ms = wall(pdas, reps)
    r = out["pdas"]
    its, status = r.iters.cpu().numpy(), r.status.cpu().numpy()
    solves = int(its.max())                                         # the batch runs until its last system froze

    def admm_polish():
        a = sol.box_qp(*inp, rho=rho, admm_rho=1.0, eps_abs=eps, eps_rel=eps, max_admm_iters=4000, **kw)
        act = sol.box_qp_active_set(a.z, a.y, inp[4], inp[5])
        sol.box_qp_polish(*inp, act, a, rho=rho, eps_abs=eps, eps_rel=eps, **kw)
        out["admm"] = a

    admm_ms = wall(admm_polish, reps)
    a = out["admm"]
    same = None
    conv = (status == _lib.QP_CONVERGED) & (a.status.cpu().numpy() == _lib.QP_CONVERGED)
    if conv.any():                                                  # the two answers on the systems both solved
        dx = (r.x.view(B, -1) - a.x.view(B, -1)).abs().amax(1).cpu().numpy()
        same = float(dx[conv].max())
    sol.close()
    return dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", systems=B, pdas_solves_max=solves,
                pdas_solves_mean=float(its.mean()), pdas_converged=int((status == _lib.QP_CONVERGED).sum()),
                us_pdas_total=pdas_ms * 1e3, us_per_pdas_solve=pdas_ms * 1e3 / solves,
                us_admm_polish_total=admm_ms * 1e3, admm_iters_mean=float(a.iters.cpu().numpy().mean()),
                admm_converged=int((a.status.cpu().numpy() == _lib.QP_CONVERGED).sum()),
                polish_accepted=int((a.polished.cpu().numpy() == _lib.POLISH_ACCEPTED).sum()), max_x_difference=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        rows.append(case(S, C, K, B, dt, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
