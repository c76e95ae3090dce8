"""Cost of the active-set iteration with soft state bounds beside the hard iteration on the control-only
box of section 3.9, on the same build in the same run.  Per case, for both: the reduced solves a cold Solver.box_qp_pdas call
takes, its wall time (blocking) in total and per solve, how many systems end CONVERGED.  The systems and the control boxes are
those of tools/box_qp_polish_bench.py; the soft run adds a box around half the unconstrained value of every state off x_0 with
weight 100 (the state boxes on which the hard iteration cycles).  Prints one JSON line per row.
    python tools/box_qp_soft_bench.py [--reps 5] [--weight 100] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gato_python_amd import _lib, synth                # noqa: E402
from box_qp_polish_bench import problem, wall          # noqa: E402


def state_box(s, lo, hi, weight):
    """(lo, hi, w): the control box (lo, hi) plus -+(0.5 |dz| + 0.05) on every state off x_0, those soft with `weight`."""
    dz, _ = synth.dense_kkt_solve(s) if s.N <= 4000 else (sparse_dz(s), None)
    n, idx = s.S + s.C, np.arange(s.N)
    state = (idx % n < s.S) & (idx >= s.S)
    half = 0.5 * np.abs(dz) + 0.05
    return np.where(state, -half, lo), np.where(state, half, hi), np.where(state, float(weight), 0.0)


def sparse_dz(s):
    from scipy import sparse
    from scipy.sparse.linalg import splu
    N, SK = s.N, s.S * s.K
    G = sparse.csr_matrix((np.asarray(s.G_val, np.float64), s.G_col, s.G_row), shape=(N, N)) + s.rho * sparse.identity(N)
    Cm = sparse.csr_matrix((np.asarray(s.C_val, np.float64), s.C_col, s.C_row), shape=(SK, N))
    return splu(sparse.bmat([[G, Cm.T], [Cm, None]], format="csc")).solve(np.concatenate([s.g, s.c]))[:N]


def case(S, C, K, B, dt, reps, weight):
    sol, inp, systems, boxes = problem(S, C, K, B, dt)
    rho = systems[0].rho
    f64 = dt == np.float64
    kw = dict(exit_tol=1e-12 if f64 else 1e-8, max_iters=500)
    eps = 1e-6 if f64 else 1e-4
    soft = [state_box(s, *b, weight) for s, b in zip(systems[:len(boxes)], boxes)]
    cat = lambda j: sol.to_device(np.concatenate([soft[b % len(soft)][j] for b in range(B)]).astype(dt))
    sinp = inp[:4] + (cat(0), cat(1))
    w = cat(2)
    out = {}

    def run(name, args, **extra):
        def f():
            out[name] = sol.box_qp_pdas(*args, rho=rho, eps_abs=eps, eps_rel=eps, max_pdas_iters=30, **kw, **extra)
        ms = wall(f, reps)
        its, status = out[name].iters.cpu().numpy(), out[name].status.cpu().numpy()
        solves = int(its.max())                                     # the batch runs until its last system froze
        return dict(solves_max=solves, solves_mean=float(its.mean()), converged=int((status == _lib.QP_CONVERGED).sum()),
                    us_total=ms * 1e3, us_per_solve=ms * 1e3 / solves)

    hard = run("hard", inp)
    sft = run("soft", sinp, soft_weight=w)
    act = out["soft"].act.view(B, -1).cpu().numpy()
    sol.close()
    row = dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", systems=B, weight=weight,
               soft_active_mean=float(((act != 0) & (w.view(B, -1).cpu().numpy() > 0)).sum(1).mean()))
    row.update({"soft_" + k: v for k, v in sft.items()})
    row.update({"hard_control_box_" + k: v for k, v in hard.items()})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        rows.append(case(S, C, K, B, dt, a.reps, a.weight))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
