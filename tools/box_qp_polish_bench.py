"""Cost of the box-QP polish and of the differentiable layer.  Per case: microseconds of one polish
call (active set + assembly + PCG + finish, blocking) beside one ADMM iteration and one whole solve (Solver.linsys_blocks)
measured in the same run, and the forward and backward of box_qp_layer; then, for each problem of the section's table, the
fewest ADMM iterations after which the polish is accepted against the iterations plain ADMM needs to converge.  Control-only
boxes at half the unconstrained controls.  Prints one JSON line per row.
    python tools/box_qp_polish_bench.py [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gato_python_amd                                 # noqa: E402
from gato_python_amd import _lib, synth                # noqa: E402
from gato_python_amd.solver import Solver              # noqa: E402
from oracle import gato_oracle as o                    # noqa: E402


def wall(fn, reps):
    """median wall time (ms) of a blocking call, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def control_box(s):
    dz, _ = synth.dense_kkt_solve(s)
    n = s.S + s.C
    ctrl = (np.arange(s.N) % n) >= s.S
    w = np.where(ctrl, 0.5 * np.abs(dz) + 0.05, np.inf)
    return -w, w


def problem(S, C, K, B, dt, seed=700):
    distinct = [synth.make_system(S, C, K, seed=seed + b) for b in range(min(B, 8))]
    systems = [distinct[b % len(distinct)] for b in range(B)]
    boxes = [control_box(s) for s in distinct]
    sol = Solver(S, C, K, dt, batch=B)
    Gs, Cs = zip(*(o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, S, C, K, 0.0) for s in systems))
    cat = lambda arrs: sol.to_device(np.concatenate([np.asarray(a, np.float64) for a in arrs]).astype(dt))
    inp = (cat(Gs), cat(Cs), cat([s.g for s in systems]), cat([s.c for s in systems]),
           cat([boxes[b % len(boxes)][0] for b in range(B)]), cat([boxes[b % len(boxes)][1] for b in range(B)]))
    return sol, inp, systems, boxes


def case(S, C, K, B, dt, reps):
    sol, inp, systems, boxes = problem(S, C, K, B, dt)
    rho = systems[0].rho
    f64 = dt == np.float64
    kw = dict(exit_tol=1e-12 if f64 else 1e-8, max_iters=500)
    # fp32: the polished residuals of 14/7/512 sit between 1e-5 and 1e-4 (the active set is the reference's), and ADMM at
    # eps 1e-4 stops before its active set is final - so the polish timed here follows 300 fixed ADMM iterations
    eps = 1e-6 if f64 else 1e-4
    adm = dict(kw, admm_rho=1.0, eps_abs=eps, eps_rel=eps)
    fixed = 100
    fixed_ms = wall(lambda: sol.box_qp(*inp, rho=rho, **dict(adm, eps_abs=0.0, eps_rel=0.0, max_admm_iters=fixed,
                                                                check_every=fixed)), reps)
    r = sol.box_qp(*inp, rho=rho, **(dict(adm, max_admm_iters=4000) if f64 else
                                     dict(adm, eps_abs=0.0, eps_rel=0.0, max_admm_iters=300)))
    torch.cuda.synchronize()
    admm_its = r.iters.cpu().numpy()

    def polish():
        act = sol.box_qp_active_set(r.z, r.y, inp[4], inp[5])
        sol.box_qp_polish(*inp, act, r, rho=rho, eps_abs=eps, eps_rel=eps, **kw)

    pol_ms = wall(polish, reps)
    codes = r.polished.cpu().numpy()
    lam, dz = sol.new(B * S * K), sol.new(B * sol.N)
    solve_ms = wall(lambda: sol.linsys_blocks(inp[0], inp[1], inp[2], inp[3], kw["exit_tol"], kw["max_iters"], rho, lam, dz),
                    reps)
    # the layer: forward (ADMM + active set + polish) and backward (adjoint re-solve + gradient launches)
    tdt = torch.float64 if f64 else torch.float32
    distinct = [_blocks(s) for s in systems[:min(B, 8)]]
    blocks = [np.stack([distinct[b % len(distinct)][i] for b in range(B)]) for i in range(7)]
    ts = [torch.from_numpy(b).to("cuda", tdt).requires_grad_() for b in blocks]
    bnd = []
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        parts = [_split(boxes[b % len(boxes)][j], S, C, K)[i] for b in range(B)]
        bnd.append(torch.from_numpy(np.stack(parts)).to("cuda", tdt).requires_grad_())
    lkw = dict(rho=rho, max_admm_iters=4000, **adm)
    out = {}

    def fwd():
        out["x"], out["lam"], out["info"] = gato_python_amd.box_qp_layer(*ts, *bnd, **lkw)

    fwd_ms = wall(fwd, reps)
    w = torch.randn_like(out["x"])

    def bwd():
        for t in ts + bnd:
            t.grad = None
        (out["x"] * w).sum().backward(retain_graph=True)

    accepted = int((out["info"].polished.cpu().numpy() == 0).sum())
    bwd_ms = wall(bwd, reps) if accepted == B else None             # a system not polished has no gradient
    return dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", us_polish=pol_ms * 1e3, us_per_admm_iter=fixed_ms * 1e3 / fixed,
                us_whole_solve=solve_ms * 1e3, polish_accepted=int((codes == _lib.POLISH_ACCEPTED).sum()), systems=B,
                admm_iters_mean=float(admm_its.mean()), us_layer_forward=fwd_ms * 1e3,
                us_layer_backward=None if bwd_ms is None else bwd_ms * 1e3,
                layer_polish_accepted=accepted)


def _blocks(s):
    import kkt_grad_ref
    return kkt_grad_ref.blocks_of(s)


def _split(v, S, C, K):
    import box_qp_polish_ref
    return box_qp_polish_ref.split_states_controls(v, S, C, K)


def table():
    """per problem of DESIGN.md 3.8: plain ADMM iterations to eps 1e-6 (at most 4000) and the fewest ADMM iterations (of a
    ladder) after which the polish is accepted"""
    import box_qp_polish_ref as P
    rows = []
    ladder = (5, 10, 25, 50, 60, 100, 200, 400, 800, 1000, 1100, 1200, 1300, 1500, 2000, 3000)
    for name in P.PROBLEMS:
        s, lo, hi, arho = P.problem(name)
        sol = Solver(s.S, s.C, s.K, np.float64)
        Gs, Cs = o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, s.S, s.C, s.K, 0.0)
        inp = tuple(sol.to_device(np.asarray(a, np.float64)) for a in (Gs, Cs, s.g, s.c, lo, hi))
        kw = dict(rho=s.rho, exit_tol=1e-20, max_iters=1000, admm_rho=arho)
        plain = sol.box_qp(*inp, max_admm_iters=4000, **kw)
        first = None
        for its in ladder:
            r = sol.box_qp(*inp, max_admm_iters=its, **kw)
            act = sol.box_qp_active_set(r.z, r.y, inp[4], inp[5])
            if int(sol.box_qp_polish(*inp, act, r, rho=s.rho, exit_tol=1e-20, max_iters=1000)[0]) == _lib.POLISH_ACCEPTED:
                first = its
                break
        rows.append(dict(case=f"table {name}", plain_admm_iters=int(plain.iters[0]), plain_status=int(plain.status[0]),
                         polish_accepted_from=first, ladder=list(ladder)))
        sol.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        rows.append(case(S, C, K, B, dt, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    for row in table():
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
