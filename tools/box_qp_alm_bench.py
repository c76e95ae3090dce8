"""Hard state bounds by the augmented-Lagrangian outer loop beside ADMM with a polish, to the same eps, on
the same build in the same process: the two double integrators with a hard velocity bound, 6/3/20 seed 2, and the pinned 14/7/9
problem of tests/box_qp_alm_ref.py at B = 1 and replicated to B = 512.  Per problem the two methods are timed in alternation, round
after round (blocking wall time): per method the median, the range, the solves (ALM: reduced solves; ADMM: x-steps), how many
systems converged and - ALM - the outer steps and the last weight.  Prints one JSON line per problem.
--accuracy FILE also writes, per cell of tests/test_gpu_box_qp_alm.py, the device's |x - x*|_inf and the reference's own at the same
eps (the bar of that test is ten times the second; it is never computed from the first).
    python tools/box_qp_alm_bench.py [--reps 7] [--out FILE] [--accuracy FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                           # noqa: E402
import box_qp_active_ref as AS                         # noqa: E402
import box_qp_alm_ref as A                             # noqa: E402
from box_qp_device import dev_inputs, host, solver     # noqa: E402
from gato_python_amd import _lib                       # noqa: E402

ADMM_RHO = {"di57": 0.1, "di60": 0.1, "6_3_20": 10.0, "14_7_9": 1.0}      # box_qp_polish_ref.problem's penalties


def case(name, p, B, reps):
    s = p["s"]
    sol = solver(s.S, s.C, s.K, np.float64, batch=B)
    inp = dev_inputs(sol, [s] * B, [(p["lo"], p["hi"])] * B)
    kw = dict(rho=s.rho, exit_tol=1e-12, max_iters=500)
    out, times = {}, dict(alm=[], admm=[])

    def alm():
        out["alm"] = sol.box_qp_alm(*inp, **kw)

    def admm():
        r = sol.box_qp(*inp, admm_rho=ADMM_RHO[name], **kw)
        act = sol.box_qp_active_set(r.z, r.y, inp[4], inp[5])
        sol.box_qp_polish(*inp, act, r, **kw)
        out["admm"] = r

    runs = dict(alm=alm, admm=admm)
    for fn in runs.values():                                       # warm-up: every kernel loaded, every work area sized
        fn()
        torch.cuda.synchronize()
    for _ in range(reps):                                          # alternate the methods: the host and the clocks drift
        for m, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) * 1e6)
    row = dict(case=f"{B} x {name} ({s.S}/{s.C}/{s.K}) float64", systems=B, reps=reps)
    for m in runs:
        r = out[m]
        row.update({m + "_us": float(np.median(times[m])), m + "_us_min": float(min(times[m])), m + "_us_max": float(max(times[m])),
                    m + "_solves": int(r.iters.max()), m + "_converged": int((r.status == _lib.QP_CONVERGED).sum())})
    row.update(alm_outer=int(out["alm"].outer.max()), alm_weight=float(out["alm"].weight.max()),
               alm_us_per_solve=row["alm_us"] / row["alm_solves"], admm_us_per_step=row["admm_us"] / row["admm_solves"],
               admm_over_alm=row["admm_us"] / row["alm_us"],
               x_diff=float((out["alm"].x - out["admm"].x).abs().max()))
    sol.close()
    return row


def accuracy():
    rows = []
    for cells, f32 in ((A.F64_CASES, False), (A.F32_CASES, True)):
        for S, C, K in cells:
            p = A.alm_box(S, C, K, f32)
            sol = solver(S, C, K, np.float32 if f32 else np.float64)
            inp = dev_inputs(sol, [p["s"]], [(p["lo"], p["hi"])])
            r = sol.box_qp_alm(*inp, rho=p["s"].rho, eps_abs=p["eps"], eps_rel=p["eps"], max_iters=1000,
                               exit_tol=AS.F32_EXIT_TOL if f32 else 1e-20)
            x = host(r.x, 1, sol.N)[0]
            rows.append(dict(cell=f"{S}/{C}/{K} {'float32' if f32 else 'float64'}", seed=p["seed"], form=p["form"], dropped=p["drop"],
                             eps=p["eps"], status=int(r.status[0]), outer=int(r.outer[0]), solves=int(r.iters[0]), weight=float(r.weight[0]),
                             device_dist=float(np.abs(x - p["exact"]["x"]).max()),
                             reference_dist=float(np.abs(p["run"]["x"] - p["exact"]["x"]).max())))
            sol.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--accuracy")
    a = ap.parse_args()
    pin = A.alm_box(14, 7, 9)
    rows = []
    for name, p, B in [(n, A.named(n), 1) for n in A.NAMED] + [("14_7_9", pin, 1), ("14_7_9", pin, 512)]:
        rows.append(case(name, p, B, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    for path, content in ((a.out, "\n".join(json.dumps(r) for r in rows) + "\n"),
                          (a.accuracy, None)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(content if content is not None else json.dumps(accuracy(), indent=1) + "\n")


if __name__ == "__main__":
    main()
