"""Records profiles/asm_accuracy.json: the assembly's and dz's per-block error against the dense longdouble reference of
tests/asm_ref.py beside the two CPU orders' own, for the cases of tests/test_gpu_asm_ref.py (stage entries and whole calls in both
paths at every shape, K in 1, 2, 3, 5, both dtypes; the batches; the horizon past the grid caps).

    python tools/asm_accuracy.py [out.json]          # on the GPU; default profiles/asm_accuracy.json

Per buffer and dtype: the largest device error and the largest CPU-order error in eps, and the largest ratio
device / max(worse CPU order, floor) - the number the bar's factor (asm_ref.FACTOR) is held against."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import asm_ref as ar                               # noqa: E402
from gato_python_amd.solver import Solver         # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "asm_accuracy.json")
rows = {}


def note(group, dt, e_dev, e_or, names, what):
    eps = ar.eps_of(dt)
    for n in names:
        eo = max(e[n] for e in e_or)
        r = rows.setdefault(f"{group} {dt} {n}", dict(group=group, dtype=dt, buffer=n, cases=0, device_eps=0.0, cpu_orders_eps=0.0,
                                                      ratio=0.0, worst="", past_bar=0))
        ratio = e_dev[n] / max(eo, ar.FLOOR_EPS * eps)
        r["cases"] += 1
        r["device_eps"] = max(r["device_eps"], e_dev[n] / eps)
        r["cpu_orders_eps"] = max(r["cpu_orders_eps"], eo / eps)
        if ratio > r["ratio"]:
            r["ratio"], r["worst"] = ratio, what
        r["past_bar"] += int(not e_dev[n] <= ar.bar([eo], dt))


for (S, C, K, dt) in ar.stage_cases():
    cid = ar.case_id(S, C, K, dt)
    _, e_dev, e_or = ar.device_stage_case(S, C, K, dt)
    note("stage entries", dt, e_dev, e_or, ar.STAGE_BUFFERS, cid)
    s, ref = ar.system_of(S, C, K, dt), ar.reference_of(S, C, K, dt)
    for mode, name in ((1, "linsys, stage launches"), (2, "linsys, fused launch")):
        sol = Solver(S, C, K, np.dtype(dt))
        got = ar.whole_call(sol, s, mode)
        sol.close()
        note(name, dt, ar.errors(got, ref.buf, S, C, K, ar.WHOLE_BUFFERS), ar.oracle_chain_errors(S, C, K, dt), ar.WHOLE_BUFFERS, cid)
    print(cid, flush=True)

for (S, C, K) in ar.BATCH_CASES:
    for dt in ar.DTYPES:
        for mode in (1, 2):
            for b, (e, e_or) in enumerate(ar.device_batch_case(S, C, K, dt, mode)[1]):
                note("batch of 3", dt, e, e_or, ar.WHOLE_BUFFERS, f"{ar.case_id(S, C, K, dt, b)} asm_mode {mode}")
        print("batch", S, C, K, dt, flush=True)

for dt in ar.DTYPES:
    _, _, e_dev, e_or, _ = ar.long_horizon_case(dt)
    note("stage entries, %d/%d/%d (C order alone)" % ar.LONG, dt, e_dev, e_or, ar.STAGE_BUFFERS, "windows at %s" % (ar.LONG_WINDOWS,))
    print("long", dt, flush=True)

doc = dict(what="per-block error max|got - truth| / max|truth| against the dense longdouble reference (tests/asm_ref.py), largest over the "
                "cases of a group, in eps of the dtype; ratio = device / max(worse of the C and numpy orders, floor)",
           inputs=dict(cond=ar.COND, grade=ar.GRADE, rho=ar.RHO), bar=dict(factor=ar.FACTOR, floor_eps=ar.FLOOR_EPS),
           device=torch.cuda.get_device_name(0), max_ratio=max(r["ratio"] for r in rows.values()),
           past_bar=sum(r["past_bar"] for r in rows.values()), rows=list(rows.values()))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", out, "largest ratio %.2f" % doc["max_ratio"], "past the bar:", doc["past_bar"])
