"""Records profiles/pcg_accuracy.json: the per-knot error of every PCG route, of dz from every launch that forms it and of the
re-solve's gamma against the longdouble references of tests/pcg_ref.py, beside the two CPU orders' own, for the cases of
tests/test_gpu_pcg_ref.py.

    python tools/pcg_accuracy.py [out.json]          # on the GPU; default profiles/pcg_accuracy.json
    python tools/pcg_accuracy.py --cpu               # no GPU: the CPU orders against each other, the counts the factors come from

Per case and buffer: the device's error, the CPU orders' errors and the bar, in eps of the dtype, and the ratio
device / max(worse CPU order, floor); the largest ratio overall."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import asm_ref as ar                               # noqa: E402
import pcg_ref as pr                               # noqa: E402


def cpu_counts():
    for n in pr.NS:
        past, ratio, lo, hi, cmp = {1: 0, 2: 0, 4: 0, 8: 0}, 0.0, float("inf"), 0.0, 0
        for case in pr.CASES:
            eps = ar.eps_of(case.dt)
            for seed in pr.SEEDS:
                e = [x[f"lambda after {n}"] for x in pr.cpu_pcg_errors(case.name, seed)]
                lo, hi = min(lo, min(e) / eps), max(hi, max(e) / eps)
                for x, y in (e, e[::-1]):
                    cmp += 1
                    ratio = max(ratio, x / max(y, pr.FLOOR_EPS * eps))
                    for f in past:
                        past[f] += int(not x <= ar.bar([y], case.dt, f))
        print(f"n = {n}: {cmp} comparisons, errors {lo:.0f} - {hi:.0f} eps, past 1 / 2 / 4 / 8 x: {list(past.values())}, "
              f"largest ratio {ratio:.2f}, factor used {pr.PCG_FACTOR[n]:.0f}")


if "--cpu" in sys.argv[1:]:
    cpu_counts()
    sys.exit(0)

import torch                                       # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pcg_accuracy.json")
rows, wrong = [], []


def record(what, dt, e_dev, e_or, factor):
    eps = ar.eps_of(dt)
    for n in e_dev:
        eo = [e[n] for e in e_or]
        rows.append(dict(case=what, dtype=dt, buffer=n, device_eps=round(e_dev[n] / eps, 2), cpu_orders_eps=[round(x / eps, 2) for x in eo],
                         bar_eps=round(ar.bar(eo, dt, factor) / eps, 2), factor=factor,
                         ratio=round(e_dev[n] / max(max(eo), pr.FLOOR_EPS * eps), 3), past_bar=int(not e_dev[n] <= ar.bar(eo, dt, factor))))


def note(group, name, result):
    facts, _ = result
    wrong.extend(f"{group}: {what}" for what, ok in facts if not ok)
    print(group, name, flush=True)


dev = pr.Device()
for case in pr.CASES:
    note("pcg routes", case.name, pr.run_pcg_route(case, dev, record=record))
for case in pr.DZ_CASES:
    note("dz epilogues", case.name, pr.run_dz_case(case, dev, record=record))
for case, nofuse in pr.RESOLVE_RUNS:
    note("re-solve", case.name, pr.run_resolve_case(case, nofuse, dev, record=record))

worst = max(rows, key=lambda r: r["ratio"])
doc = dict(what="per-knot error max|got - truth| / max|truth| against the longdouble references of tests/pcg_ref.py (lambda after n fixed "
                "iterations: textbook PCG on the dense matrices; dz: the back-substitution of the device's own lambda; gamma: c - C G^-1 g), "
                "in eps of the dtype; ratio = device / max(worse of the two CPU orders, floor)",
           inputs=dict(cond=ar.COND, grade=ar.GRADE, rho=ar.RHO),
           bar=dict(pcg_factor={str(n): f for n, f in pr.PCG_FACTOR.items()}, gamma_dz_factor=pr.FACTOR, floor_eps=pr.FLOOR_EPS),
           device=torch.cuda.get_device_name(0), max_ratio=worst["ratio"], worst=f"{worst['case']} {worst['buffer']}",
           past_bar=sum(r["past_bar"] for r in rows), other_checks_failed=wrong, rows=rows)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", out, "largest ratio %.2f (%s)" % (doc["max_ratio"], doc["worst"]), "past the bar:", doc["past_bar"], "other checks failed:", wrong)
