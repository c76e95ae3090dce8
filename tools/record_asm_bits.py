"""Records tests/golden/asm_bits_parent.json: SHA-256 of the assembly's work buffers for every case of tests/asm_bits_cases.py,
from the library of the PARENT commit (the one before the Gauss-Jordan issue order changed).

    git worktree add build/parent <parent commit> && make -C build/parent/gato_python_amd/csrc -j8      # all six shapes
    cp build/parent/gato_python_amd/libgato_hip.so build/ab/libgato_hip_parent.so
    GATO_HIP_LIB=$PWD/build/ab/libgato_hip_parent.so python tools/record_asm_bits.py [out.json]          # on the GPU

(GATO_HIP_LIB is how tools/ab_libs.py points the package at an A/B library.)  Every case runs twice and must give the same
digests; with --check FILE the digests of the loaded library are compared with FILE instead of written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import asm_bits_cases as ab                        # noqa: E402

args = sys.argv[1:]
check = None
if args and args[0] == "--check":
    check, args = args[1], args[2:]
out = args[0] if args else ab.GOLDEN
digests = {}
for cid, case in ab.all_cases():
    first = ab.run_case(case)
    assert ab.run_case(case) == first, ("not reproducible", cid)
    digests[cid] = first
    same = all(first["stage"][b] == first["fused"][b] for b in ab.BUFFERS)
    print(cid, "stage == fused" if same else "stage != fused", flush=True)
if check:
    with open(check) as f:
        want = json.load(f)["digests"]
    bad = [cid for cid in digests if digests[cid] != want.get(cid)]
    print("library", os.environ.get("GATO_HIP_LIB", "(the package's own)"), "differs in" if bad else "matches", bad or check)
    sys.exit(1 if bad else 0)
doc = dict(what="SHA-256 of the raw bytes of each work buffer; stage = asm_mode 1, fused = asm_mode 2; %d PCG iterations" % ab.PCG_ITERS,
           recorded_from="parent commit library (see tools/record_asm_bits.py)", digests=digests)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", out, len(digests), "cases")
