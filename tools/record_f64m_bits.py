"""Records tests/golden/f64m_outside_loop_parent.json: SHA-256 of lambda and dz and the iteration count of every case of
tests/f64m_outside_loop_cases.py, from the library of the PARENT commit (the one before pcg_single_f64m_kernel's loads and its
hand-off of lambda to the dz helper blocks changed).

    git worktree add build/parent <parent commit> && make -C build/parent/gato_python_amd/csrc -j8
    cp build/parent/gato_python_amd/libgato_hip.so build/ab/libgato_hip_parent.so
    GATO_HIP_LIB=$PWD/build/ab/libgato_hip_parent.so python tools/record_f64m_bits.py [out.json]          # on the GPU

(GATO_HIP_LIB is how tools/ab_libs.py points the package at an A/B library.)  Every case runs twice and must give the same
digests, through the default route (pair = 2, images, dz in the helper blocks); with --check FILE the digests of the loaded
library are compared with FILE instead of written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f64m_outside_loop_cases as fc               # noqa: E402

args = sys.argv[1:]
check = None
if args and args[0] == "--check":
    check, args = args[1], args[2:]
out = args[0] if args else fc.GOLDEN
digests = {}
for cid, case in fc.all_cases():
    first, route = fc.run_case(case)
    assert route == dict(pair=2, image=1, dz_fused=2), (cid, route)
    assert fc.run_case(case)[0] == first, ("not reproducible", cid)
    digests[cid] = first
    print(cid, "iterations", first["iters"], flush=True)
if check:
    with open(check) as f:
        want = json.load(f)["digests"]
    bad = [cid for cid in digests if digests[cid] != want.get(cid)]
    print("library", os.environ.get("GATO_HIP_LIB", "(the package's own)"), "differs in" if bad else "matches", bad or check)
    sys.exit(1 if bad else 0)
doc = dict(what="SHA-256 of the raw bytes of lambda and dz, and the iteration count the solve reports; 14/7 fp64, synth.make_system(14, 7, K, seed=100 + K)",
           recorded_from="parent commit library (see tools/record_f64m_bits.py)", digests=digests)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", out, len(digests), "cases")
