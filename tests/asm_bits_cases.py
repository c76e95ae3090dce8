"""Cases and runner of the assembly bit-pinning (tests/test_gpu_asm_bits.py, tests/test_asm_bits_golden_cpu.py,
tools/record_asm_bits.py): one seeded system per case, through the stage launches and through the fused launch, SHA-256
of the raw bytes of every work buffer downstream of the Gauss-Jordan eliminations.

The stage path and the fused path share gj_inverse_reg, so comparing them with each other cannot see a change of the
elimination's arithmetic; the digests in tests/golden/asm_bits_parent.json were recorded once from the library of the
commit BEFORE the elimination's issue order was changed, and pin every bit against that commit."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "asm_bits_parent.json")
BUFFERS = ("Ginv", "S", "Pinv", "gamma", "lam", "dz")
PATHS = (("stage", 1), ("fused", 2))                     # name -> solver option asm_mode
PCG_ITERS = 3

# smallest sizes at which each code path of the eliminations and of the fused launch can go wrong: n = 14 and 7 (the flagship), 2 / 1
# (a 1 x 1 elimination: no row update at all), 4 / 2, 6 / 3, 32 / 16 (the augmented matrix fills all 64 lanes; multipliers in two
# groups); K = 1 (first knot only), 2 (k == 1: the left neighbour's theta is -Q_0), 3 (first knot whose left theta is a Schur
# block), 5 (last knot: no R_k, with full knots in front of it)
SHAPES = ((14, 7), (2, 1), (4, 2), (6, 3), (32, 16))
KNOTS = (1, 2, 3, 5)
DTYPES = ("float64", "float32")


def case_id(S, C, K, dt, batch=1, pivot=None):
    return f"{S}-{C}-{K}-{dt}-b{batch}" + (f"-pivot{pivot}" if pivot else "")


def all_cases():
    """[(id, dict(S, C, K, dt, batch, pivot))] in a fixed order."""
    out = []
    for (S, C) in SHAPES:
        for K in KNOTS:
            for dt in DTYPES:
                out.append((case_id(S, C, K, dt), dict(S=S, C=C, K=K, dt=dt, batch=1, pivot=None)))
    for dt in DTYPES:                                    # one batch: grid.y > 1 in every launch
        out.append((case_id(14, 7, 3, dt, 3), dict(S=14, C=7, K=3, dt=dt, batch=3, pivot=None)))
    for pivot in ("1e-300", "1e+300"):                   # the reciprocal at the ends of the exponent range (fp64)
        out.append((case_id(14, 7, 5, "float64", 1, pivot), dict(S=14, C=7, K=5, dt="float64", batch=1, pivot=pivot)))
    return out


def systems_of(case):
    """The case's seeded systems (one per batch entry).  Dense Q_k, so that the Q eliminations have non-zero multipliers."""
    from gato_python_amd import synth
    S, C, K = case["S"], case["C"], case["K"]
    seed = 1000 * S + 10 * K
    if case["pivot"] is None:
        return [synth.make_system(S, C, K, seed=seed + b, dense_q=True) for b in range(case["batch"])]
    # every pivot of Q_2 near 1e-300 (its inverse, phi and theta of the knots behind it near 1e+300) or near 1e+300; rho = 0
    # because rho on the diagonal would be the pivot otherwise
    Q, R, A, B, q, r, c = synth.make_blocks(S, C, K, seed, dense_q=True)
    Q[2] *= float(case["pivot"])
    return [synth.blocks_to_csr(Q, R, A, B, q, r, c, rho=0.0, dense_q=True)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(case):
    """{path: {buffer: digest}} of the library that gato_python_amd loads, on cuda:0."""
    import torch
    from gato_python_amd.solver import Solver
    S, C, K, B = case["S"], case["C"], case["K"], case["batch"]
    dt = np.dtype(case["dt"])
    systems = systems_of(case)
    out = {}
    for name, mode in PATHS:
        sol = Solver(S, C, K, dt, batch=B)
        sol.set_option("asm_mode", mode)
        if B == 1:
            dev = sol.upload_system(systems[0])
            sol.linsys(*dev, 0.0, PCG_ITERS, systems[0].rho)
        else:
            dev = sol.upload_batch(systems)
            lam, dz = sol.new(B * S * K), sol.new(B * sol.N)
            sol.linsys_batched(*dev, 0.0, PCG_ITERS, systems[0].rho, lam, dz)
        torch.cuda.synchronize()
        sol.check_status()
        assert sol.get_option("last_asm_fused") == mode - 1, (name, sol.get_option("last_asm_fused"))
        got = {b: sol.read_buffer(b) for b in BUFFERS if b not in ("lam", "dz") or B == 1}
        if B > 1:
            got["lam"], got["dz"] = lam.cpu().numpy(), dz.cpu().numpy()
        sol.close()
        out[name] = {b: digest(got[b]) for b in BUFFERS}
    return out
