"""Cases and runner of the bit-pinning of the one-workgroup fp64 solve (tests/test_gpu_f64m_outside_loop.py,
tools/record_f64m_bits.py): whole solves at 14/7 in fp64 through pcg_single_f64m_kernel, SHA-256 of the raw bytes of lambda
and dz plus the iteration count.

What that kernel does OUTSIDE its loop (the order and the route of its loads of gamma, S and Pinv, the hand-off of lambda to
the dz helper blocks) may not change a bit of any result.  Routes of one library cannot check each other against a change
that all of them share, so tests/golden/f64m_outside_loop_parent.json holds digests recorded once from the library of the
commit BEFORE those changes (tools/record_f64m_bits.py)."""
import ctypes as ct
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "f64m_outside_loop_parent.json")
S, C = 14, 7
# the smallest K the kernel serves (17 knots = 119 two-row lanes; 16 knots in the DPP rows whatever K), two-row lane counts just
# short of the wave boundaries at 128 and 192 (K = 34: 126, K = 42: 182) and across one (K = 44: 196), and the largest (49: 231, 50: 238)
KNOTS = (33, 34, 42, 44, 49, 50)
STOPS = ((0.0, 100), (1e-9, 300))             # (exit_tol, max_iters): a fixed number of iterations, and a converged solve


def case_id(K, tol, iters):
    return f"K{K}-tol{tol:g}-it{iters}"


def all_cases():
    return [(case_id(K, tol, it), dict(K=K, tol=tol, iters=it)) for K in KNOTS for (tol, it) in STOPS]


_SYSTEMS = {}


def system_of(K, dtype=np.float64):
    from gato_python_amd import synth
    if K not in _SYSTEMS:
        _SYSTEMS[K] = synth.make_system(S, C, K, seed=100 + K)
    return _SYSTEMS[K]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def read_iters(sol):
    import torch
    buf = (ct.c_int * 1)()
    torch.cuda.synchronize()
    assert ct.CDLL("libamdhip64.so").hipMemcpy(buf, ct.c_void_p(sol.buffer_ptr(8)), 4, 2) == 0
    return int(buf[0])


class Solve:
    """One solver on one seeded system; run() is one whole solve into NaN-filled lambda / dz (lam0: true warm start)."""

    def __init__(self, K, dtype=np.float64, **opts):
        from gato_python_amd.solver import Solver
        self.K, self.s = K, system_of(K)
        self.sol = Solver(S, C, K, dtype)
        for k, v in opts.items():
            self.sol.set_option(k, v)
        self.dev = self.sol.upload_system(self.s)
        self.lam, self.dz = self.sol.new(S * K), self.sol.new(self.sol.N)

    def run(self, tol, iters, lam0=None, launched=None):
        """launched: called behind the solve's launches and in front of the wait for them."""
        import torch
        if lam0 is None:
            self.lam.fill_(float("nan"))
        else:
            self.lam.copy_(torch.from_numpy(np.ascontiguousarray(lam0, self.sol.np_dtype)))
        self.dz.fill_(float("nan"))
        self.sol.linsys(*self.dev, tol, iters, self.s.rho, self.lam, self.dz)
        if launched is not None:
            launched()
        torch.cuda.synchronize()
        self.sol.check_status()
        return dict(lam=digest(self.lam.cpu().numpy()), dz=digest(self.dz.cpu().numpy()), iters=read_iters(self.sol))

    def route(self):
        g = self.sol.get_option
        return dict(pair=g("last_pair"), image=g("last_image"), dz_fused=g("last_dz_fused"))

    def close(self):
        self.sol.close()


def run_case(case, **opts):
    """{lam, dz, iters} of the library that gato_python_amd loads, on cuda:0, and the route the solve took."""
    sv = Solve(case["K"], **opts)
    out = sv.run(case["tol"], case["iters"])
    route = sv.route()
    sv.close()
    return out, route
