"""The C calls behind the public Solver API, as data: every call of a fixed script of Solver methods with its function name, its
scalar arguments' values, null / non-null per pointer argument and which non-null pointers of the call share an address.  The
object _lib.lib() returns is wrapped in a recorder for the length of the script, so the trace is what solver.py hands the
library and nothing of what the library computes.  tests/test_gpu_solver_calls.py compares a fresh trace with
tests/golden/solver_calls.json, recorded by this tool on the commit before solver.py's operand table; the script uses public
methods only, so it runs on either side of such a change.  A box-QP call's parameter record is noted whole: the polish, active-set
and augmented-Lagrangian entries leave its ADMM fields at the library's defaults (max_admm_iters 4000) and do not read them; the
ADMM calls of the script set max_admm_iters to 50.
    python tools/solver_call_trace.py [--out FILE]"""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import _lib, synth                 # noqa: E402
from gato_python_amd.solver import Solver               # noqa: E402

TOL, ITERS, ADMM_ITERS, RHO = 1e-10, 20, 50, 1e-3        # max_iters <= 20 and max_admm_iters <= 50 in every call
_BYREF = type(ct.byref(ct.c_int()))


class Recorder:
    """Stands in for the ctypes library: every function called through it is recorded, then called.  Only calls on solvers
    created through this recorder count (another solver's destructor may run at any time)."""

    def __init__(self, real):
        self._real, self.calls, self._mine = real, [], set()

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("gato_"):
            return fn

        def call(*args):
            h = args[0].value if args and isinstance(args[0], ct.c_void_p) else None
            foreign = h is not None and h not in self._mine and not name.startswith("gato_solver_create")
            if not foreign:
                self.calls.append(dict(fn=name, args=[_arg(a) for a in args], alias=_alias(args)))
            rc = fn(*args)
            if name.startswith("gato_solver_create"):
                self._mine.add(args[-1]._obj.value)
            return rc
        return call


def _address(a):
    return a.value if isinstance(a, ct.c_void_p) and a.value else None


def _arg(a):
    if a is None:
        return "null"
    if isinstance(a, ct.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, bytes):
        return a.decode()
    obj = a._obj if isinstance(a, _BYREF) else a
    if isinstance(obj, ct.Structure):
        return {name: getattr(obj, name) for name, _ in obj._fields_}
    return "out"                                         # a ctypes scalar or array the call writes


def _alias(args):
    """The groups of argument positions (two or more) that hold the same non-null address."""
    at = {}
    for i, a in enumerate(args):
        if _address(a) is not None:
            at.setdefault(_address(a), []).append(i)
    return sorted(g for g in at.values() if len(g) > 1)


# ---- the fixed script ----------------------------------------------------------------------------------------------------------
def _problem(sol, seed=0):
    """B seeded systems with a cross term on one CSR pattern -> (the device CSR arrays and g as linsys_cross takes them, c)."""
    S, C, K, B = sol.S, sol.C, sol.K, sol.batch
    systems = [synth.make_system(S, C, K, seed=seed + b, dense_q=True, cross_scale=0.5) for b in range(B)]
    G_row, G_col, G_val, C_row, C_col, C_val, g, c = sol.upload_batch(systems)
    return (G_row, G_col, G_val, C_row, C_col, C_val, g), c


def _rand(sol, n, seed):
    return sol.to_device(np.random.default_rng(seed).standard_normal(n))


def _box(sol):
    """(lo, hi) [B N]: the states of x_0 free, every other state in [-2, 2] and every control in [-0.3, 0.3]."""
    S, n, N, B = sol.S, sol.n, sol.N, sol.batch
    hi = np.where(np.arange(N) % n < S, 2.0, 0.3)
    hi[:S] = np.inf
    hi = np.tile(hi, B)
    return sol.to_device(-hi), sol.to_device(hi)


def cross_and_tangents(S, C, K, B, R, dt):
    """The CSR and block cross solves, their re-solves, gradients and tangents, then the plain ones on the scattered blocks."""
    sol = Solver(S, C, K, dt, batch=B)
    N, sk, Gs, Cs, Ms = sol.N, sol.sizes["sk"], sol.sizes["G_dense"], sol.sizes["C_dense"], sol.M_size
    csr, c = _problem(sol)
    g = csr[6]
    lam, dz = sol.new(B * sk), sol.new(B * N)
    sol.linsys_cross(*csr, c, TOL, ITERS, RHO, lam, dz)
    sol.linsys_cross(*csr, c, TOL, ITERS, RHO)
    sol.cross_prepare_csr(*csr, RHO)
    Gb, Mb, Cb = sol.cross_prepare_csr(*csr, RHO, G_out=sol.new(B * Gs), M_out=sol.new(B * Ms), C_out=sol.new(B * Cs))
    pattern = csr[0], csr[1], csr[3], csr[4]
    sol.kkt_grad_csr_cross(*pattern, dz, lam, _rand(sol, B * N, 1), _rand(sol, B * sk, 2), Gbar_val=sol.new(csr[2].numel()),
                           Cbar_val=sol.new(csr[5].numel()))
    sol.kkt_grad_csr_cross(*pattern, dz, lam, _rand(sol, B * N, 1), _rand(sol, B * sk, 2), Gbar_val=sol.new(csr[2].numel()))
    Mk, Ck = (Mb, Cb) if K > 1 else (None, None)
    sol.linsys_blocks_cross(Gb, Mk, Ck, g, c, TOL, ITERS, RHO, lam, dz)
    sol.reserve_rhs(R)
    gR, cR = _rand(sol, B * R * N, 3), _rand(sol, B * R * sk, 4)
    sol.solve_rhs_cross(gR, cR, TOL, ITERS)
    sol.solve_rhs_cross(gR, cR, TOL, ITERS, sol.new(B * R * sk), sol.new(B * R * N), sol.new(B * R, torch.int32))
    sol.kkt_grad_cross(dz, _rand(sol, B * N, 5))
    sol.kkt_grad_cross(dz, _rand(sol, B * N, 5), sol.new(B * Ms))
    dots = dict(G_dot=_rand(sol, B * R * Gs, 6), g_dot=_rand(sol, B * R * N, 7), c_dot=_rand(sol, B * R * sk, 8))
    if K > 1:
        dots.update(M_dot=_rand(sol, B * R * Ms, 9), C_dot=_rand(sol, B * R * Cs, 10))
    sol.kkt_tangent_rhs_cross(R, dz, lam, **dots)
    sol.kkt_tangent_rhs_cross(R, dz, lam, tg=sol.new(B * R * N), gp=sol.new(B * R * N), tc=sol.new(B * R * sk), **dots)
    sol.kkt_tangent_rhs_cross(R, dz, lam, tg=sol.new(B * R * N), g_dot=dots["g_dot"])
    sol.kkt_tangent_rhs_cross(R, dz, lam, gp=sol.new(B * R * N), c_dot=dots["c_dot"])
    sol.tangents_cross(R, dz, lam, TOL, ITERS, **dots)
    sol.tangents_cross(1, dz, lam, TOL, ITERS, g_dot=_rand(sol, B * N, 22))
    sol.cross_prepare(Gb, Mk, Ck, g, RHO)
    sol.cross_rhs(gR)
    sol.cross_rhs(gR, sol.new(B * R * N))
    sol.cross_finish(sol.new(B * R * N).zero_())
    # the plain solve on the same blocks, its re-solve, gradients and tangents
    sol.linsys_blocks(Gb, Cb, g, c, TOL, ITERS, RHO, lam, dz)
    sol.linsys_blocks(Gb, Cb, g, c, TOL, ITERS, RHO)
    sol.solve_rhs(gR, cR, TOL, ITERS)
    sol.solve_rhs(gR, cR, TOL, ITERS, sol.new(B * R * sk), sol.new(B * R * N), sol.new(B * R, torch.int32))
    a, beta = _rand(sol, B * N, 11), _rand(sol, B * sk, 12)
    sol.kkt_grad_blocks(dz, lam, a, beta, sol.new(B * Gs), sol.new(B * Cs))
    sol.kkt_grad_blocks(dz, lam, a, beta, Gbar=sol.new(B * Gs))
    if K > 1:                                                # K = 1 has no C: the library refuses a call without an output
        sol.kkt_grad_blocks(dz, lam, a, beta, Cbar=sol.new(B * Cs))
    plain = {k: v for k, v in dots.items() if k != "M_dot"}
    sol.kkt_tangent_rhs(R, dz, lam, tg=sol.new(B * R * N), tc=sol.new(B * R * sk), **plain)
    sol.tangents(R, dz, lam, TOL, ITERS, **plain)
    sol.tangents(R, dz, lam, TOL, ITERS, c_dot=dots["c_dot"])
    sol.synchronize()
    sol.close()


def box_qps(S, C, K, B, R, dt):
    """Every box-QP method, the tangents of an active-set point and the three bound-gradient methods."""
    sol = Solver(S, C, K, dt, batch=B)
    N, sk, Gs, Cs, Ms = sol.N, sol.sizes["sk"], sol.sizes["G_dense"], sol.sizes["C_dense"], sol.M_size
    csr, c = _problem(sol)
    g = csr[6]
    Gb, Mb, Cb = sol.cross_prepare_csr(*csr, RHO, G_out=sol.new(B * Gs), M_out=sol.new(B * Ms), C_out=sol.new(B * Cs))
    lo, hi = _box(sol)
    qp = Gb, Cb, g, c, lo, hi
    pcg = dict(rho=RHO, exit_tol=TOL, max_iters=ITERS)
    r = sol.box_qp(*qp, max_admm_iters=ADMM_ITERS, **pcg)
    sol.box_qp(*qp, max_admm_iters=ADMM_ITERS, admm_rho=0.2, sigma=1e-5, alpha=1.5, eps_abs=1e-5, eps_rel=1e-4, check_every=10,
               x=sol.new(B * N), z=r.z, y=r.y, lam=r.lam, warm=True, **pcg)
    sol.box_qp_cross(Gb, Mb, Cb, g, c, lo, hi, max_admm_iters=ADMM_ITERS, **pcg)
    r = sol.box_qp(*qp, max_admm_iters=ADMM_ITERS, **pcg)
    act = sol.box_qp_active_set(r.z, r.y, lo, hi)
    sol.box_qp_active_set(r.z, r.y, lo, hi, sol.new(B * N, torch.int8))
    sol.box_qp_polish(*qp, act, r, eps_abs=1e-5, eps_rel=1e-4, **pcg)
    w = sol.to_device(np.full(B * N, 10.0))
    m = sol.to_device(np.full(B * N, 0.5))
    ph = sol.box_qp_pdas(*qp, max_pdas_iters=10, **pcg)
    sol.box_qp_pdas(*qp, max_pdas_iters=10, act=act, x=sol.new(B * N), z=sol.new(B * N), y=sol.new(B * N), lam=sol.new(B * sk),
                    eps_abs=1e-5, eps_rel=1e-4, **pcg)
    ps = sol.box_qp_pdas(*qp, max_pdas_iters=10, soft_weight=w, **pcg)
    sol.box_qp_pdas(*qp, max_pdas_iters=10, soft_weight=w, line_search=True, **pcg)
    sol.box_qp_pdas(*qp, max_pdas_iters=10, soft_weight=w, soft_cap=m, line_search=True, **pcg)
    p = sol.box_qp_pdas(*qp, max_pdas_iters=10, soft_weight=w, soft_cap=m, **pcg)
    dots = dict(G_dot=_rand(sol, B * R * Gs, 6), C_dot=_rand(sol, B * R * Cs, 10), g_dot=_rand(sol, B * R * N, 7),
                c_dot=_rand(sol, B * R * sk, 8), lo_dot=_rand(sol, B * R * N, 13), hi_dot=_rand(sol, B * R * N, 14),
                w_dot=_rand(sol, B * R * N, 15), m_dot=_rand(sol, B * R * N, 16))
    sol.tangents(R, p.x, p.lam, TOL, ITERS, Gb=Gb, Cb=Cb, act=p.act, soft_weight=w, soft_cap=m, lo=lo, hi=hi, **dots)
    sol.tangents(R, ps.x, ps.lam, TOL, ITERS, Gb=Gb, Cb=Cb, act=ps.act, soft_weight=w, lo=lo, hi=hi, g_dot=dots["g_dot"],
                 lo_dot=dots["lo_dot"])
    sol.tangents(R, ph.x, ph.lam, TOL, ITERS, Gb=Gb, Cb=Cb, act=ph.act, g_dot=dots["g_dot"], hi_dot=dots["hi_dot"])
    xbar, a, beta = _rand(sol, B * N, 17), _rand(sol, B * N, 18), _rand(sol, B * sk, 19)
    sol.box_qp_bound_grad(Gb, Cb, ph.act, xbar, a, beta)
    sol.box_qp_bound_grad(Gb, Cb, ph.act, xbar, a, beta, sol.new(B * N), sol.new(B * N))
    sol.box_qp_soft_grad(Gb, Cb, ps.act, w, lo, hi, ps.x, xbar, a, beta)
    sol.box_qp_soft_grad(Gb, Cb, ph.act, None, lo, hi, ph.x, xbar, a, beta, w_bar=sol.new(B * N))
    sol.box_qp_huber_grad(Gb, Cb, p.act, w, m, lo, hi, p.x, xbar, a, beta)
    sol.box_qp_huber_grad(Gb, Cb, ps.act, w, None, lo, hi, ps.x, xbar, a, beta, cap_bar=sol.new(B * N))
    xc, xplus = _rand(sol, B * N, 20), _rand(sol, B * N, 21)
    sol.box_qp_line_search(Gb, g, lo, hi, w, m, xc, xplus, rho=RHO)
    sol.box_qp_line_search(Gb, g, lo, hi, w, None, xc, xplus, rho=RHO, x=sol.new(B * N))
    r = sol.box_qp_alm(*qp, max_pdas_iters=10, max_alm_iters=5, **pcg)
    half = sol.to_device(np.tile(np.where(np.arange(N) % sol.n < S, 0.0, 10.0), B))
    sol.box_qp_alm(*qp, max_pdas_iters=10, max_alm_iters=5, alm_weight=50.0, alm_growth=5.0, alm_weight_max=1e6,
                   act=torch.zeros(B * N, dtype=torch.int8, device=g.device), mu=sol.new(B * N).zero_(), x=sol.new(B * N),
                   z=sol.new(B * N), y=sol.new(B * N), lam=sol.new(B * sk), soft_weight=half, soft_cap=m, eps_abs=1e-5, eps_rel=1e-4, **pcg)
    wB = torch.full((B,), 100.0, dtype=torch.float64, device=g.device)
    vB = torch.full((B,), float("inf"), dtype=torch.float64, device=g.device)
    sol.box_qp_alm_update(r.x, r.y, r.lam, sol.new(B * N).zero_(), wB, vB, lo, hi)
    sol.box_qp_alm_update(r.x, r.y, r.lam, sol.new(B * N).zero_(), wB, vB, lo, hi, eps_abs=1e-5, eps_rel=1e-4, alm_growth=5.0,
                          alm_weight_max=1e6, last=True, soft_weight=half, lo2=sol.new(B * N), hi2=sol.new(B * N), w2=sol.new(B * N),
                          z=sol.new(B * N))
    sol.synchronize()
    sol.close()


def record():
    """The trace of the whole script: {part: [call, ...]}."""
    real = _lib.lib()
    trace = {}
    parts = (("f64 cross and tangents 2/1/3", cross_and_tangents, (2, 1, 3, 2, 2, np.float64)),
             ("f64 box QPs 2/1/3", box_qps, (2, 1, 3, 2, 2, np.float64)),
             ("f64 cross and tangents 2/1/1", cross_and_tangents, (2, 1, 1, 2, 2, np.float64)),
             ("f32 cross and tangents 2/1/3", cross_and_tangents, (2, 1, 3, 2, 2, np.float32)),
             ("f32 box QPs 2/1/3", box_qps, (2, 1, 3, 2, 2, np.float32)))
    try:
        for name, part, args in parts:
            _lib._LIB = rec = Recorder(real)           # what _lib.lib() returns: the one private name this tool depends on
            part(*args)
            trace[name] = rec.calls
    finally:
        _lib._LIB = real
    return trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    trace = record()
    text = json.dumps(trace, indent=0, sort_keys=True)
    print({k: len(v) for k, v in trace.items()})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
