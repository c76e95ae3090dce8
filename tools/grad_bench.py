"""Device time of the differentiable solve (gato_python_amd.kkt_solve): forward, backward, and the stages the backward is
made of - the adjoint re-solve (Solver.solve_rhs) and the gradient kernel (gato_kkt_grad_blocks) - beside the whole solve.
Fixed iteration counts (exit_tol = 0) so that forward and adjoint run the same PCG work.  Prints one JSON line per case.
    python tools/grad_bench.py [--iters 30] [--reps 50] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gato_python_amd import autograd, synth            # noqa: E402


def timed(fn, reps):
    """median device time (ms) of fn() between two events, after warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def case(S, C, K, B, dt, it, reps):
    tdt = torch.float64 if dt == np.float64 else torch.float32
    per = [synth.make_blocks(S, C, K, seed=300 + b) for b in range(B)]
    blocks = [torch.tensor(np.stack([p[i] for p in per]), dtype=tdt, device="cuda:0", requires_grad=True) for i in range(7)]
    kw = dict(rho=1e-3, exit_tol=0.0, max_iters=it)
    rng = np.random.default_rng(0)
    N = (S + C) * K - C
    w1 = torch.tensor(rng.standard_normal((B, N)), dtype=tdt, device="cuda:0")
    w2 = torch.tensor(rng.standard_normal((B, S * K)), dtype=tdt, device="cuda:0")

    def fwd():
        return autograd.kkt_solve(*blocks, **kw)
    fwd_ms = timed(fwd, reps)
    lam, dz = fwd()
    L = (dz * w1).sum() + (lam * w2).sum()
    bwd_ms = timed(lambda: L.backward(retain_graph=True), reps)
    # the stages on the cached solver, on the packed inputs the forward used
    sol = autograd._SOLVERS[(S, C, K, B, tdt, 0)]
    Gb, Cb, g, c = autograd._pack(*[b.detach() for b in blocks])
    lam_o, dz_o = sol.new(B * S * K), sol.new(B * N)
    solve_ms = timed(lambda: sol.linsys_blocks(Gb, Cb, g, c, 0.0, it, 1e-3, lam_o, dz_o), reps)
    out = sol.new(B * S * K), sol.new(B * N), sol.new(B, torch.int32)
    resolve_ms = timed(lambda: sol.solve_rhs(w1.reshape(-1), w2.reshape(-1), 0.0, it, *out), reps)
    Gbar, Cbar = torch.empty_like(Gb), torch.empty_like(Cb)
    grad_ms = timed(lambda: sol.kkt_grad_blocks(dz_o, lam_o, out[1], out[0], Gbar, Cbar), reps)
    out_bytes = (Gbar.numel() + Cbar.numel()) * Gbar.element_size()
    return dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", forward_ms=fwd_ms, backward_ms=bwd_ms, solve_ms=solve_ms,
                resolve_ms=resolve_ms, grad_kernel_ms=grad_ms, grad_out_bytes=out_bytes,
                grad_kernel_tbps=out_bytes / (grad_ms * 1e-3) / 1e12, backward_over_solve=bwd_ms / solve_ms)


def csr_case(S, C, K, B, dt, it, reps):
    """gato_kkt_grad_csr over a shared pattern (the CSR form of kkt_solve_csr) beside the block kernel on the same vectors."""
    from gato_python_amd.solver import Solver
    systems = [synth.make_system(S, C, K, seed=400 + b) for b in range(B)]
    sol = Solver(S, C, K, dt, batch=B)
    d = sol.upload_batch(systems)
    N = sol.N
    lam, dz, its = sol.new(B * S * K), sol.new(B * N), sol.new(B, torch.int32)
    sol.linsys_batched(*d, 0.0, it, systems[0].rho, lam, dz, its)
    beta, a, _ = sol.solve_rhs(d[6], d[7], 0.0, it)
    Gv, Cv = torch.empty_like(d[2]), torch.empty_like(d[5])
    csr_ms = timed(lambda: sol.kkt_grad_csr(d[0], d[1], d[3], d[4], dz, lam, a, beta, Gv, Cv), reps)
    Gb, Cb = sol.new(B * sol.sizes["G_dense"]), sol.new(B * sol.sizes["C_dense"])
    blk_ms = timed(lambda: sol.kkt_grad_blocks(dz, lam, a, beta, Gb, Cb), reps)
    out_bytes = (Gv.numel() + Cv.numel()) * Gv.element_size()
    blk_bytes = (Gb.numel() + Cb.numel()) * Gb.element_size()
    sol.close()
    return dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name} CSR", grad_csr_ms=csr_ms, grad_csr_out_bytes=out_bytes,
                grad_csr_tbps=out_bytes / (csr_ms * 1e-3) / 1e12, grad_blocks_ms=blk_ms, grad_blocks_out_bytes=blk_bytes,
                grad_blocks_tbps=blk_bytes / (blk_ms * 1e-3) / 1e12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = [case(14, 7, 50, 1, np.float64, a.iters, a.reps), case(14, 7, 50, 512, np.float64, a.iters, a.reps),
            case(14, 7, 4096, 1, np.float32, a.iters, a.reps), csr_case(14, 7, 50, 512, np.float64, a.iters, a.reps)]
    for r in rows:
        r["pcg_iters"] = a.iters
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
