"""Cost of the box-constrained QP solve (Solver.box_qp): microseconds per ADMM iteration and per QP,
PCG iterations per ADMM iteration, and the outer loop users write today - a whole solve (Solver.linsys_blocks: assembly and
a cold PCG) plus the update in torch ops per iteration - on the same problems.  Boxes at half the unconstrained solution,
so that many bounds are active.  Prints one JSON line per case.
    python tools/box_qp_bench.py [--fixed 200] [--reps 5] [--out FILE]"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gato_python_amd import synth                      # noqa: E402
from gato_python_amd.solver import Solver              # noqa: E402
from oracle import gato_oracle as o                    # noqa: E402


def problem(S, C, K, B, dt, seed=500):
    """B systems (8 distinct ones repeated) with their boxes, on the device"""
    distinct = [synth.make_system(S, C, K, seed=seed + b) for b in range(min(B, 8))]
    systems = [distinct[b % len(distinct)] for b in range(B)]
    box = []
    for s in distinct:
        dz, _ = synth.dense_kkt_solve(s)
        w = 0.5 * np.abs(dz) + 0.05
        w[:S] = np.inf                                   # x_0 is pinned by c_0
        box.append(w)
    los, his = [-box[b % len(box)] for b in range(B)], [box[b % len(box)] for b in range(B)]
    sol = Solver(S, C, K, dt, batch=B)
    Gs, Cs = zip(*(o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, S, C, K, 0.0) for s in systems))
    cat = lambda arrs: sol.to_device(np.concatenate([np.asarray(a, np.float64) for a in arrs]).astype(dt))
    inp = (cat(Gs), cat(Cs), cat([s.g for s in systems]), cat([s.c for s in systems]), cat(los), cat(his))
    return sol, inp, systems[0].rho


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


def outer_loop(sol, inp, rho, kw, iters):
    """What a user writes today: per iteration a whole solve on G + diag(sigma + rho_i) (re-assembly, cold PCG), then the
    relaxation, projection and dual update in torch ops.  Returns ms per iteration and the PCG iterations of the last solve."""
    Gb, Cb, g, c, lo, hi = inp
    B, N, S, C, K = sol.batch, sol.N, sol.S, sol.C, sol.K
    sigma, alpha, arho = kw["sigma"], kw["alpha"], kw["admm_rho"]
    lo2, hi2 = lo.view(B, N), hi.view(B, N)
    free = torch.isinf(lo2) & torch.isinf(hi2)
    pen = torch.where(free, 0.0, torch.where(lo2 == hi2, 1e3 * arho, arho)).to(g.dtype)
    Gp = Gb.clone().view(B, -1)
    n, SS, CC = S + C, S * S, C * C
    for k in range(K):                                   # the diagonal of Q_k, R_k
        for i in range(S if k == K - 1 else n):
            off = k * (SS + CC) + (i * S + i if i < S else SS + (i - S) * C + (i - S))
            Gp[:, off] += sigma + pen[:, k * n + i]
    Gp = Gp.reshape(-1).contiguous()
    z = torch.zeros(B, N, dtype=g.dtype, device=g.device)
    x, y = z.clone(), z.clone()
    lam, dz = sol.new(B * S * K), sol.new(B * N)

    def step():
        nonlocal x, z, y
        gt = (g.view(B, N) + sigma * x + pen * z - y).reshape(-1).contiguous()
        sol.linsys_blocks(Gp, Cb, gt, c, kw["exit_tol"], kw["max_iters"], rho, lam, dz)
        xt = dz.view(B, N)
        xh = alpha * xt + (1 - alpha) * z
        x = alpha * xt + (1 - alpha) * x
        zn = torch.where(free, xh, torch.clamp(xh + y / torch.where(free, 1.0, pen), lo2, hi2))
        y = torch.where(free, 0.0, y + pen * (xh - zn))
        z = zn

    ms = wall(lambda: [step() for _ in range(iters)], 3) / iters
    return ms, device_int(sol.buffer_ptr(8))


def device_int(ptr):
    out = ct.c_int()
    torch.cuda.synchronize()
    if ct.CDLL("libamdhip64.so").hipMemcpy(ct.byref(out), ct.c_void_p(ptr), ct.c_size_t(4), 2) != 0:
        raise RuntimeError("hipMemcpy failed")
    return out.value


def case(S, C, K, B, dt, fixed, reps):
    sol, inp, rho = problem(S, C, K, B, dt)
    # admm_rho 10: the synthetic systems' scale (Q up to 1e3) converges slowly at the default 0.1
    kw = dict(exit_tol=1e-12 if dt == np.float64 else 1e-8, max_iters=500, admm_rho=10.0, sigma=1e-6, alpha=1.6)
    # fixed ADMM iterations (eps = 0): the cost per iteration; one live-count read at the end
    fix = dict(kw, eps_abs=0.0, eps_rel=0.0, max_admm_iters=fixed, check_every=fixed)
    fixed_ms = wall(lambda: sol.box_qp(*inp, rho=rho, **fix), reps)
    pcg_fixed = sol.box_qp_pcg_iters()
    # solves to eps = 1e-4, at most 2000 ADMM iterations (fixed rho: these synthetic boxes converge slowly)
    eps = 1e-4
    conv = dict(kw, eps_abs=eps, eps_rel=eps, max_admm_iters=2000)
    r = sol.box_qp(*inp, rho=rho, **conv)
    torch.cuda.synchronize()
    its = r.iters.cpu().numpy()
    pcg = sol.box_qp_pcg_iters()
    qp_ms = wall(lambda: sol.box_qp(*inp, rho=rho, **conv), reps)
    row = dict(case=f"{B} x {S}/{C}/{K} {np.dtype(dt).name}", us_per_admm_iter=fixed_ms * 1e3 / fixed, fixed_iters=fixed,
               pcg_per_admm_iter_fixed=float(pcg_fixed.mean()) / fixed, eps=eps, admm_iters_mean=float(its.mean()),
               admm_iters_max=int(its.max()), converged=int((r.status.cpu().numpy() == 0).sum()), us_per_qp=qp_ms * 1e3,
               pcg_per_admm_iter=float((pcg / np.maximum(its, 1)).mean()))
    return sol, inp, rho, kw, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixed", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for S, C, K, B, dt in ((14, 7, 50, 1, np.float64), (14, 7, 50, 512, np.float64), (14, 7, 512, 1, np.float32)):
        sol, inp, rho, kw, row = case(S, C, K, B, dt, a.fixed, a.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if B == 1 and dt == np.float64:
            # the same iteration as an outer loop over whole solves (cold PCG, re-assembly every iteration)
            its = 50
            ms, pcg_cold = outer_loop(sol, inp, rho, kw, its)
            row = dict(case=f"outer loop of linsys_blocks, {B} x {S}/{C}/{K} {np.dtype(dt).name}", us_per_admm_iter=ms * 1e3,
                       iters=its, pcg_iters_cold_last_solve=pcg_cold,
                       outer_over_box_qp=ms * 1e3 / rows[-1]["us_per_admm_iter"])
            rows.append(row)
            print(json.dumps(row), flush=True)
        sol.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
