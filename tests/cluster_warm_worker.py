"""Worker of tests/test_gpu_cluster.py::test_cluster_warm_started_solves_one_process_per_rank: one rank of a cluster, one PROCESS
per rank, all on cuda:0.  Three whole solves through linsys_solve_cluster with true_warm_start on ONE state, a new system of the
same pattern each time: the first from zero (a fresh state: the connect probe's lambda must not be its guess), the next ones from
the previous gathered lambda - each rank reads its own rows of its own buffer only."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gato_python_amd import synth                                       # noqa: E402
from gato_python_amd.dist import close_state, linsys_solve_cluster      # noqa: E402
from oracle import gato_oracle as o                                     # noqa: E402


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def main():
    S, C, K = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    tol, mi = 1e-9, 150
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    state, prev = None, None
    for call in range(3):
        s = synth.make_system(S, C, K, seed=70 + call)
        lam, dz, its, state = linsys_solve_cluster(s, tol, mi, np.float64, 0, None, state,
                                                   solver_options={"true_warm_start": 1})
        lam, dz, it = lam.cpu().numpy().copy(), dz.cpu().numpy().copy(), int(its.cpu()[0])
        lam_o, dz_o, it_o = o.linsys_solve(*s.csr_args(), S, C, K, tol, mi, s.rho, dtype=np.float64, lam0=prev)
        assert it == it_o, (rank, call, it, it_o)
        assert rel(lam, lam_o) < 1e-8 and rel(dz, dz_o) < 1e-8, (rank, call, rel(lam, lam_o), rel(dz, dz_o))
        prev = lam
    close_state(state)
    dist.destroy_process_group()
    print(f"rank {rank}/{world} warm ok iters={it}")


if __name__ == "__main__":
    main()
