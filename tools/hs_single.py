"""Where the one-workgroup fp64 launch (pcg_single_f64m_kernel, 14/7/50) spends its time OUTSIDE the loop: s_memrealtime stamps
(100 MHz) of the solving workgroup's thread 0 and of the helper wave that does knot 0's dz.

Needs a SCRATCH build (a copy of csrc/ outside the tree, built as another .so and selected with GATO_HIP_LIB; not committed):
__builtin_amdgcn_s_memrealtime() of thread 0 of the solving workgroup, kept in registers until the kernel's end (a store in
between would count in the loads' vmcnt waits) and then written as doubles to eta_hist[2000 + i]:
    0 kernel entry                           1 in front of the set-up barrier (own loads landed)   2 behind it
    3 behind the first block sum             4 behind the barrier in front of the loop             5 loop left
    6 behind the flag store
and of lane 0 of the helper wave with kq == 0 in one_system_helper: [2007] behind the poll of the flag, [2008] behind its dz
stores and an s_waitcnt vmcnt(0).
    GATO_HIP_LIB=/path/to/libgato_hs.so python tools/hs_single.py [launches=30]
Prints, per phase, the median and the range over the launches, in microseconds."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402
from gato_python_amd import synth                      # noqa: E402
from gato_python_amd.solver import Solver              # noqa: E402

S, C, K, ITERS = 14, 7, 50, 100
n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
s = synth.make_system(S, C, K, seed=0)
sol = Solver(S, C, K, np.float64)
sol.set_option("record_eta", 1)
dev = sol.upload_system(s)
lam, dz = sol.new(S * K), sol.new(sol.N)
rows = []
for i in range(n + 5):
    sol.linsys(*dev, 0.0, ITERS, s.rho, lam, dz)
    torch.cuda.synchronize()
    if i >= 5:
        rows.append(sol.eta_history(2010)[2000:2009].copy())
sol.check_status()
sol.close()
t = np.array(rows) / 100.0                              # us
names = [("entry -> own loads of gamma and Pinv landed", 0, 1), ("-> set-up barrier passed", 1, 2),
         ("-> first product and block sum done", 2, 3), ("-> loop entered (all of S landed)", 3, 4),
         ("loop, %d iterations" % ITERS, 4, 5), ("loop left -> lambda stored and flag stored", 5, 6),
         ("flag stored -> seen by knot 0's helper wave", 6, 7), ("-> that wave's dz stored", 7, 8),
         ("OUTSIDE the loop: entry -> loop entered", 0, 4), ("OUTSIDE the loop: loop left -> dz stored", 5, 8),
         ("entry -> dz stored", 0, 8)]
print("library", os.environ.get("GATO_HIP_LIB", "(the package's own)"), "-", n, "launches")
for name, a, b in names:
    d = t[:, b] - t[:, a]
    print(f"  {name:52s} median {np.median(d):7.2f}   min {d.min():7.2f}   max {d.max():7.2f}")
