"""gato_python_amd - MI355X-native PCG / Schur-complement KKT solve (the hot path of gato-python).

Public surface:
  gato_python_amd.linsys_solve(...)      drop-in for gpu_library.linsys_solve (gpu_library.cu:236-239)
  gato_python_amd.linsys_resolve(...)    the last linsys_solve's system again, for a new g / c (no re-assembly)
  gato_python_amd.Solver                 device-resident stage-level API over include/gato_hip.h
  gato_python_amd.kkt_solve(...)         differentiable solve from math-shaped blocks (torch autograd, autograd.py)
  gato_python_amd.kkt_solve(..., M=M)    the same with a state-control cross term x_k^T M_k u_k in the stage cost
  gato_python_amd.kkt_solve_csr(...)     differentiable solve on device CSR input
  gato_python_amd.kkt_solve_csr(..., cross=True)   the same for a G whose state rows hold control columns: the cross term read
                                         from the CSR itself; without it such entries are dropped
  gato_python_amd.box_qp(...)            box-constrained QP (bounds on states and controls) by ADMM over the re-solve, or
                                         by the active-set iteration (method="pdas": hard, soft and capped soft bounds;
                                         line_search=True: the exact line search that makes the all-soft iteration converge),
                                         or by the method of multipliers over that iteration (method="alm": hard bounds on
                                         states too, where ADMM is slow and the hard active-set iteration cycles)
  gato_python_amd.box_qp(..., M=M)       the ADMM solve with the cross term x_k^T M_k u_k in the stage cost
  gato_python_amd.box_qp_layer(...)      differentiable box-constrained QP: ADMM, then the polish on its active set, or the
                                         active-set iteration alone, with hard or soft bounds (one autograd Function,
                                         qp._BoxQPLayer, whose backward branches on "weights present"); line_search=True
                                         changes the forward pass only
  gato_python_amd.kkt_solve_tangents(...)      kkt_solve and its forward-mode sensitivities along R directions (one re-solve);
                                         M=M: with the cross term, a tangent named "M" included
  gato_python_amd.box_qp_layer_tangents(...)   box_qp_layer and its forward-mode sensitivities; both also take
                                         torch.autograd.forward_ad dual tensors (one direction per pass)
  gato_python_amd.synth                  synthetic OCP inputs (the reference ships pendulum data only)
"""
from .linsys import (clear_problem_size, last_stats, linsys_resolve, linsys_solve, set_precision,  # noqa: F401
                     set_problem_size)


def __getattr__(name):
    if name == "Solver":              # torch import deferred: linsys_solve itself needs only ctypes
        from .solver import Solver
        return Solver
    if name in ("kkt_solve", "kkt_solve_csr", "kkt_solve_tangents"):
        from . import autograd
        return getattr(autograd, name)
    if name in ("box_qp", "box_qp_layer", "box_qp_layer_tangents"):
        from . import qp
        return getattr(qp, name)
    raise AttributeError(name)
