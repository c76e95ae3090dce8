"""ctypes binding of libgato_hip.so (include/gato_hip.h).

The HIP library IS the product path: if it is missing this module raises, there is no CPU
fallback anywhere in gato_python_amd (the oracle under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("GATO_HIP_LIB") or os.path.join(_HERE, "libgato_hip.so")   # override: A/B builds only
_LIB = None

GATO_F32, GATO_F64 = 0, 1
PCG_AUTO, PCG_RESIDENT, PCG_STREAMING = 0, 1, 2
PRECON_STAIR, PRECON_BLOCK_JACOBI, PRECON_POINT_JACOBI = 0, 1, 2

ERRORS = {-1: "EINVAL", -2: "ESHAPE", -3: "EHIP", -4: "ENODEV", -5: "ETIMEOUT"}

# Every symbol include/gato_hip.h declares (tests check the .so exports all of them).
SYMBOLS = [
    "gato_last_error", "gato_version", "gato_num_shapes", "gato_shape", "gato_device_info",
    "gato_infer_shape", "gato_solver_create", "gato_solver_create_batched", "gato_linsys_device_batched",
    "gato_solver_destroy", "gato_solver_buffer",
    "gato_solver_set_option", "gato_solver_get_option", "gato_convert", "gato_form_schur",
    "gato_form_ss", "gato_pcg", "gato_pcg_status", "gato_pcg_last_ms", "gato_compute_dz", "gato_linsys_device",
    "gato_linsys_solve_f32", "gato_linsys_solve_f64",
    "gato_shard_pcg_init", "gato_shard_pcg_phase_a", "gato_shard_pcg_phase_b", "gato_shard_pcg_finish",
    "gato_shard_pcg_done", "gato_linsys_device_blocks", "gato_release_cache", "gato_solver_recover",
    "gato_cluster_knot_range", "gato_cluster_create", "gato_cluster_local_mirror", "gato_cluster_connect",
    "gato_cluster_pcg", "gato_cluster_linsys", "gato_cluster_destroy", "gato_cluster_launches_left", "gato_cluster_rewind", "gato_cluster_fits", "gato_last_stage_ms", "gato_solver_tune",
    "gato_solver_reserve_rhs", "gato_solve_rhs", "gato_linsys_resolve_f32", "gato_linsys_resolve_f64",
    "gato_kkt_grad_blocks", "gato_kkt_grad_csr", "gato_box_qp_default_params", "gato_box_qp_solve",
    "gato_box_qp_active_set", "gato_box_qp_polish", "gato_box_qp_bound_grad", "gato_box_qp_pdas",
    "gato_box_qp_pdas_soft", "gato_box_qp_soft_grad", "gato_box_qp_pdas_huber", "gato_box_qp_huber_grad",
    "gato_box_qp_pdas_ls", "gato_box_qp_line_search", "gato_kkt_tangent_rhs", "gato_box_qp_alm", "gato_box_qp_alm_update",
    "gato_linsys_device_blocks_cross", "gato_solve_rhs_cross", "gato_kkt_grad_cross", "gato_cross_prepare", "gato_cross_rhs",
    "gato_cross_finish", "gato_box_qp_solve_cross", "gato_kkt_tangent_rhs_cross",
    "gato_cross_prepare_csr", "gato_linsys_device_cross", "gato_kkt_grad_csr_cross",
]


QP_CONVERGED, QP_MAX_ITERS, QP_NONFINITE, QP_BAD_BOUNDS, QP_BAD_ACTIVE = 0, 1, 2, 3, 4
ALM_ACCEPT, ALM_GROW, ALM_KEEP, ALM_LAST, ALM_INNER = 0, 1, 2, 3, 4      # Solver.box_qp_alm_update's decisions
POLISH_ACCEPTED, POLISH_REJECTED, POLISH_NONFINITE, POLISH_BAD_ACTIVE = 0, 1, 2, 3


class BoxQpParams(ct.Structure):
    """gato_box_qp_params (include/gato_hip.h)."""
    _fields_ = [("rho", ct.c_double), ("admm_rho", ct.c_double), ("sigma", ct.c_double), ("alpha", ct.c_double),
                ("eps_abs", ct.c_double), ("eps_rel", ct.c_double), ("exit_tol", ct.c_double), ("max_iters", ct.c_int),
                ("max_admm_iters", ct.c_int), ("check_every", ct.c_int), ("warm", ct.c_int)]


class GatoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libgato_hip: {ERRORS.get(code, code)}: {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(SO_PATH):
        cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4", "-s"] + (["-B"] if force else [])
        subprocess.check_call(cmd)
    return SO_PATH


def lib() -> ct.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH) and "GATO_HIP_LIB" not in os.environ:
            try:                       # source tree without the built library: compile it (hipcc; a clean build of all shapes is ~3 min at -j8, ~6 CPU-minutes); no fallback
                build()
            except Exception as e:     # noqa: BLE001
                raise ImportError(f"{SO_PATH} is missing and building it failed: {e}") from e
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gato_python_amd/csrc`.  There is no CPU fallback.")
        L = ct.CDLL(SO_PATH)
        L.gato_last_error.restype = ct.c_char_p
        L.gato_solver_buffer.restype = ct.c_void_p
        vp, ip, i, d = ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_double
        L.gato_solver_create.argtypes = [i, i, i, i, i, ct.POINTER(ct.c_void_p)]
        L.gato_solver_create_batched.argtypes = [i, i, i, i, i, i, ct.POINTER(ct.c_void_p)]
        L.gato_linsys_device_batched.argtypes = [vp, ip, ip, vp, i, ip, ip, vp, i, vp, vp, d, i, d, vp, vp, vp, vp]
        L.gato_solver_destroy.argtypes = [vp]
        L.gato_solver_buffer.argtypes = [vp, i]
        L.gato_solver_set_option.argtypes = [vp, ct.c_char_p, i]
        L.gato_solver_get_option.argtypes = [vp, ct.c_char_p, ct.POINTER(ct.c_int)]
        L.gato_convert.argtypes = [vp, ip, ip, vp, ip, ip, vp, d, vp, vp, vp]
        L.gato_form_schur.argtypes = [vp] * 10
        L.gato_form_ss.argtypes = [vp, vp, vp, vp]
        L.gato_pcg.argtypes = [vp, vp, vp, vp, vp, d, i, vp, vp]
        L.gato_pcg_status.argtypes = [vp, ct.POINTER(ct.c_int)]
        L.gato_pcg_last_ms.argtypes = [vp, ct.POINTER(ct.c_float)]
        L.gato_last_stage_ms.argtypes = [vp, ct.POINTER(ct.c_float)]
        L.gato_compute_dz.argtypes = [vp] * 7
        L.gato_linsys_device.argtypes = [vp, ip, ip, vp, ip, ip, vp, vp, vp, d, i, d, vp, vp, vp]
        L.gato_infer_shape.argtypes = [ip, i, i, i] + [ct.POINTER(ct.c_int)] * 3
        L.gato_device_info.argtypes = [i, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int), ct.c_char_p, i]
        L.gato_shard_pcg_init.argtypes = [vp, i, i, i, i, vp, vp, vp, d, i, vp, vp]
        L.gato_shard_pcg_phase_a.argtypes = [vp, i, vp, vp, vp, vp]
        L.gato_shard_pcg_phase_b.argtypes = [vp, i, vp, vp, vp, vp]
        L.gato_shard_pcg_finish.argtypes = [vp, vp, vp, vp, vp]
        L.gato_shard_pcg_done.argtypes = [vp, ct.POINTER(ct.c_int), vp]
        L.gato_linsys_device_blocks.argtypes = [vp, vp, vp, vp, vp, d, i, d, vp, vp, vp]
        L.gato_solver_recover.argtypes = [vp, ct.POINTER(ct.c_int), vp]
        L.gato_cluster_knot_range.argtypes = [i, i, i, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)]
        L.gato_cluster_create.argtypes = [vp, i, i, vp]
        L.gato_cluster_local_mirror.argtypes = [vp]
        L.gato_cluster_local_mirror.restype = ct.c_void_p
        L.gato_cluster_connect.argtypes = [vp, vp, vp]
        L.gato_cluster_pcg.argtypes = [vp, vp, vp, vp, vp, d, i, vp, vp]
        L.gato_cluster_linsys.argtypes = [vp, ip, ip, vp, ip, ip, vp, vp, vp, d, i, d, vp, vp, vp, vp]
        L.gato_cluster_destroy.argtypes = [vp]
        L.gato_cluster_launches_left.argtypes = [vp, i, ct.POINTER(ct.c_longlong)]
        L.gato_cluster_rewind.argtypes = [vp]
        L.gato_cluster_fits.argtypes = [vp, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)]
        L.gato_solver_tune.argtypes = [vp, vp]
        L.gato_solver_reserve_rhs.argtypes = [vp, i]
        L.gato_solve_rhs.argtypes = [vp, i, vp, vp, d, i, vp, vp, vp, vp]
        L.gato_kkt_grad_blocks.argtypes = [vp] * 8
        L.gato_kkt_grad_csr.argtypes = [vp, ip, ip, i, ip, ip, i, vp, vp, vp, vp, vp, vp, vp]
        L.gato_box_qp_default_params.argtypes = [ct.POINTER(BoxQpParams)]
        L.gato_box_qp_default_params.restype = None
        L.gato_box_qp_solve.argtypes = [vp] * 7 + [ct.POINTER(BoxQpParams)] + [vp] * 8
        L.gato_box_qp_active_set.argtypes = [vp] * 7
        L.gato_box_qp_polish.argtypes = [vp] * 8 + [ct.POINTER(BoxQpParams)] + [vp] * 8
        L.gato_box_qp_bound_grad.argtypes = [vp] * 10
        L.gato_box_qp_pdas.argtypes = [vp] * 8 + [ct.POINTER(BoxQpParams), i] + [vp] * 8
        L.gato_box_qp_pdas_soft.argtypes = [vp] * 9 + [ct.POINTER(BoxQpParams), i] + [vp] * 8
        L.gato_box_qp_soft_grad.argtypes = [vp] * 15
        L.gato_box_qp_pdas_huber.argtypes = [vp] * 10 + [ct.POINTER(BoxQpParams), i] + [vp] * 8
        L.gato_box_qp_huber_grad.argtypes = [vp] * 17
        L.gato_box_qp_pdas_ls.argtypes = [vp] * 10 + [ct.POINTER(BoxQpParams), i] + [vp] * 9
        L.gato_box_qp_line_search.argtypes = [vp] * 7 + [d] + [vp] * 6
        L.gato_kkt_tangent_rhs.argtypes = [vp, i] + [vp] * 20
        L.gato_box_qp_alm.argtypes = [vp] * 10 + [ct.POINTER(BoxQpParams), i, d, d, d, i] + [vp] * 11
        L.gato_box_qp_alm_update.argtypes = [vp] * 10 + [d, d, d, d, i] + [vp] * 8
        L.gato_linsys_device_blocks_cross.argtypes = [vp, vp, vp, vp, vp, vp, d, i, d, vp, vp, vp]
        L.gato_solve_rhs_cross.argtypes = [vp, i, vp, vp, d, i, vp, vp, vp, vp]
        L.gato_kkt_grad_cross.argtypes = [vp] * 5
        L.gato_cross_prepare.argtypes = [vp, vp, vp, vp, vp, d, vp]
        L.gato_cross_rhs.argtypes = [vp, i, vp, vp, vp]
        L.gato_cross_finish.argtypes = [vp, i, vp, vp]
        L.gato_box_qp_solve_cross.argtypes = [vp] * 8 + [ct.POINTER(BoxQpParams)] + [vp] * 8
        L.gato_kkt_tangent_rhs_cross.argtypes = [vp, i] + [vp] * 11
        L.gato_cross_prepare_csr.argtypes = [vp, ip, ip, vp, i, ip, ip, vp, i, vp, d, vp, vp, vp, vp]
        L.gato_linsys_device_cross.argtypes = [vp, ip, ip, vp, i, ip, ip, vp, i, vp, vp, d, i, d, vp, vp, vp]
        L.gato_kkt_grad_csr_cross.argtypes = [vp, ip, ip, i, ip, ip, i, vp, vp, vp, vp, vp, vp, vp]
        f = ct.c_float
        L.gato_linsys_solve_f32.argtypes = [ip, i, ip, vp, i, ip, i, ip, vp, i, vp, i, vp, i, vp,
                                            i, i, i, i, f, i, i, f, vp, vp, vp, vp]
        L.gato_linsys_solve_f64.argtypes = [ip, i, ip, vp, i, ip, i, ip, vp, i, vp, i, vp, i, vp,
                                            i, i, i, i, d, i, i, d, vp, vp, vp, vp]
        L.gato_linsys_resolve_f32.argtypes = [vp, i, vp, i, f, i, vp, vp, vp]
        L.gato_linsys_resolve_f64.argtypes = [vp, i, vp, i, d, i, vp, vp, vp]
        _LIB = L
    return _LIB


def check(rc: int):
    if rc != 0:
        raise GatoError(rc, lib().gato_last_error().decode())


def shapes():
    L = lib()
    out = []
    for k in range(L.gato_num_shapes()):
        s, c = ct.c_int(), ct.c_int()
        L.gato_shape(k, ct.byref(s), ct.byref(c))
        out.append((s.value, c.value))
    return out
