"""Device-resident solver object over the C ABI (include/gato_hip.h).

Mirrors the reference's per-solve driver gato_linsys (gpu_library.cu:25-83) and the three
launch wrappers it calls - form_schur (src/gato_schur.cuh:885-1009), solve_pcg
(src/gato_pcg.cuh:476-567), compute_dz (src/gato_schur.cuh:1012-1022) - with the same stage
names, on device buffers.  torch is used only to hold device memory and name the stream.
"""
from __future__ import annotations

import ctypes as ct
import functools

import numpy as np
import torch

from . import _lib

_TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
# alm_weight_max=None of Solver.box_qp_alm (DESIGN.md section 3.14 says how the float32 value was chosen)
ALM_WEIGHT_MAX = {np.dtype(np.float64): 1e8, np.dtype(np.float32): 1e5}


class BoxQPResult:
    """Result of a box-constrained QP solve: x, z, y [.., N], lam [.., S K], iters, status [..] (int32: _lib.QP_*),
    res_prim, res_dual [..] (float64) - the true QP residuals of the returned iterate - and polished [..] (int32:
    _lib.POLISH_*; None unless a polish was asked for); act [.., N] (int8) the final active set of an active-set solve
    (box_qp_pdas; None otherwise); alpha [.., max_pdas_iters] (float64) the step length of every reduced solve of an
    active-set solve with line_search=True (None otherwise); outer [..] (int32) and weight [..] (float64) the outer steps and
    the last step's weight of an augmented-Lagrangian solve (box_qp_alm; None otherwise)."""
    __slots__ = ("x", "z", "y", "lam", "iters", "status", "res_prim", "res_dual", "polished", "act", "alpha", "outer", "weight")

    def __init__(self, x, z, y, lam, iters, status, res_prim, res_dual, polished=None, act=None, alpha=None, outer=None,
                 weight=None):
        self.x, self.z, self.y, self.lam = x, z, y, lam
        self.iters, self.status, self.res_prim, self.res_dual = iters, status, res_prim, res_dual
        self.polished, self.act, self.alpha, self.outer, self.weight = polished, act, alpha, outer, weight

    def __repr__(self):
        pol = "" if self.polished is None else f", polished={self.polished.tolist()}"
        return (f"BoxQPResult(iters={self.iters.tolist()}, status={self.status.tolist()}, "
                f"res_prim={self.res_prim.tolist()}, res_dual={self.res_dual.tolist()}{pol})")


def operand_sizes(S, C, K):
    """Entries per system of every layout an operand can have: the blocks G_dense, C_dense and M (the cross term's), the
    block-tridiagonal bd, and the vectors N (dz's layout) and sk (lambda's)."""
    return dict(G_dense=(S * S + C * C) * K - C * C, C_dense=(S * S + S * C) * (K - 1), M=(K - 1) * S * C, bd=3 * S * S * K,
                sk=S * K, N=(S + C) * K - C)


# dtype kind -> (torch dtype, its name in a message); "value": the solver's own dtype, "index": a CSR index array
_KINDS = dict(int8=(torch.int8, "torch.int8"), int32=(torch.int32, "torch.int32"), index=(torch.int32, "int32"),
              float64=(torch.float64, "float64"))
# The one operand table: name -> (key of operand_sizes: the entries per system, None: one; dtype kind), for every operand a
# Solver method takes by that name.  The CSR arrays have no size here: their callers state it (check_operands' entries).
OPERANDS = {name: (key, kind) for key, kind, names in (
    ("G_dense", "value", "Gb G_blocks G_dot G_out Gbar"), ("C_dense", "value", "Cb C_blocks C_dot C_out Cbar"),
    ("M", "value", "Mb M_blocks M_dot M_out Mbar"), ("sk", "value", "c lam beta alam c_dot tc"),
    ("N", "value", "g x z y lo hi dz adz a xbar gp tg g_dot lo_dot hi_dot w_dot m_dot soft_weight soft_cap mu xc xplus lo2 hi2 w2 "
                   "lo_bar hi_bar w_bar cap_bar"),
    ("N", "int8", "act"), (None, "int32", "status iters"), (None, "float64", "w v_prev"), (None, "value", "G_val C_val"),
    (None, "index", "G_row G_col C_row C_col")) for name in names.split()}


def operand_table(sizes, batch, dtype):
    """OPERANDS resolved for `batch` systems of operand_sizes `sizes` and the value dtype `dtype`: name -> (entries per right-hand
    side or direction, torch dtype, the dtype's name in a message)."""
    return {name: (batch * (sizes[key] if key else 1), *((dtype, str(dtype)) if kind == "value" else _KINDS[kind]))
            for name, (key, kind) in OPERANDS.items()}


def check_operands(table, what, operands, R=1, entries=None, got=True, optional=False):
    """ValueError in the name of the method `what` unless every operand of the dict `operands` (name -> tensor) is a contiguous CUDA
    tensor of the dtype and of R times the entries that `table` (an operand_table) has for it.  entries: name -> the count of an
    operand whose size the table cannot know (nnz; None: any, at least one).  optional: an operand that is None is skipped.
    got=False: the message does not say what was given."""
    for name, t in operands.items():
        if t is None and optional:
            continue
        n, dt, text = table[name]
        n = entries[name] if entries and name in entries else n * R
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or not t.is_contiguous() or \
                (t.numel() < 1 if n is None else t.numel() != n):
            given = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} must be a contiguous {text} CUDA tensor{'' if n is None else ' of %d entries' % n}"
                             + (f", got {given}" if got else ""))


def zero_rhs(g, c):
    """The re-solve's zero rule: the mask [...] of the right-hand sides (g [..., N], c [..., S K]) that are all zero.  Such a
    system's solution is zero, and its PCG would form 0/0 (eta / p.Sp): every caller of a re-solve writes zeros there."""
    return ~(g.ne(0).any(-1) | c.ne(0).any(-1))


def hard_active(act, w=None):
    """The hard-active rule: the mask of the variables that sit on a hard bound - act != 0 and no positive soft weight w.  The
    reduced system does not read a right-hand side there (Ginv' has zero rows), so it is masked before zero_rhs."""
    return act != 0 if w is None else (act != 0) & ~(w > 0)


def bound_tangents(x_d, act, hard, lo_dot=None, hi_dot=None):
    """x_d with the tangent of the bound a variable sits on (hi_dot where act > 0, lo_dot elsewhere; None: zero) on the
    hard-active set: such a variable moves with its bound."""
    z = torch.zeros((), dtype=x_d.dtype, device=x_d.device)
    return torch.where(hard, torch.where(act > 0, z if hi_dot is None else hi_dot, z if lo_dot is None else lo_dot), x_d)


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_cuda and t.is_contiguous()
        return ct.c_void_p(t.data_ptr())
    return ct.c_void_p(int(t))


def _given(**operands):
    """The operands that are not None, by name."""
    return {name: t for name, t in operands.items() if t is not None}


class Solver:
    """Workspace + kernels for one (STATE_SIZE, CONTROL_SIZE, KNOT_POINTS, dtype) on one GPU."""

    def __init__(self, S: int, C: int, K: int, dtype=np.float32, device: int = 0, batch: int = 1):
        self.S, self.C, self.K = int(S), int(C), int(K)
        self.batch = int(batch)
        self.np_dtype = np.dtype(dtype)
        self.dtype = _TORCH_DT[self.np_dtype]
        self.device = int(device)
        self._h = ct.c_void_p()
        code = _lib.GATO_F32 if self.np_dtype == np.float32 else _lib.GATO_F64
        _lib.check(_lib.lib().gato_solver_create_batched(self.S, self.C, self.K, self.batch, code, self.device,
                                                         ct.byref(self._h)))
        self.n = self.S + self.C
        self.N = self.n * self.K - self.C
        self.sizes = operand_sizes(self.S, self.C, self.K)
        self._operands = operand_table(self.sizes, self.batch, self.dtype)
        self._check = functools.partial(check_operands, self._operands)      # _check(what, {name: tensor}, R=1, ...)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().gato_solver_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- options -------------------------------------------------------------------------
    def set_option(self, name: str, value: int):
        _lib.check(_lib.lib().gato_solver_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ct.c_int()
        _lib.check(_lib.lib().gato_solver_get_option(self._h, name.encode(), ct.byref(v)))
        return v.value

    def tune(self):
        """Measure the hosting XCD of the one-XCD launches for the geometry the CURRENT options plan (blocking, ~1 ms;
        gato_solver_tune).  The constructor did it for the default geometry."""
        _lib.check(_lib.lib().gato_solver_tune(self._h, self._stream()))

    def _stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    def new(self, n, dtype=None):
        return torch.empty(int(n), dtype=dtype or self.dtype, device=f"cuda:{self.device}")

    def to_device(self, a, dtype=None):
        a = np.ascontiguousarray(a, dtype or self.np_dtype)
        return torch.from_numpy(a).to(f"cuda:{self.device}")

    def _out(self, name, t, R=1):
        """The output operand `name`: t where given, else a new, uninitialised tensor of the table's size and dtype."""
        return self.new(self._operands[name][0] * R, self._operands[name][1]) if t is None else t

    # ---- stages (device tensors in, device tensors out) -------------------------------------
    def convert(self, G_row, G_col, G_val, C_row, C_col, C_val, rho):
        Gd, Cd = self.new(self.sizes["G_dense"]), self.new(max(self.sizes["C_dense"], 1))
        _lib.check(_lib.lib().gato_convert(self._h, _ptr(G_row), _ptr(G_col), _ptr(G_val), _ptr(C_row),
                                           _ptr(C_col), _ptr(C_val), float(rho), _ptr(Gd), _ptr(Cd),
                                           self._stream()))
        return Gd, Cd[: self.sizes["C_dense"]]

    def form_schur(self, Gd, Cd, g, c):
        Sb, Pb = self.new(self.sizes["bd"]), self.new(self.sizes["bd"])
        gam, Gi = self.new(self.sizes["sk"]), self.new(self.sizes["G_dense"])
        _lib.check(_lib.lib().gato_form_schur(self._h, _ptr(Gd), _ptr(Cd), _ptr(g), _ptr(c), _ptr(Sb),
                                              _ptr(Pb), _ptr(gam), _ptr(Gi), self._stream()))
        return Sb, Pb, gam, Gi

    def form_ss(self, Sb, Pb):
        _lib.check(_lib.lib().gato_form_ss(self._h, _ptr(Sb), _ptr(Pb), self._stream()))
        return Pb

    def pcg(self, Sb, Pb, gamma, exit_tol, max_iters, lam=None, iters=None, check=True):
        """lam: output; with set_option("true_warm_start", 1) it is also the initial guess (in place)."""
        lam = self.new(self.sizes["sk"]) if lam is None else lam
        iters = self.new(1, torch.int32) if iters is None else iters
        _lib.check(_lib.lib().gato_pcg(self._h, _ptr(Sb), _ptr(Pb), _ptr(gamma), _ptr(lam), float(exit_tol),
                                       int(max_iters), _ptr(iters), self._stream()))
        if check:
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(_lib.lib().gato_pcg_status(self._h, None))
        return lam, iters

    def compute_dz(self, Gi, Cd, g, lam):
        dz = self.new(self.N)
        _lib.check(_lib.lib().gato_compute_dz(self._h, _ptr(Gi), _ptr(Cd), _ptr(g), _ptr(lam), _ptr(dz),
                                              self._stream()))
        return dz

    # ---- whole solve on device-resident CSR (gato_linsys, gpu_library.cu:25-83) ----------------
    def linsys(self, G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho,
               lam=None, dz=None):
        _lib.check(_lib.lib().gato_linsys_device(self._h, _ptr(G_row), _ptr(G_col), _ptr(G_val), _ptr(C_row),
                                                 _ptr(C_col), _ptr(C_val), _ptr(g), _ptr(c), float(exit_tol),
                                                 int(max_iters), float(rho), _ptr(lam), _ptr(dz),
                                                 self._stream()))

    def linsys_blocks(self, G_blocks, C_blocks, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        """Direct block input: G_blocks / C_blocks in the G_dense / C_dense layouts, rho not yet added."""
        _lib.check(_lib.lib().gato_linsys_device_blocks(self._h, _ptr(G_blocks), _ptr(C_blocks), _ptr(g), _ptr(c),
                                                        float(exit_tol), int(max_iters), float(rho), _ptr(lam),
                                                        _ptr(dz), self._stream()))

    def linsys_batched(self, G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho,
                       lam, dz, iters=None):
        """B systems with a shared CSR structure: G_val [B*nnzG], C_val [B*nnzC], g [B*N], c [B*S*K]."""
        nnzG, nnzC = G_val.numel() // self.batch, C_val.numel() // self.batch
        _lib.check(_lib.lib().gato_linsys_device_batched(
            self._h, _ptr(G_row), _ptr(G_col), _ptr(G_val), nnzG, _ptr(C_row), _ptr(C_col), _ptr(C_val), nnzC,
            _ptr(g), _ptr(c), float(exit_tol), int(max_iters), float(rho), _ptr(lam), _ptr(dz), _ptr(iters),
            self._stream()))

    # ---- re-solve of the latest assembly for new right-hand sides (gato_solve_rhs) ------------------------------------
    def reserve_rhs(self, R: int):
        """Room for up to R right-hand sides per system in the re-solve work area (blocking; only grows)."""
        _lib.check(_lib.lib().gato_solver_reserve_rhs(self._h, int(R)))

    def _resolve(self, cross, g, c, exit_tol, max_iters, lam, dz, iters):
        """The body of solve_rhs (cross False) and solve_rhs_cross: R from g, lam / dz / iters as given or new, the method's own
        checks - entry counts for the plain one, which sits on timed paths; every operand for the cross one - and the entry."""
        B, N, sk = self.batch, self.N, self.sizes["sk"]
        R = g.numel() // (B * N) if isinstance(g, torch.Tensor) and g.numel() % (B * N) == 0 else 0
        if R < 1 or c.numel() != B * R * sk:
            raise ValueError(f"solve_rhs_cross: g and c must hold B*R*N and B*R*S*K entries with B = {B}, N = {N}, S*K = {sk}, R >= 1"
                             if cross else f"solve_rhs: g has {g.numel()} entries and c {c.numel()}: want B*R*N and B*R*S*K with "
                             f"B = {B}, N = {N}, S*K = {sk}, R >= 1")
        lam = self.new(B * R * sk) if lam is None else lam
        dz = self.new(B * R * N) if dz is None else dz
        iters = self.new(B * R, torch.int32) if iters is None else iters
        if cross:
            self._check("solve_rhs_cross", dict(g=g, c=c, lam=lam, dz=dz), R)
            if iters.numel() != B * R or iters.dtype != torch.int32:
                raise ValueError("solve_rhs_cross: iters must hold B*R int32 entries")
        elif lam.numel() != B * R * sk or dz.numel() != B * R * N or iters.numel() != B * R:
            raise ValueError("solve_rhs: lam / dz / iters do not hold B*R*S*K / B*R*N / B*R entries")
        entry = _lib.lib().gato_solve_rhs_cross if cross else _lib.lib().gato_solve_rhs
        _lib.check(entry(self._h, R, _ptr(g), _ptr(c), float(exit_tol), int(max_iters), _ptr(lam), _ptr(dz), _ptr(iters), self._stream()))
        return lam, dz, iters

    def solve_rhs(self, g, c, exit_tol, max_iters, lam=None, dz=None, iters=None):
        """Re-solve the matrices of the most recent linsys / linsys_blocks / linsys_batched call for new right-hand sides:
        g [B][R][N], c [B][R][S K] (flat device tensors; R = g.numel() / (B N)) -> (lam [B R S K], dz [B R N], iters [B R])."""
        return self._resolve(False, g, c, exit_tol, max_iters, lam, dz, iters)

    # ---- gradients of a solve from dz, lambda and the adjoint (a, beta) (gato_kkt_grad_*) --------------------------------
    def kkt_grad_blocks(self, dz, lam, adz, alam, Gbar=None, Cbar=None):
        """G_bar [B][G_dense] and / or C_bar [B][C_dense] (either None: skipped) from dz, adz [B N] and lam, alam [B S K]."""
        _lib.check(_lib.lib().gato_kkt_grad_blocks(self._h, _ptr(dz), _ptr(lam), _ptr(adz), _ptr(alam), _ptr(Gbar),
                                                   _ptr(Cbar), self._stream()))
        return Gbar, Cbar

    def kkt_grad_csr(self, G_row, G_col, C_row, C_col, dz, lam, adz, alam, Gbar_val=None, Cbar_val=None):
        """The same gradient per CSR value of a pattern the B systems share: Gbar_val [B nnz_G], Cbar_val [B nnz_C]."""
        _lib.check(_lib.lib().gato_kkt_grad_csr(self._h, _ptr(G_row), _ptr(G_col), G_col.numel(), _ptr(C_row), _ptr(C_col),
                                                C_col.numel(), _ptr(dz), _ptr(lam), _ptr(adz), _ptr(alam), _ptr(Gbar_val),
                                                _ptr(Cbar_val), self._stream()))
        return Gbar_val, Cbar_val

    # ---- a state-control cross term in the stage cost (gato_*_cross) --------------------------------
    @property
    def M_size(self):
        """Entries of M_blocks per system: (K - 1) S C."""
        return self.sizes["M"]

    def _cross_inputs(self, what, G_blocks, M_blocks, C_blocks, g):
        self._check(what, dict(G_blocks=G_blocks, g=g, **(dict(M_blocks=M_blocks, C_blocks=C_blocks) if self.K > 1 else {})))

    def _check_solve_io(self, what, c, lam, dz):
        """The check of a whole cross solve's c [B S K] and of the outputs lam [B S K] and dz [B N] that are given."""
        self._check(what, dict(c=c, **_given(lam=lam, dz=dz)))

    def linsys_blocks_cross(self, G_blocks, M_blocks, C_blocks, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        """linsys_blocks with the cross term x_k^T M_k u_k in the stage cost (gato_linsys_device_blocks_cross): M_blocks [B (K-1) S C],
        per knot M_k S x C column-major as B_k lies in C_blocks (K = 1: None).  Every G_k + rho I must be positive definite.  lam
        and dz are those of the original problem; the solver's assembly afterwards is the transformed one (solve_rhs_cross
        re-solves the original problem, plain solve_rhs the transformed one).  Asynchronous but for a solver's first call."""
        self._cross_inputs("linsys_blocks_cross", G_blocks, M_blocks, C_blocks, g)
        self._check_solve_io("linsys_blocks_cross", c, lam, dz)
        _lib.check(_lib.lib().gato_linsys_device_blocks_cross(self._h, _ptr(G_blocks), _ptr(M_blocks if self.K > 1 else None),
                                                              _ptr(C_blocks), _ptr(g), _ptr(c), float(exit_tol), int(max_iters),
                                                              float(rho), _ptr(lam), _ptr(dz), self._stream()))

    def solve_rhs_cross(self, g, c, exit_tol, max_iters, lam=None, dz=None, iters=None):
        """solve_rhs for the original problem of the latest linsys_blocks_cross (gato_solve_rhs_cross): g [B][R][N], c [B][R][S K]
        -> (lam [B R S K], dz [B R N], iters [B R]).  Raises when the solver's current assembly is not that cross solve's."""
        return self._resolve(True, g, c, exit_tol, max_iters, lam, dz, iters)

    def kkt_grad_cross(self, dz, adz, Mbar=None):
        """M_bar [B (K-1) S C] (M's layout) of a cross solve from dz and the adjoint's a [B N], both in the original variables
        (gato_kkt_grad_cross): -(a_x dz_u^T + dz_x a_u^T) per knot, M_k and M_k^T perturbed together."""
        Mbar = self._out("Mbar", Mbar)
        self._check("kkt_grad_cross", dict(dz=dz, adz=adz, Mbar=Mbar))
        _lib.check(_lib.lib().gato_kkt_grad_cross(self._h, _ptr(dz), _ptr(adz), _ptr(Mbar), self._stream()))
        return Mbar

    def cross_prepare(self, G_blocks, M_blocks, C_blocks, g, rho):
        """The first stage of linsys_blocks_cross alone (gato_cross_prepare): the transformed blocks, W and g' into the work area
        (read_cross).  Forgets a recorded cross assembly."""
        self._cross_inputs("cross_prepare", G_blocks, M_blocks, C_blocks, g)
        _lib.check(_lib.lib().gato_cross_prepare(self._h, _ptr(G_blocks), _ptr(M_blocks if self.K > 1 else None), _ptr(C_blocks),
                                                 _ptr(g), float(rho), self._stream()))

    def cross_rhs(self, g, gp=None):
        """g' [B R N] of R right-hand sides g [B R N] from the stored W (gato_cross_rhs)."""
        R = g.numel() // (self.batch * self.N)
        gp = self.new(g.numel()) if gp is None else gp
        self._check("cross_rhs", dict(g=g, gp=gp), max(R, 1), entries=dict(gp=g.numel()))
        _lib.check(_lib.lib().gato_cross_rhs(self._h, R, _ptr(g), _ptr(gp), self._stream()))
        return gp

    def cross_finish(self, dz):
        """u <- v - W x in place on R solutions dz [B R N] from the stored W (gato_cross_finish)."""
        R = dz.numel() // (self.batch * self.N)
        self._check("cross_finish", dict(dz=dz), max(R, 1))
        _lib.check(_lib.lib().gato_cross_finish(self._h, R, _ptr(dz), self._stream()))
        return dz

    # ---- CSR entry to the cross solve (gato_*_csr*cross) ----------------------------------------------
    def _csr_cross_inputs(self, what, G_row, G_col, G_val, C_row, C_col, C_val, g):
        """ValueError unless the index arrays are contiguous int32 CUDA tensors of N + 1 / S K + 1 pointers and one column per
        value, and the values [B nnz] and g [B N] contiguous CUDA tensors of the solver's dtype.  -> (nnz_G, nnz_C) per system."""
        self._check(what, dict(G_row=G_row, G_col=G_col, C_row=C_row, C_col=C_col),
                    entries=dict(G_row=self.N + 1, G_col=None, C_row=self.sizes["sk"] + 1, C_col=None))
        nnzG, nnzC = G_col.numel(), C_col.numel()
        self._check(what, dict(G_val=G_val, C_val=C_val, g=g), entries=dict(G_val=self.batch * nnzG, C_val=self.batch * nnzC))
        return nnzG, nnzC

    def linsys_cross(self, G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        """linsys / linsys_batched for a G whose state rows hold control columns (gato_linsys_device_cross): such an entry of knot
        k < K-1 is M_k[isr, isc - S] of the stage cost's x_k^T M_k u_k, its mirror in the control rows is not read, and rho goes
        onto every diagonal entry of G, stored or not (the scatter rule: include/gato_hip.h).  Values [B nnz] on one shared
        pattern, one call for B = 1 and batches.  Afterwards the solver's assembly is a cross one, as after linsys_blocks_cross:
        solve_rhs_cross, tangents_cross and kkt_grad_cross follow it.  Asynchronous but for a solver's first cross call."""
        what = "linsys_cross"
        nnzG, nnzC = self._csr_cross_inputs(what, G_row, G_col, G_val, C_row, C_col, C_val, g)
        self._check_solve_io(what, c, lam, dz)
        _lib.check(_lib.lib().gato_linsys_device_cross(self._h, _ptr(G_row), _ptr(G_col), _ptr(G_val), nnzG, _ptr(C_row), _ptr(C_col),
                                                       _ptr(C_val), nnzC, _ptr(g), _ptr(c), float(exit_tol), int(max_iters),
                                                       float(rho), _ptr(lam), _ptr(dz), self._stream()))

    def cross_prepare_csr(self, G_row, G_col, G_val, C_row, C_col, C_val, g, rho, G_out=None, M_out=None, C_out=None):
        """The first stage of linsys_cross alone (gato_cross_prepare_csr): one launch gathers the CSR values and writes what
        cross_prepare writes into the work area (read_cross), bit for bit cross_prepare on the scattered blocks.  G_out
        [B G_dense] (without rho), M_out [B (K-1) S C], C_out [B C_dense]: each None or written whole with the scattered blocks.
        Forgets a recorded cross assembly."""
        what = "cross_prepare_csr"
        nnzG, nnzC = self._csr_cross_inputs(what, G_row, G_col, G_val, C_row, C_col, C_val, g)
        self._check(what, dict(G_out=G_out, M_out=M_out, C_out=C_out), optional=True)
        _lib.check(_lib.lib().gato_cross_prepare_csr(self._h, _ptr(G_row), _ptr(G_col), _ptr(G_val), nnzG, _ptr(C_row), _ptr(C_col),
                                                     _ptr(C_val), nnzC, _ptr(g), float(rho), _ptr(G_out), _ptr(M_out), _ptr(C_out),
                                                     self._stream()))
        return G_out, M_out, C_out

    def kkt_grad_csr_cross(self, G_row, G_col, C_row, C_col, dz, lam, adz, alam, Gbar_val=None, Cbar_val=None):
        """kkt_grad_csr through linsys_cross's scatter (gato_kkt_grad_csr_cross): a kept cross entry of G carries M_bar at its
        slot (kkt_grad_cross, bit for bit); a mirror entry, a cross entry of the last knot and an overwritten entry get 0."""
        _lib.check(_lib.lib().gato_kkt_grad_csr_cross(self._h, _ptr(G_row), _ptr(G_col), G_col.numel(), _ptr(C_row), _ptr(C_col),
                                                      C_col.numel(), _ptr(dz), _ptr(lam), _ptr(adz), _ptr(alam), _ptr(Gbar_val),
                                                      _ptr(Cbar_val), self._stream()))
        return Gbar_val, Cbar_val

    _CROSS_BUFFERS = dict(G=(13, "G_dense"), C=(14, "C_dense"), W=(15, "M"), g=(16, "N"))       # name -> (buffer, key of sizes)

    def cross_buffer_ptr(self, name: str) -> int:
        return self.buffer_ptr(self._CROSS_BUFFERS[name][0])

    def read_cross(self, name: str):
        """Host copy of a part of the cross-term work area (all systems): G (Q'' | R), C (A^' | B^), W or g (g')."""
        return self._read_buffer(*self._CROSS_BUFFERS[name])

    # ---- forward-mode sensitivities (gato_kkt_tangent_rhs) ------------------------------------------
    def kkt_tangent_rhs(self, R, x, lam, *, G_dot=None, C_dot=None, g_dot=None, c_dot=None, lo_dot=None, hi_dot=None, w_dot=None,
                        m_dot=None, Gb=None, Cb=None, act=None, soft_weight=None, soft_cap=None, lo=None, hi=None, tg=None, tc=None):
        """The right-hand side (tg [B R N], tc [B R S K]) of the tangent system of the point x [B N], lam [B S K] for R directions
        per system (gato_kkt_tangent_rhs): tangents G_dot [B R G_dense], C_dot [B R C_dense], g_dot, lo_dot, hi_dot, w_dot, m_dot
        [B R N], c_dot [B R S K], None = zero.  act [B N] int8 with Gb, Cb (and soft_weight with lo, hi; soft_cap) names the
        active set of a box-QP point; None: a plain KKT solve.  Asynchronous; touches no solver state."""
        R = int(R)
        if R < 1:
            raise ValueError(f"kkt_tangent_rhs: R = {R}: at least one direction")
        dots = dict(G_dot=G_dot, C_dot=C_dot, g_dot=g_dot, c_dot=c_dot, lo_dot=lo_dot, hi_dot=hi_dot, w_dot=w_dot, m_dot=m_dot)
        self._check("kkt_tangent_rhs", dots, R, optional=True)
        shared = dict(x=x, lam=lam)
        if act is not None:
            shared.update(Gb=Gb, Cb=Cb, act=act)
            if soft_weight is not None:
                shared.update(soft_weight=soft_weight, lo=lo, hi=hi, **_given(soft_cap=soft_cap))
        self._check("kkt_tangent_rhs", shared)
        tg, tc = self._out("tg", tg, R), self._out("tc", tc, R)
        self._check("kkt_tangent_rhs", dict(tg=tg, tc=tc), R, got=False)
        on = act is not None
        soft = on and soft_weight is not None
        _lib.check(_lib.lib().gato_kkt_tangent_rhs(
            self._h, R, *map(_ptr, dots.values()), _ptr(x), _ptr(lam), _ptr(Gb if on else None), _ptr(Cb if on else None),
            _ptr(act), _ptr(soft_weight if soft else None), _ptr(soft_cap if soft else None), _ptr(lo if soft else None),
            _ptr(hi if soft else None), _ptr(tg), _ptr(tc), self._stream()))
        return tg, tc

    def tangents(self, R, x, lam, exit_tol, max_iters, **inputs):
        """(lam_dot [B, R, S K], x_dot [B, R, N]): the tangents of the point (x, lam) of the solver's CURRENT assembly along R
        directions per system: kkt_tangent_rhs(R, x, lam, **inputs), one re-solve of the assembly for
        the B R right-hand sides, x_dot = b_dot on the hard-active set.  A (system, direction) pair whose right-hand side is all
        zero (off the hard-active set) gets x_dot = b_dot there, 0 elsewhere and lam_dot = 0 without its PCG, which would form
        0/0.  Blocking (reserve_rhs)."""
        B, R, N = self.batch, int(R), self.N
        tg, tc = self.kkt_tangent_rhs(R, x, lam, **inputs)
        act = inputs.get("act")
        if act is None:
            return self._tangent_solve(R, tg, tc, exit_tol, max_iters)
        act = act.view(B, 1, N)
        hard = hard_active(act, None if inputs.get("soft_weight") is None else inputs["soft_weight"].view(B, 1, N))
        lam_d, x_d = self._tangent_solve(R, tg, tc, exit_tol, max_iters, hard=hard)
        lo_d, hi_d = (None if t is None else t.view(B, R, N) for t in (inputs.get("lo_dot"), inputs.get("hi_dot")))
        return lam_d, bound_tangents(x_d, act, hard, lo_d, hi_d)

    def _tangent_solve(self, R, g, c, exit_tol, max_iters, finish=False, hard=None):
        """The middle of tangents and tangents_cross: room for R, one plain re-solve of the right-hand sides g [B R N], c [B R S K],
        cross_finish on the solutions where finish, check_status, and zeros for the pairs zero_rhs names (g masked on hard [B, 1,
        N] first, hard_active's set).  -> (lam_dot [B, R, S K], x_dot [B, R, N])."""
        B, N, sk = self.batch, self.N, self.sizes["sk"]
        self.reserve_rhs(R)
        lam_d, x_d, _ = self.solve_rhs(g, c, exit_tol, max_iters)
        if finish:
            self.cross_finish(x_d)
        self.check_status()
        g = g.view(B, R, N)
        zero = zero_rhs(g if hard is None else torch.where(hard, 0, g), c.view(B, R, sk))[:, :, None]
        return torch.where(zero, 0, lam_d.view(B, R, sk)), torch.where(zero, 0, x_d.view(B, R, N))

    # ---- forward-mode sensitivities of a cross solve (gato_kkt_tangent_rhs_cross) ------------------
    def kkt_tangent_rhs_cross(self, R, x, lam, *, G_dot=None, M_dot=None, C_dot=None, g_dot=None, c_dot=None, tg=None, gp=None,
                              tc=None):
        """The right-hand side of the tangent system of the point x [B N], lam [B S K] of the latest linsys_blocks_cross for R
        directions per system (gato_kkt_tangent_rhs_cross): tangents G_dot [B R G_dense], M_dot [B R (K-1) S C] (M's layout, M_k
        and M_k^T perturbed together), C_dot [B R C_dense], g_dot [B R N], c_dot [B R S K], None = zero.  -> (tg, gp, tc): t_g
        and the transformed g' [B R N] from the stored W, t_c [B R S K]; tg and gp both None: both are written, one given: only
        that one (the other is returned as None).  Raises when the solver's current assembly is not that cross solve's.
        Asynchronous; touches no solver state."""
        R = int(R)
        if R < 1:
            raise ValueError(f"kkt_tangent_rhs_cross: R = {R}: at least one direction")
        dots = dict(G_dot=G_dot, M_dot=M_dot, C_dot=C_dot, g_dot=g_dot, c_dot=c_dot)
        if tg is None and gp is None:
            tg, gp = self._out("tg", None, R), self._out("gp", None, R)
        tc = self._out("tc", tc, R)
        self._check("kkt_tangent_rhs_cross", dict(x=x, lam=lam))
        self._check("kkt_tangent_rhs_cross", dict(dots, tg=tg, gp=gp, tc=tc), R, optional=True)
        _lib.check(_lib.lib().gato_kkt_tangent_rhs_cross(self._h, R, *(_ptr(t) if t is not None and t.numel() else None for t in dots.values()),
                                                         _ptr(x), _ptr(lam), _ptr(tg), _ptr(gp), _ptr(tc), self._stream()))
        return tg, gp, tc

    def tangents_cross(self, R, x, lam, exit_tol, max_iters, **dots):
        """(lam_dot [B, R, S K], x_dot [B, R, N]): the tangents of the point (x, lam) of the latest linsys_blocks_cross along R
        directions per system, in the original variables: kkt_tangent_rhs_cross(R, x, lam, **dots) for
        g' and t_c, one plain re-solve of the transformed assembly for the B R right-hand sides, cross_finish on the solutions -
        three launches.  A (system, direction) pair whose right-hand side is all zero gets zeros without its PCG, which would
        form 0/0.  The assembly stays the cross one.  Blocking (reserve_rhs)."""
        R = int(R)
        _, gp, tc = self.kkt_tangent_rhs_cross(R, x, lam, gp=self._out("gp", None, max(R, 1)), **dots)
        # g' = 0 exactly where t_g = 0 (g'_u = t_g,u, and then g'_x = t_g,x), so the rule of Solver.tangents holds on g'
        return self._tangent_solve(R, gp, tc, exit_tol, max_iters, finish=self.K > 1)

    # ---- box-constrained QP by ADMM over the re-solve (gato_box_qp_solve) ------------------------
    def box_qp(self, Gb, Cb, g, c, lo, hi, *, rho, exit_tol, max_iters, admm_rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-6,
               eps_rel=1e-6, max_admm_iters=4000, check_every=25, x=None, z=None, y=None, lam=None, warm=False):
        """min 1/2 x^T (G + rho I) x - g^T x  s.t.  C x = c,  lo <= x <= hi  for every system of the batch.  Gb [B G_dense]
        (without rho), Cb [B C_dense], g / lo / hi [B N] (dz layout, +-inf allowed), c [B S K], flat or 2-D device tensors.
        x, z, y, lam: optional output tensors; warm=True reads z, y and lam (all three required) as the start.  Blocking.
        Raises ValueError for a NaN bound or lo > hi.  The solver's assembly is the QP's x-step matrix afterwards."""
        return self._box_qp_admm("box_qp", None, Gb, Cb, g, c, lo, hi, x, z, y, lam, warm, rho, exit_tol, max_iters, eps_abs, eps_rel,
                                 admm_rho=admm_rho, sigma=sigma, alpha=alpha, max_admm_iters=max_admm_iters, check_every=check_every)

    def box_qp_cross(self, Gb, Mb, Cb, g, c, lo, hi, *, rho, exit_tol, max_iters, admm_rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-6,
                     eps_rel=1e-6, max_admm_iters=4000, check_every=25, x=None, z=None, y=None, lam=None, warm=False):
        """box_qp with the cross term x_k^T M_k u_k in the stage cost (gato_box_qp_solve_cross): Mb [B (K-1)
        S C] in the layout of linsys_blocks_cross (K = 1: None, and the call is box_qp).  Every G_k + rho I must be positive
        definite.  The result is in the original variables (x, u), as are lo and hi.  The solver's assembly afterwards is the
        x-step matrix in the transformed variables of section 3.15; no cross assembly is recorded (solve_rhs_cross refuses)."""
        if self.K > 1:
            self._check("box_qp_cross", dict(Mb=Mb))
        return self._box_qp_admm("box_qp_cross", Mb if self.K > 1 else None, Gb, Cb, g, c, lo, hi, x, z, y, lam, warm, rho, exit_tol,
                                 max_iters, eps_abs, eps_rel, admm_rho=admm_rho, sigma=sigma, alpha=alpha,
                                 max_admm_iters=max_admm_iters, check_every=check_every)

    def _box_qp_admm(self, what, Mb, Gb, Cb, g, c, lo, hi, x, z, y, lam, warm, rho, exit_tol, max_iters, eps_abs, eps_rel, **admm):
        """box_qp (Mb None, what = "box_qp") or box_qp_cross: the outputs, the checks, the entry and the result record."""
        B = self.batch
        if warm and (z is None or y is None or lam is None):
            raise ValueError(f"{what}: warm=True reads z, y and lam: give all three")
        x, z, y, lam = self._out("x", x), self._out("z", z), self._out("y", y), self._out("lam", lam)
        self._check(what, dict(Gb=Gb, Cb=Cb, g=g, c=c, lo=lo, hi=hi, x=x, z=z, y=y, lam=lam))
        iters = self.new(B, torch.int32)
        status = self.new(B, torch.int32)
        res = self.new(2 * B, torch.float64)
        p = self._qp_params(rho, exit_tol, max_iters, eps_abs, eps_rel, warm=bool(warm), **admm)
        tail = (_ptr(Cb), _ptr(g), _ptr(c), _ptr(lo), _ptr(hi), ct.byref(p), _ptr(x), _ptr(z), _ptr(y), _ptr(lam), _ptr(iters),
                _ptr(status), _ptr(res), self._stream())
        if what == "box_qp":
            rc = _lib.lib().gato_box_qp_solve(self._h, _ptr(Gb), *tail)
        else:
            rc = _lib.lib().gato_box_qp_solve_cross(self._h, _ptr(Gb), _ptr(Mb), *tail)
        self._check_marked(what, rc, status, BAD_BOUNDS=_lib.QP_BAD_BOUNDS)
        res = res.view(B, 2)
        return BoxQPResult(x, z, y, lam, iters, status, res[:, 0], res[:, 1])

    # ---- polish of a box QP and its bound gradients (gato_box_qp_polish) --------------------------
    @staticmethod
    def _qp_params(rho, exit_tol, max_iters, eps_abs, eps_rel, **admm):
        """A gato_box_qp_params: the library's defaults, the five values every box-QP entry reads, and the ADMM fields given."""
        p = _lib.BoxQpParams()
        _lib.lib().gato_box_qp_default_params(ct.byref(p))
        p.rho, p.exit_tol, p.max_iters, p.eps_abs, p.eps_rel = float(rho), float(exit_tol), int(max_iters), float(eps_abs), float(eps_rel)
        for name, v in admm.items():
            setattr(p, name, type(getattr(p, name))(v))       # float or int, as the field is
        return p

    @staticmethod
    def _check_marked(what, rc, marks, **codes):
        """After a box-QP entry returned rc: where its error names one of `codes` (name in the text = value in marks, the
        entry's status or polish codes [B]), ValueError with the systems so marked; every other error as _lib.check raises it."""
        msg = _lib.lib().gato_last_error().decode() if rc != 0 else ""
        if any(name in msg for name in codes):
            bad = [i for i, v in enumerate(marks.tolist()) if v in codes.values()]
            raise ValueError(f"{what}: systems {bad}: " + msg)
        _lib.check(rc)

    def _new_point(self, what, act, x, z, y, lam):
        """The output point of an active-set-type call: x, z, y [B N] and lam [B S K] (those given; new ones are zero), a copy
        of the start act (None: nothing active), iters and status [B] int32, res [2 B] float64."""
        B, N, sk = self.batch, self.N, self.sizes["sk"]
        zeros = lambda n, dt=self.dtype: torch.zeros(n, dtype=dt, device=f"cuda:{self.device}")
        x, z, y = (zeros(B * N) if t is None else t for t in (x, z, y))
        lam = zeros(B * sk) if lam is None else lam
        if act is None:
            act = zeros(B * N, torch.int8)
        else:
            self._check(what, dict(act=act))
            act = act.detach().reshape(-1).clone()
        return x, z, y, lam, act, zeros(B, torch.int32), self.new(B, torch.int32), zeros(2 * B, torch.float64)

    def box_qp_active_set(self, z, y, lo, hi, act=None):
        """The active set of an ADMM result (z, y [B N]) for the box (lo, hi): int8 [B N], +1 upper, -1 lower (and lo ==
        hi), 0 free and on the states of x_0."""
        act = self._out("act", act)
        self._check("box_qp_active_set", dict(z=z, y=y, lo=lo, hi=hi, act=act))
        _lib.check(_lib.lib().gato_box_qp_active_set(self._h, _ptr(z), _ptr(y), _ptr(lo), _ptr(hi), _ptr(act), self._stream()))
        return act

    def box_qp_polish(self, Gb, Cb, g, c, lo, hi, act, result, *, rho, exit_tol, max_iters, eps_abs=1e-6, eps_rel=1e-6):
        """Polish `result` (a BoxQPResult of box_qp on this solver, same inputs) on the active set act [B N] int8: where the
        polished point passes the test, result's x, z, y, lam, status and residuals are replaced in place; elsewhere not
        written.  Returns the polish codes int32 [B] (_lib.POLISH_*), also stored as result.polished.  Blocking.  Raises
        ValueError for an act that names an infinite bound or a state of x_0.  The solver's assembly is the reduced system
        afterwards (solve_rhs re-solves it)."""
        B = self.batch
        res = getattr(result.res_prim, "_base", None)        # the [B][2] residual array the two are views of
        if (res is None or res is not getattr(result.res_dual, "_base", None) or res.numel() != 2 * B
                or result.res_prim.data_ptr() != res.data_ptr() or res.dtype != torch.float64 or not res.is_contiguous()):
            raise ValueError("box_qp_polish: result must be the BoxQPResult of Solver.box_qp on this solver")
        self._check("box_qp_polish", dict(Gb=Gb, Cb=Cb, g=g, c=c, lo=lo, hi=hi, act=act, x=result.x, z=result.z, y=result.y,
                                          lam=result.lam, status=result.status))
        p = self._qp_params(rho, exit_tol, max_iters, eps_abs, eps_rel)
        codes = self.new(B, torch.int32)
        rc = _lib.lib().gato_box_qp_polish(self._h, _ptr(Gb), _ptr(Cb), _ptr(g), _ptr(c), _ptr(lo), _ptr(hi), _ptr(act), ct.byref(p),
                                           _ptr(result.x), _ptr(result.z), _ptr(result.y), _ptr(result.lam), _ptr(result.status),
                                           _ptr(res), _ptr(codes), self._stream())
        self._check_marked("box_qp_polish", rc, codes, BAD_ACTIVE=_lib.POLISH_BAD_ACTIVE)
        result.polished = codes
        return codes

    # (weights, caps, line search) -> the C entry of box_qp_pdas and which of the weights (w) and caps (m) it has arguments for
    _PDAS_ENTRIES = {(False, False, False): ("gato_box_qp_pdas", ""), (True, False, False): ("gato_box_qp_pdas_soft", "w"),
                     (True, True, False): ("gato_box_qp_pdas_huber", "wm"), (True, False, True): ("gato_box_qp_pdas_ls", "wm"),
                     (True, True, True): ("gato_box_qp_pdas_ls", "wm")}

    def box_qp_pdas(self, Gb, Cb, g, c, lo, hi, *, rho, exit_tol, max_iters, eps_abs=1e-6, eps_rel=1e-6, max_pdas_iters=30,
                    act=None, x=None, z=None, y=None, lam=None, soft_weight=None, soft_cap=None, line_search=False):
        """The box QP of box_qp by the primal-dual active-set iteration (gato_box_qp_pdas): the polish
        iterated from the active set act [B N] int8 (None: nothing active, a cold start; the tensor is not written) until
        the polished point passes the polish's test.  No penalty parameter and no ADMM.  Returns a BoxQPResult: status
        CONVERGED (x, z, y, lam, res_* written), MAX_ITERS or NONFINITE (they are not: the optional output tensors x, z, y, lam
        keep what they held, new ones are zero); iters the reduced solves; polished ACCEPTED where CONVERGED; act the final
        active set, that of the solver's assembly afterwards (solve_rhs re-solves the reduced system).  Blocking.  Raises
        ValueError for a NaN bound or lo > hi, and for an act that names an infinite bound or a state of x_0.
        soft_weight [B N] (gato_box_qp_pdas_soft): a weight w_i >= 0 per variable; w_i > 0 replaces the
        bound of variable i by the penalty (w_i / 2) dist(x_i, [lo_i, hi_i])^2 - where such a variable violates its bound it is
        active, x holds the reduced solution, z = x and y = w_i (x_i - b_i) - and w_i = 0 keeps the hard bound.  A weight that
        is NaN, negative or infinite raises ValueError.  None: gato_box_qp_pdas.
        soft_cap [B N] (with soft_weight; gato_box_qp_pdas_huber): a cap m_i >= 0 on the penalty force of
        variable i, read where w_i > 0; +inf: none.  The penalty is then the Huber function; where w_i (x_i - b_i) passes m_i the
        variable is saturated - act = +2 above hi, -2 below lo - and y = +-m_i.  act may hold +-2 on such variables.  A cap that is
        NaN or negative raises ValueError.  None: gato_box_qp_pdas_soft.
        line_search=True (with soft_weight; gato_box_qp_pdas_ls): every solve after the first moves an
        iterate xc to the exact minimiser of the penalised objective along the direction to the solve's point, and the next
        act is that of xc; the result's alpha [B, max_pdas_iters] holds the step lengths (1: a full step, 0: no step taken).
        Every variable off x_0 with a finite bound must have a positive weight: a finite hard bound raises ValueError."""
        if soft_cap is not None and soft_weight is None:
            raise ValueError("box_qp_pdas: soft_cap needs soft_weight (a cap is read only where the weight is positive)")
        if line_search and soft_weight is None:
            raise ValueError("box_qp_pdas: line_search=True needs soft_weight (the line search takes soft bounds only: every "
                             "variable with a finite bound needs a positive weight)")
        B = self.batch
        x, z, y, lam, act, iters, status, res = self._new_point("box_qp_pdas", act, x, z, y, lam)
        self._check("box_qp_pdas", dict(Gb=Gb, Cb=Cb, g=g, c=c, lo=lo, hi=hi, x=x, z=z, y=y, lam=lam,
                                        **_given(soft_weight=soft_weight, soft_cap=soft_cap)))
        p = self._qp_params(rho, exit_tol, max_iters, eps_abs, eps_rel)
        alpha = torch.zeros(B, int(max_pdas_iters), dtype=torch.float64, device=act.device) if line_search else None
        entry, takes = self._PDAS_ENTRIES[soft_weight is not None, soft_cap is not None, bool(line_search)]
        soft = {"": (), "w": (soft_weight,), "wm": (soft_weight, soft_cap)}[takes]        # what the entry takes before act
        steps = (alpha,) if line_search else ()                                            # and after res
        rc = getattr(_lib.lib(), entry)(self._h, *map(_ptr, (Gb, Cb, g, c, lo, hi, *soft, act)), ct.byref(p), int(max_pdas_iters),
                                        *map(_ptr, (x, z, y, lam, iters, status, res, *steps)), self._stream())
        self._check_marked("box_qp_pdas", rc, status, BAD_BOUNDS=_lib.QP_BAD_BOUNDS, BAD_ACTIVE=_lib.QP_BAD_ACTIVE)
        res = res.view(B, 2)
        codes = torch.where(status == _lib.QP_CONVERGED, _lib.POLISH_ACCEPTED,
                            torch.where(status == _lib.QP_NONFINITE, _lib.POLISH_NONFINITE, _lib.POLISH_REJECTED)).to(torch.int32)
        return BoxQPResult(x, z, y, lam, iters, status, res[:, 0], res[:, 1], codes, act, alpha)

    def box_qp_line_search(self, Gb, g, lo, hi, soft_weight, soft_cap, xc, xplus, *, rho, x=None):
        """The line search of box_qp_pdas(line_search=True) alone (gato_box_qp_line_search): from the
        iterate xc and the Newton point xplus [B N], along d = xplus - xc, -> (alpha [B], slope [B, 2], x): the slopes phi'(0)
        and phi'(1) of the penalised objective with H = G + rho I (float64), the step length alpha (float64; 1 where phi'(1) <=
        0 or phi'(0) >= 0, else the root of phi' in (0, 1)) and, where x [B N] is given, x = xc + alpha d (xplus bit for bit where
        alpha = 1).  soft_cap None: no caps.  Asynchronous."""
        self._check("box_qp_line_search", dict(Gb=Gb, g=g, lo=lo, hi=hi, soft_weight=soft_weight, xc=xc, xplus=xplus,
                                               **_given(soft_cap=soft_cap, x=x)))
        alpha = torch.zeros(self.batch, dtype=torch.float64, device=g.device)
        slope = torch.zeros(self.batch, 2, dtype=torch.float64, device=g.device)
        _lib.check(_lib.lib().gato_box_qp_line_search(self._h, _ptr(Gb), _ptr(g), _ptr(lo), _ptr(hi), _ptr(soft_weight), _ptr(soft_cap),
                                                      float(rho), _ptr(xc), _ptr(xplus), _ptr(alpha), _ptr(slope), _ptr(x),
                                                      self._stream()))
        return alpha, slope, x

    # ---- hard bounds by an augmented-Lagrangian outer loop (gato_box_qp_alm) ----------------------
    def box_qp_alm(self, Gb, Cb, g, c, lo, hi, *, rho, exit_tol, max_iters, eps_abs=1e-6, eps_rel=1e-6, max_pdas_iters=30,
                   alm_weight=100.0, alm_growth=10.0, alm_weight_max=None, max_alm_iters=50, act=None, mu=None, x=None, z=None,
                   y=None, lam=None, soft_weight=None, soft_cap=None):
        """The box QP of box_qp with hard bounds on states and controls, by the method of multipliers over
        box_qp_pdas(line_search=True) (gato_box_qp_alm).  Every variable off x_0 with a finite bound and
        no positive soft_weight gets a multiplier (start: mu [B N], None: 0) and the penalty weight w (start: alm_weight); each
        outer step is one line-search iteration on the bounds shifted by -mu / w, from the act the step before ended on (start:
        act, None: nothing active), then mu <- its force y, and w <- alm_growth w where the violation did not fall below a
        quarter of the step before (while w < alm_weight_max; None: 1e8 in float64, 1e5 in float32).  A variable with
        soft_weight > 0 stays the soft bound of box_qp_pdas (soft_cap: its cap).  Returns a BoxQPResult: status CONVERGED (x; z =
        x clipped on the hard variables; y; lam; res_* written) where the violation is within eps_abs + eps_rel |x|_inf, MAX_ITERS
        after max_alm_iters steps (res_prim = the last violation; an infeasible box ends so) or where an inner iteration did not
        converge, NONFINITE; iters the reduced solves of all steps, outer the steps, weight the last step's w; act the accepted
        act.  The optional output tensors keep what they held for a system that did not converge.  Blocking.  Raises ValueError
        for bad bounds, weights, caps or parameters and for a start act the iteration cannot take."""
        if soft_cap is not None and soft_weight is None:
            raise ValueError("box_qp_alm: soft_cap needs soft_weight (a cap is read only where the weight is positive)")
        if alm_weight_max is None:
            alm_weight_max = max(ALM_WEIGHT_MAX[self.np_dtype], float(alm_weight))
        B, dev = self.batch, f"cuda:{self.device}"
        x, z, y, lam, act, iters, status, res = self._new_point("box_qp_alm", act, x, z, y, lam)
        self._check("box_qp_alm", dict(Gb=Gb, Cb=Cb, g=g, c=c, lo=lo, hi=hi, x=x, z=z, y=y, lam=lam,
                                       **_given(soft_weight=soft_weight, soft_cap=soft_cap, mu=mu)))
        outer = torch.zeros(B, dtype=torch.int32, device=dev)
        weight = torch.zeros(B, dtype=torch.float64, device=dev)
        p = self._qp_params(rho, exit_tol, max_iters, eps_abs, eps_rel)
        rc = _lib.lib().gato_box_qp_alm(self._h, _ptr(Gb), _ptr(Cb), _ptr(g), _ptr(c), _ptr(lo), _ptr(hi), _ptr(soft_weight),
                                        _ptr(soft_cap), _ptr(act), ct.byref(p), int(max_pdas_iters), float(alm_weight),
                                        float(alm_growth), float(alm_weight_max), int(max_alm_iters), _ptr(mu), _ptr(x), _ptr(z),
                                        _ptr(y), _ptr(lam), _ptr(iters), _ptr(status), _ptr(res), _ptr(outer), _ptr(weight),
                                        self._stream())
        self._check_marked("box_qp_alm", rc, status, BAD_BOUNDS=_lib.QP_BAD_BOUNDS, BAD_ACTIVE=_lib.QP_BAD_ACTIVE)
        res = res.view(B, 2)
        return BoxQPResult(x, z, y, lam, iters, status, res[:, 0], res[:, 1], None, act, None, outer, weight)

    def box_qp_alm_update(self, x, y, lam, mu, w, v_prev, lo, hi, *, eps_abs=1e-6, eps_rel=1e-6, alm_growth=10.0, alm_weight_max=1e8,
                          last=False, soft_weight=None, lo2=None, hi2=None, w2=None, z=None):
        """The update and the decision of one outer step of box_qp_alm alone (gato_box_qp_alm_update), on converged inner points x,
        y [B N], lam [B S K] with the multipliers mu [B N] (updated in place), the weights w [B] and the violations of the step
        before v_prev [B] (float64; inf: the first step).  -> dict v, xinf [B] (float64), dec [B] (int32, _lib.ALM_*), mu, and
        lo2, hi2, w2 [B N] - the next inner bounds and weights, written on the ALM variables of a system that goes on - and z [B N],
        written for an accepted system (the four may be given; new ones start as NaN).  soft_weight [B N]: the variables with a
        positive weight are soft bounds, not ALM variables (caps play no part in the update).  Asynchronous."""
        B, N = self.batch, self.N
        dev = f"cuda:{self.device}"
        nans = lambda: torch.full((B * N,), float("nan"), dtype=self.dtype, device=dev)
        lo2, hi2, w2, z = (nans() if t is None else t for t in (lo2, hi2, w2, z))
        self._check("box_qp_alm_update", dict(x=x, y=y, lam=lam, mu=mu, lo=lo, hi=hi, lo2=lo2, hi2=hi2, w2=w2, z=z,
                                              **_given(soft_weight=soft_weight)))
        self._check("box_qp_alm_update", dict(w=w, v_prev=v_prev), got=False)
        v = torch.zeros(B, dtype=torch.float64, device=dev)
        xinf = torch.zeros(B, dtype=torch.float64, device=dev)
        dec = torch.zeros(B, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().gato_box_qp_alm_update(self._h, _ptr(x), _ptr(y), _ptr(lam), _ptr(mu), _ptr(w), _ptr(v_prev), _ptr(lo),
                                                     _ptr(hi), _ptr(soft_weight), float(eps_abs), float(eps_rel),
                                                     float(alm_growth), float(alm_weight_max), int(bool(last)), _ptr(v), _ptr(xinf),
                                                     _ptr(dec), _ptr(lo2), _ptr(hi2), _ptr(w2), _ptr(z), self._stream()))
        return dict(v=v, xinf=xinf, dec=dec, mu=mu, lo2=lo2, hi2=hi2, w2=w2, z=z)

    def _bound_grads(self, entry, what, Gb, Cb, act, soft, xbar, a, beta, **bars):
        """The body of the three bound-gradient methods: allocates the outputs bars (by name) that are None, checks every
        operand as `what`, calls the C entry and returns the outputs.  soft: the operands only the soft and the capped entry
        take, by name and in the entry's order (a soft_weight or soft_cap of None goes as a null pointer); {} for the entry
        without weights."""
        bars = {name: self._out(name, t) for name, t in bars.items()}
        own = {name: t for name, t in soft.items() if name not in ("soft_weight", "soft_cap") or t is not None}
        self._check(what, dict(Gb=Gb, Cb=Cb, act=act, **own, xbar=xbar, a=a, beta=beta, **bars))
        _lib.check(entry(self._h, _ptr(Gb), _ptr(Cb), _ptr(act), *map(_ptr, soft.values()), _ptr(xbar), _ptr(a), _ptr(beta),
                         *map(_ptr, bars.values()), self._stream()))
        return tuple(bars.values())

    def box_qp_bound_grad(self, Gb, Cb, act, xbar, a, beta, lo_bar=None, hi_bar=None):
        """(lo_bar, hi_bar) [B N] of a polished solution from its active set, the upstream x_bar and the adjoint (a, beta) of
        the reduced system (solve_rhs after the polish)."""
        return self._bound_grads(_lib.lib().gato_box_qp_bound_grad, "box_qp_bound_grad", Gb, Cb, act, {}, xbar, a, beta,
                                 lo_bar=lo_bar, hi_bar=hi_bar)

    def box_qp_soft_grad(self, Gb, Cb, act, soft_weight, lo, hi, x, xbar, a, beta, lo_bar=None, hi_bar=None, w_bar=None):
        """(lo_bar, hi_bar, w_bar) [B N] of a converged box_qp_pdas(soft_weight=) point (gato_box_qp_soft_grad) from its act,
        the upstream x_bar and the adjoint (a, beta) of its last assembly (solve_rhs after the call): the hard formula of
        box_qp_bound_grad on the hard-active set, w_i a_i and a_i (b_i - x_i) on the soft-active one, 0 elsewhere.
        soft_weight None: all hard."""
        return self._bound_grads(_lib.lib().gato_box_qp_soft_grad, "box_qp_soft_grad", Gb, Cb, act,
                                 dict(soft_weight=soft_weight, lo=lo, hi=hi, x=x), xbar, a, beta, lo_bar=lo_bar, hi_bar=hi_bar, w_bar=w_bar)

    def box_qp_huber_grad(self, Gb, Cb, act, soft_weight, soft_cap, lo, hi, x, xbar, a, beta, lo_bar=None, hi_bar=None,
                          w_bar=None, cap_bar=None):
        """(lo_bar, hi_bar, w_bar, cap_bar) [B N] of a converged box_qp_pdas(soft_weight=, soft_cap=) point
        (gato_box_qp_huber_grad): a saturated variable (act = +-2, s its sign) gets cap_bar_i = -s a_i and 0 in the other
        three, every other variable what box_qp_soft_grad gives it and cap_bar_i = 0.  soft_cap None: no caps."""
        return self._bound_grads(_lib.lib().gato_box_qp_huber_grad, "box_qp_huber_grad", Gb, Cb, act,
                                 dict(soft_weight=soft_weight, soft_cap=soft_cap, lo=lo, hi=hi, x=x), xbar, a, beta, lo_bar=lo_bar,
                                 hi_bar=hi_bar, w_bar=w_bar, cap_bar=cap_bar)

    def box_qp_pcg_iters(self):
        """PCG iterations of all x-steps of the latest box_qp call, per system (host int array)."""
        return self._read_device(self.buffer_ptr(12), np.zeros(self.batch, np.int32))

    def _read_device(self, ptr, out):
        """Fill the host array out from device memory at ptr, after everything queued on the device has finished."""
        torch.cuda.synchronize(self.device)
        rc = ct.CDLL("libamdhip64.so").hipMemcpy(out.ctypes.data_as(ct.c_void_p), ct.c_void_p(ptr), ct.c_size_t(out.nbytes), 2)
        if rc != 0:
            raise RuntimeError(f"hipMemcpy failed: {rc}")
        return out

    def _read_buffer(self, which, key):
        """Host copy of the work buffer `which`, of sizes[key] entries per system (all systems of a batch)."""
        out = np.empty(self.sizes[key] * self.batch, self.np_dtype)
        return out if out.size == 0 else self._read_device(self.buffer_ptr(which), out)

    def read_rhs_gamma(self, R: int):
        """Host copy of the re-solve's gamma [B][R][S K] (buffer 11) after a re-solve of R right-hand sides."""
        n = self.batch * int(R) * self.sizes["sk"]
        return self._read_device(self.buffer_ptr(11), np.empty(n, self.np_dtype))

    def upload_batch(self, systems):
        """list of KKTSystem with identical sparsity -> device tensors in linsys_batched() argument order."""
        s0 = systems[0]
        for s in systems:
            assert np.array_equal(s.G_row, s0.G_row) and np.array_equal(s.G_col, s0.G_col)
            assert np.array_equal(s.C_row, s0.C_row) and np.array_equal(s.C_col, s0.C_col)
        dev = f"cuda:{self.device}"
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        cat = lambda name: np.concatenate([getattr(s, name) for s in systems])
        return (t(s0.G_row, np.int32), t(s0.G_col, np.int32), t(cat("G_val"), self.np_dtype),
                t(s0.C_row, np.int32), t(s0.C_col, np.int32), t(cat("C_val"), self.np_dtype),
                t(cat("g"), self.np_dtype), t(cat("c"), self.np_dtype))

    def buffer_ptr(self, which: int) -> int:
        return int(_lib.lib().gato_solver_buffer(self._h, which))

    # name -> (buffer, key of sizes)
    _BUFFERS = dict(G_dense=(0, "G_dense"), C_dense=(1, "C_dense"), Ginv=(2, "G_dense"), S=(3, "bd"), Pinv=(4, "bd"), gamma=(5, "sk"),
                    lam=(6, "sk"), dz=(7, "N"))

    def read_buffer(self, name: str):
        """Host copy of one of the solver's own work buffers (all systems of a batch), for tests and debugging."""
        return self._read_buffer(*self._BUFFERS[name])

    def pcg_last_ms(self) -> float:
        """Device time of the last PCG launch (needs set_option("time_pcg", 1))."""
        ms = ct.c_float()
        _lib.check(_lib.lib().gato_pcg_last_ms(self._h, ct.byref(ms)))
        return ms.value

    def last_stage_ms(self):
        """{assembly, pcg, dz} device times (ms) of the last linsys / linsys_blocks call (needs set_option("time_stages", 1))."""
        ms = (ct.c_float * 3)()
        _lib.check(_lib.lib().gato_last_stage_ms(self._h, ms))
        return dict(assembly=ms[0], pcg=ms[1], dz=ms[2])

    def eta_history(self, n: int):
        """eta = r . Pinv r after the initial step and after each of the first n iterations (needs record_eta=1)."""
        return self._read_device(self.buffer_ptr(10), np.empty(n + 1, np.float64))

    def check_status(self):
        """Raises GatoError(ETIMEOUT) if a hand-off of any PCG launch since the last check timed out."""
        _lib.check(_lib.lib().gato_pcg_status(self._h, None))

    def recover(self) -> bool:
        """After linsys / linsys_blocks: if a persistent launch timed out (its workgroups were not co-resident), re-run
        the PCG through the streaming kernels and recompute dz into the same buffers.  True if that happened."""
        v = ct.c_int()
        _lib.check(_lib.lib().gato_solver_recover(self._h, ct.byref(v), self._stream()))
        return bool(v.value)

    def upload_system(self, sysm):
        """KKTSystem (host CSR) -> tuple of device tensors in linsys() argument order."""
        return self.upload_batch([sysm])
