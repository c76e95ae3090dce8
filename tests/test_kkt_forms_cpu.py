"""The one autograd Function of the KKT solve (gato_python_amd.autograd._KktSolve) against a recording stub in place of Solver,
on CPU tensors: which solver methods each of the four input forms calls, and in which order - forward, backward on a fresh and on
a stale assembly, backward without incoming gradients, backward for some inputs only.  The expected sequences are those of the
four Function classes this one replaced (_BlocksSolve, _CrossSolve, _CsrSolve, _CsrCrossSolve), read off their code."""
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from gato_python_amd import autograd as ag

S, C, K, B = 2, 1, 3, 2
OPTS = (1e-3, 0.0, 5)                       # rho, exit_tol, max_iters


class StubSolver:
    """Solver's methods as far as _KktSolve uses them: each records its name; a whole solve fills lam and dz with fixed values
    when they are given, a re-solve returns zeros, a gradient call fills what it is given."""

    def __init__(self, S, C, K, B):
        self.batch, self.N, self.sizes = B, (S + C) * K - C, {"sk": S * K}
        self.calls, self.gen = [], 7

    def _whole(self, name, lam, dz):
        self.calls.append(name)
        if lam is not None:
            lam.fill_(0.5)
        if dz is not None:
            dz.fill_(-2.0)

    def linsys_blocks(self, Gb, Cb, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        self._whole("linsys_blocks", lam, dz)

    def linsys_blocks_cross(self, Gb, Mb, Cb, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        self._whole("linsys_blocks_cross", lam, dz)

    def linsys(self, G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        self._whole("linsys", lam, dz)

    def linsys_batched(self, G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam, dz, iters=None):
        self._whole("linsys_batched", lam, dz)

    def linsys_cross(self, G_row, G_col, G_val, C_row, C_col, C_val, g, c, exit_tol, max_iters, rho, lam=None, dz=None):
        self._whole("linsys_cross", lam, dz)

    def check_status(self):
        self.calls.append("check_status")

    def get_option(self, name):
        self.calls.append(f"get_option({name})")
        return self.gen if name == "assembly_gen" else 1

    def reserve_rhs(self, R):
        self.calls.append("reserve_rhs")

    def _resolve(self, name, g):
        self.calls.append(name)
        return (torch.zeros(self.batch * self.sizes["sk"], dtype=g.dtype), torch.zeros(self.batch * self.N, dtype=g.dtype),
                torch.zeros(self.batch, dtype=torch.int32))

    def solve_rhs(self, g, c, exit_tol, max_iters, lam=None, dz=None, iters=None):
        return self._resolve("solve_rhs", g)

    def solve_rhs_cross(self, g, c, exit_tol, max_iters, lam=None, dz=None, iters=None):
        return self._resolve("solve_rhs_cross", g)

    def _grad(self, name, *bars):
        self.calls.append(name)
        for b in bars:
            if b is not None:
                b.zero_()

    def kkt_grad_blocks(self, dz, lam, adz, alam, Gbar=None, Cbar=None):
        self._grad("kkt_grad_blocks", Gbar, Cbar)

    def kkt_grad_cross(self, dz, adz, Mbar=None):
        self._grad("kkt_grad_cross", Mbar)

    def kkt_grad_csr(self, G_row, G_col, C_row, C_col, dz, lam, adz, alam, Gbar_val=None, Cbar_val=None):
        self._grad("kkt_grad_csr", Gbar_val, Cbar_val)

    def kkt_grad_csr_cross(self, G_row, G_col, C_row, C_col, dz, lam, adz, alam, Gbar_val=None, Cbar_val=None):
        self._grad("kkt_grad_csr_cross", Gbar_val, Cbar_val)


IDX = tuple(torch.zeros(3, dtype=torch.int32) for _ in range(4))
# form -> (the record, idx, per-system sizes of its matrix tensors, forward call, re-solve, gradient calls with all inputs wanted)
FORMS = {
    "blocks": (ag._BLOCKS, None, ("G", "C"), "linsys_blocks", "solve_rhs", ["kkt_grad_blocks"]),
    "blocks_cross": (ag._BLOCKS_CROSS, None, ("G", "M", "C"), "linsys_blocks_cross", "solve_rhs_cross",
                     ["kkt_grad_blocks", "kkt_grad_cross"]),
    "csr": (ag._CSR, IDX, ("nnzG", "nnzC"), "linsys_batched", "solve_rhs", ["kkt_grad_csr"]),
    "csr_cross": (ag._CSR_CROSS, IDX, ("nnzG", "nnzC"), "linsys_cross", "solve_rhs_cross", ["kkt_grad_csr_cross"]),
}
FRESH = ["get_option(assembly_gen)", "get_option(assembly_valid)"]
STALE = ["get_option(assembly_gen)"]                      # the generation differs: assembly_valid is not asked for


def sizes(K):
    return dict(G=K * S * S + (K - 1) * C * C, C=(K - 1) * (S * S + S * C), M=(K - 1) * S * C, nnzG=5, nnzC=4)


def run_forward(name, need=None, K=K, dual=False):
    """-> (sol, inputs by name, lam, dz); need: the names of the inputs that require grad (None: all)."""
    form, idx, parts, *_ = FORMS[name]
    sol = StubSolver(S, C, K, B)
    gen = torch.Generator().manual_seed(0)
    names = ("g", "c") + parts
    n = dict(sizes(K), g=sol.N, c=sol.sizes["sk"])
    ins = {k: torch.randn(B, n[k], dtype=torch.float64, generator=gen) for k in names}
    for k, t in ins.items():
        t.requires_grad_(need is None or k in need)
    if dual:
        ins["g"] = fwAD.make_dual(ins["g"].detach(), torch.ones_like(ins["g"]))
    lam, dz = ag._KktSolve.apply(form, idx, sol, *OPTS, *ins.values())
    return sol, ins, lam, dz


@pytest.mark.parametrize("name", FORMS)
def test_forward(name):
    sol, _, lam, dz = run_forward(name)
    assert sol.calls == [FORMS[name][3], "check_status", "get_option(assembly_gen)"]
    assert lam.shape == (B, S * K) and dz.shape == (B, (S + C) * K - C)
    assert torch.all(lam == 0.5) and torch.all(dz == -2.0)


def test_csr_forward_of_one_system_is_linsys():
    sol = StubSolver(S, C, K, 1)
    ins = [torch.randn(1, n, dtype=torch.float64, requires_grad=True) for n in (sol.N, sol.sizes["sk"], 5, 4)]
    ag._KktSolve.apply(ag._CSR, IDX, sol, *OPTS, *ins)
    assert sol.calls == ["linsys", "check_status", "get_option(assembly_gen)"]


@pytest.mark.parametrize("name", FORMS)
def test_backward_on_a_fresh_assembly(name):
    sol, ins, lam, dz = run_forward(name)
    sol.calls.clear()
    (lam.sum() + dz.sum()).backward()
    _, _, _, _, resolve, grads = FORMS[name]
    assert sol.calls == FRESH + ["reserve_rhs", resolve, "check_status"] + grads
    assert all(t.grad is not None and t.grad.shape == t.shape for t in ins.values())


@pytest.mark.parametrize("name", FORMS)
def test_backward_on_a_stale_assembly_repeats_the_forward_once(name):
    sol, ins, lam, dz = run_forward(name)
    sol.calls.clear()
    sol.gen += 1                                          # another solve replaced the assembly
    (lam.sum() + dz.sum()).backward()
    _, _, _, fwd, resolve, grads = FORMS[name]
    assert sol.calls == STALE + [fwd, "check_status", "reserve_rhs", resolve, "check_status"] + grads
    assert torch.all(lam == 0.5) and torch.all(dz == -2.0)          # the repeat wrote into the solver's own buffers


class _DropGrad(torch.autograd.Function):
    """identity whose backward hands on no gradient"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("name", FORMS)
def test_backward_without_incoming_gradients_calls_nothing(name):
    sol, ins, lam, dz = run_forward(name)
    sol.calls.clear()
    (_DropGrad.apply(lam).sum() + _DropGrad.apply(dz).sum()).backward()
    assert sol.calls == []
    assert all(t.grad is None for t in ins.values())


@pytest.mark.parametrize("name", FORMS)
def test_one_incoming_gradient_is_enough(name):
    sol, ins, lam, dz = run_forward(name)
    sol.calls.clear()
    dz.sum().backward()
    _, _, _, _, resolve, grads = FORMS[name]
    assert sol.calls == FRESH + ["reserve_rhs", resolve, "check_status"] + grads


@pytest.mark.parametrize("name", FORMS)
def test_no_gradient_call_when_no_matrix_gradient_is_wanted(name):
    sol, ins, lam, dz = run_forward(name, need=("g", "c"))
    sol.calls.clear()
    (lam.sum() + dz.sum()).backward()
    assert sol.calls == FRESH + ["reserve_rhs", FORMS[name][4], "check_status"]
    assert ins["g"].grad is not None and ins["c"].grad is not None
    assert all(ins[k].grad is None for k in FORMS[name][2])


@pytest.mark.parametrize("need, grads", [(("G",), ["kkt_grad_blocks"]), (("C",), ["kkt_grad_blocks"]), (("M",), ["kkt_grad_cross"]),
                                         (("G", "M"), ["kkt_grad_blocks", "kkt_grad_cross"]), (("g",), [])])
def test_cross_gradient_calls_follow_what_is_wanted(need, grads):
    sol, ins, lam, dz = run_forward("blocks_cross", need=need)
    sol.calls.clear()
    (lam.sum() + dz.sum()).backward()
    assert sol.calls == FRESH + ["reserve_rhs", "solve_rhs_cross", "check_status"] + grads
    assert [k for k, t in ins.items() if t.grad is not None] == [k for k in ins if k in need]


@pytest.mark.parametrize("name, need, grads", [("blocks", ("G",), ["kkt_grad_blocks"]), ("csr", ("nnzC",), ["kkt_grad_csr"]),
                                               ("csr_cross", ("nnzG",), ["kkt_grad_csr_cross"])])
def test_one_matrix_gradient_is_one_gradient_call(name, need, grads):
    sol, ins, lam, dz = run_forward(name, need=need)
    sol.calls.clear()
    (lam.sum() + dz.sum()).backward()
    assert sol.calls == FRESH + ["reserve_rhs", FORMS[name][4], "check_status"] + grads
    assert [k for k, t in ins.items() if t.grad is not None] == list(need)


def test_an_empty_M_gets_no_gradient_call():
    sol, ins, lam, dz = run_forward("blocks_cross", K=1)             # K = 1: M has no entries
    assert ins["M"].numel() == 0
    sol.calls.clear()
    (lam.sum() + dz.sum()).backward()
    assert sol.calls == FRESH + ["reserve_rhs", "solve_rhs_cross", "check_status", "kkt_grad_blocks"]
    assert ins["M"].grad is not None and ins["M"].grad.shape == ins["M"].shape


@pytest.mark.parametrize("name", ["blocks_cross", "csr", "csr_cross"])
def test_forward_ad_is_not_built_for_the_other_forms(name):
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError):
            run_forward(name, dual=True)
