"""The pure parts of gato_python_amd.solver on CPU tensors, without a library handle: the operand table against the closed forms of
the layouts, check_operands' messages against the literal messages the methods raised before there was one checker, and the two
re-solve rules (zero_rhs, hard_active) and bound_tangents against the expressions they replaced in Solver.tangents,
Solver.tangents_cross, autograd._adjoint and _BoxQPLayer.backward, written out here."""
import itertools

import pytest
import torch

from gato_python_amd import solver as sv

F64 = torch.float64


# ---- the operand table ---------------------------------------------------------------------------------------------------------
BLOCKS = dict(G="Gb G_blocks G_dot G_out Gbar", C="Cb C_blocks C_dot C_out Cbar", M="Mb M_blocks M_dot M_out Mbar")
VECTORS = dict(N="g x z y lo hi dz adz a xbar gp tg g_dot lo_dot hi_dot w_dot m_dot soft_weight soft_cap mu xc xplus lo2 hi2 w2 lo_bar "
                 "hi_bar w_bar cap_bar act", sk="c lam beta alam c_dot tc", one="status iters w v_prev")
STATED = "G_val C_val G_row G_col C_row C_col"            # their callers state the size


@pytest.mark.parametrize("K", [3, 1])
def test_every_operand_has_the_entries_of_its_layout(K):
    S, C, B, R = 2, 1, 2, 2
    per = dict(G=(S * S + C * C) * K - C * C, C=(S * S + S * C) * (K - 1), M=(K - 1) * S * C, N=(S + C) * K - C, sk=S * K, one=1)
    if K == 1:
        assert per["M"] == 0 and per["C"] == 0
    sizes = sv.operand_sizes(S, C, K)
    assert sizes["M"] == per["M"] and sizes["N"] == per["N"]
    want = {name: per[key] for key, names in {**BLOCKS, **VECTORS}.items() for name in names.split()}
    assert set(want) | set(STATED.split()) == set(sv.OPERANDS)
    table = sv.operand_table(sizes, B, F64)
    for name, n in want.items():
        assert table[name][0] == B * n, name
    assert all(sv.OPERANDS[name][0] is None for name in STATED.split())
    good = {name: on_device(B * R * n, dtype=table[name][1]) for name, n in want.items() if n}        # and R multiplies it
    sv.check_operands(table, "any", good, R)


def test_the_dtype_kinds():
    kinds = {name: kind for name, (_, kind) in sv.OPERANDS.items()}
    other = dict(act="int8", status="int32", iters="int32", w="float64", v_prev="float64", G_row="index", G_col="index", C_row="index",
                 C_col="index")
    assert kinds == {name: other.get(name, "value") for name in kinds}


# ---- the checker's messages ----------------------------------------------------------------------------------------------------
B, R = 2, 2
TABLE = sv.operand_table(sv.operand_sizes(2, 1, 3), B, F64)              # G_dense 14, C_dense 12, M 4, N 8, sk 6


def check(what, R=1, **kw):
    """check_operands on TABLE: the keywords that name an operand are the operands, the others the checker's own."""
    operands = {k: kw.pop(k) for k in list(kw) if k in sv.OPERANDS}
    sv.check_operands(TABLE, what, operands, R, **kw)


class OnDevice(torch.Tensor):
    """A CPU tensor that says it is a CUDA one: what passes the check, and every reason to fail but the device on its own."""
    is_cuda = property(lambda self: True)


def on_device(*shape, dtype=F64):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


# one operand of each of the six places that held the predicate: (call, the message before the one checker)
MESSAGES = [
    # Solver._check_cross (kkt_grad_cross), a CPU tensor
    (lambda: check("kkt_grad_cross", Mbar=torch.zeros(8, dtype=F64)),
     "kkt_grad_cross: Mbar must be a contiguous torch.float64 CUDA tensor of 8 entries, got torch.float64 (8,) on cpu"),
    # Solver._csr_cross_inputs: a wrong size; any size but none; a non-tensor
    (lambda: check("linsys_cross", entries=dict(G_row=9), G_row=on_device(5, dtype=torch.int32)),
     "linsys_cross: G_row must be a contiguous int32 CUDA tensor of 9 entries, got torch.int32 (5,) on cpu"),
    (lambda: check("cross_prepare_csr", entries=dict(C_col=None), C_col=on_device(0, dtype=torch.int32)),
     "cross_prepare_csr: C_col must be a contiguous int32 CUDA tensor, got torch.int32 (0,) on cpu"),
    (lambda: check("linsys_cross", entries=dict(G_col=None), G_col=[0, 1]),
     "linsys_cross: G_col must be a contiguous int32 CUDA tensor, got list"),
    (lambda: check("linsys_cross", entries=dict(G_val=10), G_val=on_device(12)),
     "linsys_cross: G_val must be a contiguous torch.float64 CUDA tensor of 10 entries, got torch.float64 (12,) on cpu"),
    # Solver.kkt_tangent_rhs, the tangents: a wrong dtype
    (lambda: check("kkt_tangent_rhs", R, G_dot=on_device(56, dtype=torch.float32)),
     "kkt_tangent_rhs: G_dot must be a contiguous torch.float64 CUDA tensor of 56 entries, got torch.float32 (56,) on cpu"),
    # Solver.kkt_tangent_rhs, the outputs: no tail
    (lambda: check("kkt_tangent_rhs", R, got=False, tc=on_device(23)),
     "kkt_tangent_rhs: tc must be a contiguous torch.float64 CUDA tensor of 24 entries"),
    # Solver._check_vecs (box_qp_pdas): a non-contiguous act, a status of the value dtype
    (lambda: check("box_qp_pdas", act=on_device(4, 8, dtype=torch.int8)[:, ::2]),
     "box_qp_pdas: act must be a contiguous torch.int8 CUDA tensor of 16 entries, got torch.int8 (4, 4) on cpu"),
    (lambda: check("box_qp_polish", status=on_device(2)),
     "box_qp_polish: status must be a contiguous torch.int32 CUDA tensor of 2 entries, got torch.float64 (2,) on cpu"),
    (lambda: check("box_qp", lam=None),
     "box_qp: lam must be a contiguous torch.float64 CUDA tensor of 12 entries, got NoneType"),
    # Solver.box_qp_alm_update's w and v_prev: no tail, "float64"
    (lambda: check("box_qp_alm_update", got=False, v_prev=on_device(2, dtype=torch.float32)),
     "box_qp_alm_update: v_prev must be a contiguous float64 CUDA tensor of 2 entries"),
]


@pytest.mark.parametrize("case", range(len(MESSAGES)))
def test_the_messages_are_those_of_the_six_places(case):
    call, want = MESSAGES[case]
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == want


def test_a_good_operand_passes_and_each_reason_fails_alone():
    good = dict(Gb=on_device(28), c=on_device(2, 6), act=on_device(16, dtype=torch.int8), w=on_device(2), status=on_device(2, dtype=torch.int32))
    check("box_qp", **good)
    check("kkt_tangent_rhs", R, g_dot=on_device(32), M_dot=on_device(16), tc=on_device(24))
    check("linsys_cross", entries=dict(G_row=9, G_col=None, G_val=10), G_row=on_device(9, dtype=torch.int32), G_col=on_device(1, dtype=torch.int32),
          G_val=on_device(10))
    for bad in (torch.zeros(28, dtype=F64), on_device(27), on_device(28, dtype=torch.float32), on_device(28, 2)[:, 0], None, 28):
        with pytest.raises(ValueError, match="Gb must be a contiguous"):
            check("box_qp", **dict(good, Gb=bad))
    check("cross_prepare_csr", optional=True, G_out=None, M_out=on_device(8), C_out=None)          # None: not given
    with pytest.raises(ValueError, match="M_out must be"):
        check("cross_prepare_csr", optional=True, G_out=None, M_out=on_device(7))
    with pytest.raises(ValueError, match="box_qp: c must be"):               # the first bad operand in the order given
        check("box_qp", Gb=on_device(28), c=on_device(11), lam=on_device(11))


# ---- the zero rule ---------------------------------------------------------------------------------------------------------------
def rhs_cases(lead):
    """(g [*lead, N], c [*lead, SK]) with pair (0, ..) all zero, and one pair each with a nonzero in g only, in c only, a -0.0 and
    a NaN."""
    N, sk = 8, 6
    out = []
    for where, value in (("none", 0.0), ("g", 2.0), ("c", -3.0), ("g", -0.0), ("c", float("nan")), ("g", float("nan"))):
        g, c = torch.zeros(*lead, N, dtype=F64), torch.zeros(*lead, sk, dtype=F64)
        last = tuple(d - 1 for d in lead)
        if where == "g":
            g[last + (N - 1,)] = value
        elif where == "c":
            c[last + (0,)] = value
        out.append((g, c, value != 0.0))                     # NaN != 0: a NaN counts as nonzero, as ne(0) says
    return out


def test_zero_rule_on_systems():
    """autograd._adjoint: ~(gin.ne(0).any(1) | cin.ne(0).any(1)); _BoxQPLayer.backward's live is its negation."""
    for g, c, nonzero in rhs_cases((2,)):
        want = ~(g.ne(0).any(1) | c.ne(0).any(1))
        assert torch.equal(sv.zero_rhs(g, c), want)
        assert torch.equal(~sv.zero_rhs(g, c), g.ne(0).any(1) | c.ne(0).any(1))
        assert want.tolist() == [True, not nonzero]


def test_zero_rule_on_directions():
    """Solver.tangents and tangents_cross: ~(tg.ne(0).any(2) | tc.ne(0).any(2))."""
    for g, c, nonzero in rhs_cases((2, 2)):
        want = ~(g.ne(0).any(2) | c.ne(0).any(2))
        assert torch.equal(sv.zero_rhs(g, c), want)
        assert want.tolist() == [[True, True], [True, not nonzero]]


# ---- the hard-active rule and the bound's tangent ----------------------------------------------------------------------------------
ACT = torch.tensor([[-2, -1, 0, 1, 2, 1, -1, 0], [0, 0, 2, -2, 1, 1, -1, -1]], dtype=torch.int8)        # [B, N]
WEIGHTS = dict(none=None, zero=torch.zeros(2, 8, dtype=F64),
               some=torch.tensor([[0, 3, 1, 0, 2, 0.5, 0, 0], [1, 0, 0, 0, 0, 4, 4, 0]], dtype=F64))


@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_hard_active_rule(weights):
    """Solver.tangents: hard = act != 0, and with weights hard & ~(w > 0); _BoxQPLayer.backward the same on [B, N]."""
    w = WEIGHTS[weights]
    for shape in ((2, 8), (2, 1, 8)):
        act = ACT.view(shape)
        want = act != 0
        if w is not None:
            want = want & ~(w.view(shape) > 0)
        assert torch.equal(sv.hard_active(act, None if w is None else w.view(shape)), want)
    if weights != "some":
        assert torch.equal(sv.hard_active(ACT, w), ACT != 0)
    else:
        assert sv.hard_active(ACT, w).tolist() == [[True, False, False, True, False, False, True, False],
                                                   [False, False, True, True, True, False, False, True]]


@pytest.mark.parametrize("weights,lo_given,hi_given", list(itertools.product(WEIGHTS, (False, True), (False, True))))
def test_bound_tangents(weights, lo_given, hi_given):
    """Solver.tangents: b_dot = where(act > 0, hi_dot or 0, lo_dot or 0); x_dot = where(hard, b_dot, x_dot)."""
    Bt, Rt, N = 2, 2, 8
    gen = torch.Generator().manual_seed(1)
    x_d, lo_d, hi_d = (torch.randn(Bt, Rt, N, dtype=F64, generator=gen) for _ in range(3))
    lo_d, hi_d = lo_d if lo_given else None, hi_d if hi_given else None
    act, w = ACT.view(Bt, 1, N), WEIGHTS[weights]
    hard = act != 0
    if w is not None:
        hard = hard & ~(w.view(Bt, 1, N) > 0)
    z = torch.zeros((), dtype=F64)
    b_dot = torch.where(act > 0, z if hi_d is None else hi_d, z if lo_d is None else lo_d)
    want = torch.where(hard, b_dot, x_d)
    got = sv.bound_tangents(x_d, act, hard, lo_d, hi_d)
    assert torch.equal(got, want) and got.shape == (Bt, Rt, N)
    assert torch.equal(got[~hard.expand(Bt, Rt, N)], x_d[~hard.expand(Bt, Rt, N)])
