"""The input checks that kkt_solve, box_qp and box_qp_layer share (gato_python_amd.autograd._check_blocks and the bound
helper of gato_python_amd.qp): the exact ValueError text of each entry for the same bad calls, on CPU tensors at S / C / K =
2 / 1 / 3, unbatched and with batch 2.  Every one is raised before any library call."""
import pytest
import torch

ENTRIES = ["kkt_solve", "box_qp", "box_qp_layer"]
QP = ENTRIES[1:]
S, C, K = 2, 1, 3
OPTS = dict(rho=1e-3, exit_tol=1e-10, max_iters=100)
GPU_ONLY = "Q is on cpu: the solve runs on the GPU only (there is no CPU fallback)"


def blocks(batch, K=K):
    lead = () if batch is None else (batch,)
    z = lambda *s: torch.zeros(lead + s, dtype=torch.float64)
    return dict(Q=z(K, S, S), R=z(K - 1, C, C), A=z(K - 1, S, S), B=z(K - 1, S, C), q=z(K, S), r=z(K - 1, C), c=z(K, S)), lead


def call(entry, a, **bounds):
    import gato_python_amd
    if entry == "kkt_solve":
        return gato_python_amd.kkt_solve(*a.values(), **OPTS)
    b = dict(x_lo=-1.0, x_hi=1.0, u_lo=-1.0, u_hi=1.0)
    b.update(bounds)
    return getattr(gato_python_amd, entry)(*a.values(), *b.values(), **OPTS)


def raises(entry, a, text, **bounds):
    with pytest.raises(ValueError) as e:
        call(entry, a, **bounds)
    assert str(e.value) == f"{entry}: {text}"


def sizes(lead):
    """What kkt_solve appends to a shape message."""
    return f" (S = {S}, C = {C}, K = {K}{', batch %d' % lead[0] if lead else ''})"


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_non_tensor_R(entry, batch):
    a, _ = blocks(batch)
    a["R"] = a["R"].numpy()
    raises(entry, a, "R must be a torch.Tensor, got ndarray")


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_Q_that_is_not_square(entry, batch):
    a, lead = blocks(batch)
    a["Q"] = a["Q"][..., :-1]
    if entry == "kkt_solve":
        raises(entry, a, f"Q must be [*, K, S, S], got {lead + (K, S, S - 1)}")
    else:
        raises(entry, a, f"Q must be [*, K, S, S] and R [*, K-1, C, C], got {lead + (K, S, S - 1)} and {lead + (K - 1, C, C)}")


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", ENTRIES)
def test_A_with_one_knot_too_many(entry, batch):
    a, lead = blocks(batch)
    a["A"] = torch.zeros(lead + (K, S, S), dtype=torch.float64)
    raises(entry, a, f"A has shape {lead + (K, S, S)}, want {lead + (K - 1, S, S)}" + (sizes(lead) if entry == "kkt_solve" else ""))


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_q_of_another_batch(entry, batch):
    """A batched q beside unbatched blocks; beside blocks of batch 2, a q of batch 3."""
    a, lead = blocks(batch)
    a["q"] = torch.zeros((batch or 1) + 1, K, S, dtype=torch.float64)
    raises(entry, a, f"q has shape {tuple(a['q'].shape)}, want {lead + (K, S)}" + (sizes(lead) if entry == "kkt_solve" else ""))


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", QP)
def test_one_knot_is_too_few_for_a_qp(entry, batch):
    raises(entry, blocks(batch, K=1)[0], "K = 1: at least two knots")


@pytest.mark.parametrize("batch", [None, 2])
def test_kkt_solve_takes_one_knot(batch):
    """K = 1 passes every shape check of kkt_solve: the first thing wrong with the call is where its tensors live."""
    raises("kkt_solve", blocks(batch, K=1)[0], GPU_ONLY)


@pytest.mark.parametrize("entry", ENTRIES)
def test_good_blocks_fail_only_at_the_device(entry):
    raises(entry, blocks(2)[0], GPU_ONLY)


# ---- the bounds: checked after the blocks' device and dtype, which a CPU run has to let pass ---------------------------------
@pytest.fixture
def any_device(monkeypatch):
    import gato_python_amd.qp as qp
    monkeypatch.setattr(qp, "_common", lambda tensors, what: (None, next(iter(tensors.values())).dtype))


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", QP)
def test_a_bound_that_does_not_broadcast(entry, batch, any_device):
    a, lead = blocks(batch)
    raises(entry, a, f"x_lo of shape (5,) does not broadcast to {lead + (K, S)}", x_lo=torch.zeros(5, dtype=torch.float64))
    raises(entry, a, f"u_hi of shape (4, 2) does not broadcast to {lead + (K - 1, C)}", u_hi=torch.zeros(4, 2, dtype=torch.float64))


@pytest.mark.parametrize("batch", [None, 2])
@pytest.mark.parametrize("entry", QP)
def test_a_bound_of_another_dtype(entry, batch, any_device):
    a, _ = blocks(batch)
    for name in ("x_lo", "x_hi", "u_lo", "u_hi"):
        raises(entry, a, f"{name} must be a torch.float64 tensor on cpu, got torch.float32 on cpu", **{name: torch.zeros(1)})
