"""The KKT gradient kernels (gato_grad.hip) and the autograd layers over them at every compiled shape, at the short horizons,
over more than one workgroup in x and in y, and on CSR patterns with shuffled rows, duplicate columns and structurally empty
rows (tests/csr_patterns.py; their slot map is checked against the scatter on the CPU, tests/test_sweep_refs_cpu.py).

e. grad_blocks_kernel as a function of its four vectors: the formulas (kkt_grad_ref.grads_dense_layout on the same host values:
   1e-14 relative in fp64, 1e-6 in fp32 - the bars of test_csr_gradient_is_bit_identical_to_the_block_gradient), exact symmetry
   of every Q_bar and R_bar block, one output null, and outputs off the 16-byte grid.
f. grad_csr_kernel: every entry bit for bit the block kernel's entry of its slot, 0 for dropped and overwritten entries.
g. kkt_solve and kkt_solve_csr against the dense reference (1e-6 relative with the PCG run to rounding, as
   tests/test_gpu_kkt_grad.py).
Every output buffer starts as NaN, so an entry no thread wrote shows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_polish_ref as P                      # noqa: E402
import csr_patterns as cp                          # noqa: E402
import kkt_grad_ref as ref                         # noqa: E402
from gato_python_amd import _lib, synth            # noqa: E402
from oracle import c_oracle as co                  # noqa: E402
from oracle import gato_oracle as o                # noqa: E402
from test_gpu_kkt_grad import F64_BAR, NAMES, TIGHT, ag, dev, grads_of, weights   # noqa: E402
from test_gpu_parity import rel                    # noqa: E402
from test_gpu_resolve import solver                # noqa: E402

SHAPES = P.SWEEP_SHAPES
DTYPES = [np.float64, np.float32]
DT_IDS = ["float64", "float32"]
shape_id = lambda sh: "%d-%d" % tuple(sh)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def vectors(S, C, K, B, dt, seed=0):
    """(dz [B, N], lam [B, S K], a [B, N], beta [B, S K]): random, rounded to dt, as fp64 host arrays."""
    rng = np.random.default_rng([S, C, K, B, seed])
    N = (S + C) * K - C
    return [rng.standard_normal((B, m)).astype(dt).astype(np.float64) for m in (N, S * K, N, S * K)]


def nan_buffer(sol, n):
    return sol.new(n).fill_(float("nan"))


def run_blocks(sol, vec, G=True, Cc=True):
    """kkt_grad_blocks on the host vectors -> (G_bar [B, G_dense] or None, C_bar [B, C_dense] or None) as host arrays."""
    B = sol.batch
    Gb = nan_buffer(sol, B * sol.sizes["G_dense"]) if G else None
    Cb = nan_buffer(sol, B * sol.sizes["C_dense"]) if Cc else None
    sol.kkt_grad_blocks(*[sol.to_device(v.reshape(-1)) for v in vec], Gb, Cb)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy().reshape(B, -1) for t in (Gb, Cb))


# ---- e. the block kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", [1, 2, 3, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_block_gradients_every_shape(shape, K, dt, B):
    """K = 1: C_dense is empty, so no C output is passed and G alone must be right.  B = 3: the per-system strides 5 K - 1 of 2/1
    and 245 K - 49, 294 (K - 1) of 14/7 are no multiples of four, so fp32 vectors of four wrap from one system into the next."""
    S, C = shape
    sol = solver(S, C, K, dt, batch=B)
    vec = vectors(S, C, K, B, dt)
    has_c = sol.sizes["C_dense"] > 0
    assert has_c == (K > 1)
    Gb, Cb = run_blocks(sol, vec, Cc=has_c)
    bar = 1e-14 if dt == np.float64 else 1e-6
    for b in range(B):
        wG, wC = ref.grads_dense_layout(*[v[b] for v in vec], S, C, K)
        assert np.any(wG != 0) and rel(Gb[b], wG) < bar, (b, rel(Gb[b], wG))
        if has_c:
            assert np.any(wC != 0) and rel(Cb[b], wC) < bar, (b, rel(Cb[b], wC))
        Q, Rr = o.unpack_G(Gb[b], S, C, K)
        assert np.array_equal(Q, np.swapaxes(Q, 1, 2)) and np.array_equal(Rr, np.swapaxes(Rr, 1, 2))   # bit for bit
    # one output null: the other one keeps its bits
    if has_c:
        G_only, none = run_blocks(sol, vec, Cc=False)
        none2, C_only = run_blocks(sol, vec, G=False)
        assert none is None and none2 is None
        assert np.array_equal(G_only, Gb) and np.array_equal(C_only, Cb)
    sol.close()


ALIGN_SHAPES = [(2, 1, 2), (14, 7, 3)]             # G strides 9 and 686, C strides 6 and 588: odd, and even without being a multiple of 4


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", ["G", "C"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("S,C,K", ALIGN_SHAPES, ids=["%d-%d-%d" % c for c in ALIGN_SHAPES])
def test_block_gradients_off_the_16_byte_grid(S, C, K, dt, which, off):
    """One output as a view `off` elements into a larger buffer (fp32: 4, 8, 12 bytes off the 16-byte grid, fp64: 8 bytes or on
    it): the bits of the aligned call, and the slack in front of and behind the view untouched."""
    B, SLACK, SENTINEL = 3, 8, 7.0
    sol = solver(S, C, K, dt, batch=B)
    vec = vectors(S, C, K, B, dt, seed=1)
    want = dict(zip("GC", run_blocks(sol, vec)))
    n = {"G": B * sol.sizes["G_dense"], "C": B * sol.sizes["C_dense"]}
    buf = sol.new(n[which] + SLACK).fill_(SENTINEL)
    other = nan_buffer(sol, n["C" if which == "G" else "G"])
    view = buf[off:off + n[which]]
    assert view.data_ptr() == buf.data_ptr() + off * buf.element_size() and buf.data_ptr() % 16 == 0
    d = [sol.to_device(v.reshape(-1)) for v in vec]
    sol.kkt_grad_blocks(*d, *((view, other) if which == "G" else (other, view)))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:off] == SENTINEL) and np.all(got[off + n[which]:] == SENTINEL)
    assert np.array_equal(got[off:off + n[which]].reshape(B, -1), want[which])
    assert np.array_equal(other.cpu().numpy().reshape(B, -1), want["C" if which == "G" else "G"])
    sol.close()


# ---- f. the CSR kernel over real patterns --------------------------------------------------------------------------------------------
# K = 4, raised where a pattern would have no more than 256 entries (one workgroup in x): 2/1 K = 60, 4/2 K = 8 (K = 4: 94 .. 181
# entries), 6/3 K = 6 (K = 4: the thinned pattern has 247)
CSR_K = {(2, 1): 60, (4, 2): 8, (6, 3): 6, (12, 6): 4, (14, 7): 4, (32, 16): 4}
WG = 256                                           # grad_csr_kernel: entries per workgroup in x; SYS_PER = 8 systems per workgroup in y


@functools.lru_cache(maxsize=None)
def pattern(name, S, C, K):
    s = cp.pattern_system(name, S, C, K)
    sg, sc = ref.csr_slot_map(s.G_row, s.G_col, s.C_row, s.C_col, S, C, K)
    return s, sg, sc, cp.kinds(s, sg, sc)


def check_kinds(name, k):
    assert k["block_row_0"] > 0 and k["identity"] > 0 and k["kept_G"] > 0 and k["kept_C"] > 0, k
    if name in ("duplicates", "combined"):
        assert k["overwritten_G"] > 0 and k["overwritten_C"] > 0, k
    if name in ("empty", "combined"):
        assert k["empty_C_rows"] >= 2 and k["diagonal_only_G_rows"] > 0, k
    if name == "empty":
        assert k["identity_only_C_rows"] > 0, k


def run_csr(sol, s, vec, G=True, Cc=True):
    B, i32 = sol.batch, lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to("cuda:0")
    Gv = nan_buffer(sol, B * len(s.G_col)) if G else None
    Cv = nan_buffer(sol, B * len(s.C_col)) if Cc else None
    sol.kkt_grad_csr(i32(s.G_row), i32(s.G_col), i32(s.C_row), i32(s.C_col), *[sol.to_device(v.reshape(-1)) for v in vec], Gv, Cv)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy().reshape(B, -1) for t in (Gv, Cv))


def by_slot(blocks, slots):
    """[B, dense] gathered through a slot map -> [B, nnz], exactly 0 where the slot is -1."""
    return np.where(slots >= 0, blocks[:, np.maximum(slots, 0)], 0).astype(blocks.dtype)


@pytest.mark.parametrize("B", [1, 9, 17])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(cp.PATTERNS))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_csr_gradients_over_real_patterns(shape, name, dt, B):
    """B = 9, 17: two and three groups of eight systems, the last one partial."""
    S, C = shape
    K = CSR_K[shape]
    s, sg, sc, k = pattern(name, S, C, K)
    assert len(s.G_col) + len(s.C_col) > WG and len(s.C_col) > 0          # at least two workgroups in x, C entries behind the G ones
    check_kinds(name, k)
    sol = solver(S, C, K, dt, batch=B)
    vec = vectors(S, C, K, B, dt, seed=2)
    Gb, Cb = run_blocks(sol, vec)
    Gv, Cv = run_csr(sol, s, vec)
    wantG, wantC = by_slot(Gb, sg), by_slot(Cb, sc)
    assert np.any(wantG != 0) and np.any(wantC != 0)
    assert np.array_equal(Gv, wantG), np.argwhere(Gv != wantG)[:5]
    assert np.array_equal(Cv, wantC), np.argwhere(Cv != wantC)[:5]
    assert not Gv[:, sg < 0].any() and not Cv[:, sc < 0].any()               # dropped and overwritten: exactly 0
    # one output null (nG = 0 moves every C entry to the front of the launch)
    G_only, none = run_csr(sol, s, vec, Cc=False)
    none2, C_only = run_csr(sol, s, vec, G=False)
    assert none is None and none2 is None
    assert np.array_equal(G_only, Gv) and np.array_equal(C_only, Cv)
    sol.close()


# ---- g. the autograd layers ----------------------------------------------------------------------------------------------------------
SOLVE_CASES = [(4, 2, 9), (6, 3, 9), (12, 6, 9), (14, 7, 2), (14, 7, 3), (2, 1, 2)]


@pytest.mark.parametrize("S,C,K", SOLVE_CASES, ids=["%d-%d-%d" % c for c in SOLVE_CASES])
def test_kkt_solve_fp64_at_the_other_shapes_and_short_horizons(S, C, K):
    blocks = synth.make_blocks(S, C, K, seed=3, dense_q=True)
    s = synth.blocks_to_csr(*blocks, rho=1e-3, dense_q=True)
    w1, w2 = weights(s, 4)
    lam, dz, gr = grads_of(blocks, s, w1, w2)
    want = ref.dense_reference(s, w1, w2)
    assert rel(lam, want["lam"]) < F64_BAR and rel(dz, want["dz"]) < F64_BAR
    for n in NAMES:
        assert np.any(want[n] != 0) and rel(gr[n], want[n]) < F64_BAR, (n, rel(gr[n], want[n]))


def systems_on_a_pattern(s0, sg, sc, Bn):
    """Bn systems on the pattern of s0: an entry that wins its slot carries the value a clean system of its own seed has there
    (so the scatter builds that system with the thinned entries zero), every overwritten entry junk; C's identity entries 1."""
    S, C, K = s0.S, s0.C, s0.K
    rng = np.random.default_rng(21)
    out = []
    for b in range(Bn):
        clean = synth.make_system(S, C, K, seed=600 + b, dense_q=True)
        Gd, Cd = co.convert(*clean.csr_args()[:6], S, C, K, 0.0, np.float64)
        Gv = np.where(sg >= 0, Gd[np.maximum(sg, 0)], rng.standard_normal(len(sg)))
        Cv = np.where(sc >= 0, Cd[np.maximum(sc, 0)], rng.standard_normal(len(sc)))
        n = S + C
        rowC = np.repeat(np.arange(S * K), np.diff(s0.C_row))
        Cv[(rowC < S) | (s0.C_col // n > rowC // S - 1)] = 1.0
        out.append(synth.KKTSystem(S, C, K, s0.G_row, s0.G_col, Gv, s0.C_row, s0.C_col, Cv, clean.g, clean.c, clean.rho))
    return out


@pytest.mark.parametrize("S,C,K", [(4, 2, 4), (14, 7, 4)], ids=["4-2-4", "14-7-4"])
def test_kkt_solve_csr_nine_systems_on_the_combined_pattern(S, C, K):
    Bn = 9
    s0, sg, sc, k = pattern("combined", S, C, K)
    check_kinds("combined", k)
    systems = systems_on_a_pattern(s0, sg, sc, Bn)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda:0")
    stack = lambda name: np.stack([getattr(x, name) for x in systems])
    Gv, Cv, g, c = (dev(stack(n)) for n in ("G_val", "C_val", "g", "c"))
    lam, dz = ag().kkt_solve_csr(i32(s0.G_row), i32(s0.G_col), Gv, i32(s0.C_row), i32(s0.C_col), Cv, g, c, rho=s0.rho, **TIGHT)
    W = [weights(x, 40 + b) for b, x in enumerate(systems)]
    w1, w2 = np.stack([w[0] for w in W]), np.stack([w[1] for w in W])
    ((dz * dev(w1, grad=False)).sum() + (lam * dev(w2, grad=False)).sum()).backward()
    for b, x in enumerate(systems):
        want = ref.dense_reference(x, W[b][0], W[b][1], scatter=True)
        gG, gC = Gv.grad[b].cpu().numpy(), Cv.grad[b].cpu().numpy()
        assert rel(lam[b].detach().cpu().numpy(), want["lam"]) < F64_BAR and rel(dz[b].detach().cpu().numpy(), want["dz"]) < F64_BAR
        assert np.any(want["G_val"] != 0) and np.any(want["C_val"] != 0)
        assert rel(gG, want["G_val"]) < F64_BAR and rel(gC, want["C_val"]) < F64_BAR, (b, rel(gG, want["G_val"]), rel(gC, want["C_val"]))
        assert rel(g.grad[b].cpu().numpy(), want["a"]) < F64_BAR and rel(c.grad[b].cpu().numpy(), want["beta"]) < F64_BAR
        assert np.all(gG[sg < 0] == 0) and np.all(gC[sc < 0] == 0)             # dropped and overwritten entries: exactly 0
