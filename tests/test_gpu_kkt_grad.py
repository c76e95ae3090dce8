"""torch autograd through the KKT solve (gato_python_amd.kkt_solve / kkt_solve_csr, gato_kkt_grad_* in gato_grad.hip).

The reference for every gradient is tests/kkt_grad_ref.py: the formulas of DESIGN.md section 3.6 on the dense fp64 forward and
adjoint solves.  fp64 gradients are held to 1e-6 relative; fp32 ones beside the same formulas on the fp32 oracle's solves."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kkt_grad_ref as ref                         # noqa: E402
from f32_parity import check_f32                   # noqa: E402
from gato_python_amd import _lib, synth            # noqa: E402
from oracle import gato_oracle as o                # noqa: E402
from test_gpu_parity import rel                    # noqa: E402
from test_gpu_resolve import tol_mi                # noqa: E402

NAMES = ("Q", "R", "A", "B", "q", "r", "c")
F64_BAR = 1e-6
# fp64 against the DENSE solve: the PCG runs to rounding (eta = r.Pinv r below 1e-20) instead of tol_mi's 1e-10, which is a
# bar for comparing iterates with the oracle's iterates, not with the exact solution
TIGHT = dict(exit_tol=1e-20, max_iters=1000)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def ag():
    from gato_python_amd import autograd
    return autograd


def dev(a, dt=torch.float64, grad=True):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0", requires_grad=grad)


def system(case):
    S, C, K, seed, dq = case
    if (S, C, K) == (2, 1, 5) and seed is None:
        s = synth.pendulum_system()
        return s, ref.blocks_of(s)
    blocks = synth.make_blocks(S, C, K, seed=seed, dense_q=dq)
    return synth.blocks_to_csr(*blocks, rho=1e-3, dense_q=dq), blocks


def weights(s, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(s.N), rng.standard_normal(s.S * s.K)


def grads_of(blocks, s, w1, w2, dt=torch.float64, tol=None, mi=None, use_dz=True):
    """kkt_solve forward + backward of L = w1.dz + w2.lam -> (lam, dz, {name: grad}) as numpy."""
    t = [dev(b, dt) for b in blocks]
    tol_, mi_ = (TIGHT["exit_tol"], TIGHT["max_iters"]) if dt == torch.float64 else tol_mi(np.float32)
    lam, dz = ag().kkt_solve(*t, rho=s.rho, exit_tol=tol if tol is not None else tol_,
                             max_iters=mi if mi is not None else mi_)
    L = (lam * dev(w2, dt, False)).sum() + ((dz * dev(w1, dt, False)).sum() if use_dz else 0)
    L.backward()
    return lam.detach().cpu().numpy(), dz.detach().cpu().numpy(), {n: x.grad.cpu().numpy() for n, x in zip(NAMES, t)}


CASES = [(2, 1, 5, None, False), (14, 7, 50, 0, False), (14, 7, 512, 1, False), (32, 16, 12, 5, True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d/%d/%d" % c[:3])
def test_kkt_solve_fp64_against_the_dense_reference(case):
    s, blocks = system(case)
    w1, w2 = weights(s, 1)
    lam, dz, gr = grads_of(blocks, s, w1, w2)
    want = ref.dense_reference(s, w1, w2)
    assert rel(lam, want["lam"]) < F64_BAR and rel(dz, want["dz"]) < F64_BAR
    for n in NAMES:
        assert rel(gr[n], want[n]) < F64_BAR, (n, rel(gr[n], want[n]))
    sol = ag()._SOLVERS[(s.S, s.C, s.K, 1, torch.float64, 0)]
    if s.K == 512:
        assert sol.get_option("last_groups") > 1            # the multi-workgroup resident launch (forward and adjoint)
    if (s.S, s.K) == (14, 50):
        assert sol.get_option("last_groups") == 1


def test_directional_finite_differences_of_the_gpu_forward():
    """<grad, D> against the central difference of the GPU's own fp64 solve, symmetric directions in Q and R."""
    s, blocks = system((14, 7, 8, 3, True))
    w1, w2 = weights(s, 2)
    kw = dict(rho=s.rho, **TIGHT)                                   # converged to rounding: smooth in eps
    t = [dev(b) for b in blocks]
    lam, dz = ag().kkt_solve(*t, **kw)
    ((dz * dev(w1, grad=False)).sum() + (lam * dev(w2, grad=False)).sum()).backward()
    rng = np.random.default_rng(5)
    for _ in range(3):
        D = [rng.standard_normal(b.shape) for b in blocks]
        D[0] = 0.5 * (D[0] + np.swapaxes(D[0], 1, 2))
        D[1] = 0.5 * (D[1] + np.swapaxes(D[1], 1, 2))
        an = sum(float((x.grad.cpu().numpy() * d).sum()) for x, d in zip(t, D))
        eps = 1e-5

        def L(sign):
            with torch.no_grad():
                lp, dp = ag().kkt_solve(*[dev(b + sign * eps * d, grad=False) for b, d in zip(blocks, D)], **kw)
            return float(dp.cpu().numpy() @ w1 + lp.cpu().numpy() @ w2)
        fd = (L(1) - L(-1)) / (2 * eps)
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (fd, an)


def test_gradcheck():
    s, blocks = system((2, 1, 6, 4, False))
    kw = dict(rho=s.rho, **TIGHT)
    base = [dev(b, grad=False) for b in blocks]

    def f_vec(q, r, c):
        return ag().kkt_solve(base[0], base[1], base[2], base[3], q, r, c, **kw)

    assert torch.autograd.gradcheck(f_vec, (dev(blocks[4]), dev(blocks[5]), dev(blocks[6])), eps=1e-6, atol=1e-5, rtol=1e-4)

    def f_q(P):
        return ag().kkt_solve(0.5 * (P + P.transpose(-1, -2)), *base[1:], **kw)

    assert torch.autograd.gradcheck(f_q, (dev(blocks[0]),), eps=1e-6, atol=1e-5, rtol=1e-4)

    def f_ab(A, B):
        return ag().kkt_solve(base[0], base[1], A, B, *base[4:], **kw)

    assert torch.autograd.gradcheck(f_ab, (dev(blocks[2]), dev(blocks[3])), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_batch_of_64_systems():
    S, C, K, Bn = 14, 7, 20, 64
    per = [synth.make_blocks(S, C, K, seed=200 + b) for b in range(Bn)]
    stacked = [np.stack([p[i] for p in per]) for i in range(7)]
    t = [dev(x) for x in stacked]
    rng = np.random.default_rng(9)
    N = (S + C) * K - C
    w1, w2 = rng.standard_normal((Bn, N)), rng.standard_normal((Bn, S * K))
    lam, dz = ag().kkt_solve(*t, rho=1e-3, **TIGHT)
    assert lam.shape == (Bn, S * K) and dz.shape == (Bn, N)
    ((dz * dev(w1, grad=False)).sum() + (lam * dev(w2, grad=False)).sum()).backward()
    for b in range(Bn):
        s = synth.blocks_to_csr(*per[b], rho=1e-3)
        want = ref.dense_reference(s, w1[b], w2[b])
        for n, x in zip(NAMES, t):
            assert rel(x.grad[b].cpu().numpy(), want[n]) < F64_BAR, (b, n)


def odd_csr_systems(Bn):
    """The pendulum pattern with a duplicated G column, an unsorted C row holding an explicit zero and the identity entry
    first, and a duplicated C column (test_kkt_grad_cpu.odd_pendulum), with Bn different value sets."""
    from test_kkt_grad_cpu import odd_pendulum
    base = odd_pendulum()
    rng = np.random.default_rng(11)
    out = []
    for b in range(Bn):
        Gv = base.G_val * (1 + 0.2 * rng.random(base.G_val.shape)) if b else base.G_val.copy()
        Cv = base.C_val + (0.05 * rng.standard_normal(base.C_val.shape)) * (base.C_val != 0) if b else base.C_val.copy()
        out.append(synth.KKTSystem(base.S, base.C, base.K, base.G_row, base.G_col, Gv, base.C_row, base.C_col, Cv,
                                   base.g + 0.1 * b, base.c + 0.01 * b, base.rho))
    return out


@pytest.mark.parametrize("Bn", [1, 3])
def test_kkt_solve_csr_against_the_scatter_reference(Bn):
    systems = odd_csr_systems(Bn)
    s0 = systems[0]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda:0")
    stack = (lambda name: np.stack([getattr(x, name) for x in systems])) if Bn > 1 else (lambda name: getattr(s0, name))
    Gv, Cv, g, c = (dev(stack(n)) for n in ("G_val", "C_val", "g", "c"))
    lam, dz = ag().kkt_solve_csr(i32(s0.G_row), i32(s0.G_col), Gv, i32(s0.C_row), i32(s0.C_col), Cv, g, c, rho=s0.rho,
                                 **TIGHT)
    W = [weights(x, 20 + b) for b, x in enumerate(systems)]
    w1 = np.stack([w[0] for w in W]) if Bn > 1 else W[0][0]
    w2 = np.stack([w[1] for w in W]) if Bn > 1 else W[0][1]
    ((dz * dev(w1, grad=False)).sum() + (lam * dev(w2, grad=False)).sum()).backward()
    sg, sc = ref.csr_slot_map(s0.G_row, s0.G_col, s0.C_row, s0.C_col, s0.S, s0.C, s0.K)
    for b, x in enumerate(systems):
        want = ref.dense_reference(x, W[b][0], W[b][1], scatter=True)
        pick = (lambda t: t.grad[b]) if Bn > 1 else (lambda t: t.grad)
        gG, gC = pick(Gv).cpu().numpy(), pick(Cv).cpu().numpy()
        assert rel(gG, want["G_val"]) < F64_BAR and rel(gC, want["C_val"]) < F64_BAR
        assert rel(pick(g).cpu().numpy(), want["a"]) < F64_BAR and rel(pick(c).cpu().numpy(), want["beta"]) < F64_BAR
        assert np.all(gG[sg < 0] == 0) and np.all(gC[sc < 0] == 0)      # dropped and overwritten entries: exactly 0
        assert gC[s0.C_row[2] + 2] != 0                                    # the explicit zero carries its gradient


def test_csr_gradient_is_bit_identical_to_the_block_gradient():
    """gato_kkt_grad_csr and gato_kkt_grad_blocks on the same four vectors: each CSR entry equals the block entry of its slot
    bit for bit, batched, fp64 and fp32."""
    from gato_python_amd.solver import Solver
    for npdt in (np.float64, np.float32):
        systems = odd_csr_systems(4)
        sol = Solver(2, 1, 5, npdt, batch=4)
        d = sol.upload_batch(systems)
        tol, mi = tol_mi(npdt)
        lam, dz, its = sol.new(4 * 10), sol.new(4 * sol.N), sol.new(4, torch.int32)
        sol.linsys_batched(*d, tol, mi, systems[0].rho, lam, dz, its)
        rng = np.random.default_rng(3)
        beta, a, _ = sol.solve_rhs(sol.to_device(rng.standard_normal(4 * sol.N)), sol.to_device(rng.standard_normal(40)), tol, mi)
        Gb, Cb = sol.new(4 * sol.sizes["G_dense"]), sol.new(4 * sol.sizes["C_dense"])
        sol.kkt_grad_blocks(dz, lam, a, beta, Gb, Cb)
        nG, nC = d[2].numel() // 4, d[5].numel() // 4
        Gv, Cv = sol.new(4 * nG), sol.new(4 * nC)
        sol.kkt_grad_csr(d[0], d[1], d[3], d[4], dz, lam, a, beta, Gv, Cv)
        torch.cuda.synchronize()
        s0 = systems[0]
        sg, sc = ref.csr_slot_map(s0.G_row, s0.G_col, s0.C_row, s0.C_col, 2, 1, 5)
        Gb, Cb, Gv, Cv = (x.cpu().numpy() for x in (Gb, Cb, Gv, Cv))
        for b in range(4):
            blkG = Gb[b * sol.sizes["G_dense"]:(b + 1) * sol.sizes["G_dense"]]
            blkC = Cb[b * sol.sizes["C_dense"]:(b + 1) * sol.sizes["C_dense"]]
            eG = np.where(sg >= 0, blkG[np.maximum(sg, 0)], 0).astype(npdt)
            eC = np.where(sc >= 0, blkC[np.maximum(sc, 0)], 0).astype(npdt)
            assert np.array_equal(Gv[b * nG:(b + 1) * nG], eG) and np.array_equal(Cv[b * nC:(b + 1) * nC], eC), (npdt, b)
        # the block kernel against the formulas on the same vectors (host fp64 on the device's vectors)
        h = lambda x: x.cpu().numpy().astype(np.float64)
        for b in range(4):
            sl = lambda v, m: h(v)[b * m:(b + 1) * m]
            wG, wC = ref.grads_dense_layout(sl(dz, sol.N), sl(lam, 10), sl(a, sol.N), sl(beta, 10), 2, 1, 5)
            bar = 1e-14 if npdt == np.float64 else 1e-6
            assert rel(Gb[b * sol.sizes["G_dense"]:(b + 1) * sol.sizes["G_dense"]], wG) < bar
            assert rel(Cb[b * sol.sizes["C_dense"]:(b + 1) * sol.sizes["C_dense"]], wC) < bar
        sol.close()


def test_block_kernel_unaligned_and_odd_lengths():
    """14/7: the per-system strides are odd, so vector stores straddle systems; an output pointer off the 16-byte grid takes
    the scalar stores.  Both against the formulas."""
    from gato_python_amd.solver import Solver
    Bn, K = 3, 9
    sol = Solver(14, 7, K, np.float64, batch=Bn)
    rng = np.random.default_rng(8)
    vec = [sol.to_device(rng.standard_normal(Bn * m)) for m in (sol.N, 14 * K, sol.N, 14 * K)]
    nG, nC = Bn * sol.sizes["G_dense"], Bn * sol.sizes["C_dense"]
    Gbuf, Cbuf = sol.new(nG + 1), sol.new(nC + 1)
    sol.kkt_grad_blocks(*vec, Gbuf[:nG], Cbuf[1:])                  # Cbuf[1:] is 8 bytes off the 16-byte grid
    torch.cuda.synchronize()
    h = [v.cpu().numpy() for v in vec]
    for b in range(Bn):
        sl = lambda i, m: h[i][b * m:(b + 1) * m]
        wG, wC = ref.grads_dense_layout(sl(0, sol.N), sl(1, 14 * K), sl(2, sol.N), sl(3, 14 * K), 14, 7, K)
        G = Gbuf[:nG].cpu().numpy()[b * sol.sizes["G_dense"]:(b + 1) * sol.sizes["G_dense"]]
        Cc = Cbuf[1:].cpu().numpy()[b * sol.sizes["C_dense"]:(b + 1) * sol.sizes["C_dense"]]
        assert rel(G, wG) < 1e-14 and rel(Cc, wC) < 1e-14
    sol.close()


def test_fp32_beside_the_fp32_oracle():
    """err_gpu <= 2 err_oracle32 + 5e-6 (tests/f32_parity.py), truth = the dense fp64 reference on the fp32-rounded inputs;
    the oracle side = the formulas on oracle.linsys_solve(float32) for the forward and for the adjoint right-hand side."""
    S, C, K = 14, 7, 50
    blocks = [b.astype(np.float32).astype(np.float64) for b in synth.make_blocks(S, C, K, seed=0)]
    s = synth.blocks_to_csr(*blocks, rho=np.float64(np.float32(1e-3)))
    w1, w2 = [w.astype(np.float32).astype(np.float64) for w in weights(s, 6)]
    _, _, gr = grads_of(blocks, s, w1, w2, dt=torch.float32)
    truth = ref.dense_reference(s, w1, w2)
    tol, mi = tol_mi(np.float32)
    lam_o, dz_o, _ = o.linsys_solve(*s.csr_args(), S, C, K, tol, mi, s.rho, dtype=np.float32)
    beta_o, a_o, _ = o.linsys_solve(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, w1, w2, S, C, K, tol, mi, s.rho,
                                    dtype=np.float32)
    orc = ref.grads_math(dz_o, lam_o, a_o, beta_o, S, C, K)
    for n in NAMES:
        check_f32(f"kkt grad {n} 14/7/50", gr[n], orc[n], truth[n])


def test_stale_assembly_and_retain_graph():
    """Two forwards on one shape, then the backward of the first: its assembly was replaced, so the backward re-solves it."""
    s1, b1 = system((14, 7, 50, 30, False))
    s2, b2 = system((14, 7, 50, 31, False))
    w1, w2 = weights(s1, 12)
    t1, t2 = [dev(b) for b in b1], [dev(b) for b in b2]
    lam1, dz1 = ag().kkt_solve(*t1, rho=s1.rho, **TIGHT)
    sol = ag()._SOLVERS[(14, 7, 50, 1, torch.float64, 0)]
    gen1 = sol.get_option("assembly_gen")
    lam2, dz2 = ag().kkt_solve(*t2, rho=s2.rho, **TIGHT)
    assert sol.get_option("assembly_gen") == gen1 + 1
    assert lam1.data_ptr() != lam2.data_ptr() and lam1.data_ptr() != sol.buffer_ptr(6)     # fresh outputs
    L1 = (dz1 * dev(w1, grad=False)).sum() + (lam1 * dev(w2, grad=False)).sum()
    L1.backward(retain_graph=True)
    first = {n: x.grad.clone() for n, x in zip(NAMES, t1)}
    assert sol.get_option("assembly_gen") == gen1 + 2                                       # the re-run of the first solve
    want = ref.dense_reference(s1, w1, w2)
    for n in NAMES:
        assert rel(first[n].cpu().numpy(), want[n]) < F64_BAR, n
    for x in t1:
        x.grad = None
    L1.backward()
    for n, x in zip(NAMES, t1):
        assert torch.equal(x.grad, first[n]), n
    for x in t2:
        assert x.grad is None


def test_only_lambda_used_and_no_grad_inputs():
    s, blocks = system((14, 7, 50, 40, False))
    w1, w2 = weights(s, 13)
    _, _, gr = grads_of(blocks, s, w1, w2, use_dz=False)
    want = ref.dense_reference(s, np.zeros(s.N), w2)
    for n in NAMES:
        assert rel(gr[n], want[n]) < F64_BAR, n
    t = [dev(b, grad=False) for b in blocks]
    lam, dz = ag().kkt_solve(*t, rho=s.rho, exit_tol=1e-10, max_iters=300)
    assert not lam.requires_grad and not dz.requires_grad and lam.grad_fn is None


def test_zero_upstream_gradient_of_one_system():
    """A system of a batch whose upstream gradient is all zero gets exactly zero gradients (its adjoint right-hand side is
    zero: no 0 / 0 of the PCG leaks out), the others their reference."""
    per = [synth.make_blocks(14, 7, 20, seed=500 + b) for b in range(2)]
    t = [dev(np.stack([p[i] for p in per])) for i in range(7)]
    s0 = synth.blocks_to_csr(*per[0], rho=1e-3)
    w1, w2 = weights(s0, 14)
    W1, W2 = np.stack([w1, np.zeros_like(w1)]), np.stack([w2, np.zeros_like(w2)])
    lam, dz = ag().kkt_solve(*t, rho=1e-3, **TIGHT)
    ((dz * dev(W1, grad=False)).sum() + (lam * dev(W2, grad=False)).sum()).backward()
    want = ref.dense_reference(s0, w1, w2)
    for n, x in zip(NAMES, t):
        assert rel(x.grad[0].cpu().numpy(), want[n]) < F64_BAR, n
        assert bool((x.grad[1] == 0).all()), n


def test_input_errors_on_the_gpu():
    s, blocks = system((2, 1, 5, 0, False))
    t = [dev(b) for b in blocks]
    kw = dict(rho=1e-3, exit_tol=1e-10, max_iters=100)
    with pytest.raises(ValueError, match="dtype"):
        ag().kkt_solve(*t[:6], t[6].float(), **kw)
    with pytest.raises(ValueError, match="GPU only"):
        ag().kkt_solve(*t[:6], t[6].detach().cpu(), **kw)
    with pytest.raises(ValueError):
        ag().kkt_solve(t[0], t[1], t[2], t[3][:, :, :0], *t[4:], **kw)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda:0")
    bad_col = s.G_col.copy()
    bad_col[3] = -1
    with pytest.raises(ValueError, match="outside"):
        ag().kkt_solve_csr(i32(s.G_row), i32(bad_col), dev(s.G_val), i32(s.C_row), i32(s.C_col), dev(s.C_val), dev(s.g),
                           dev(s.c), **kw)


def test_c_abi_refusals_and_assembly_gen():
    from gato_python_amd.solver import Solver
    L = _lib.lib()
    S, C, K = 14, 7, 50
    s = synth.make_system(S, C, K, seed=21)
    sol = Solver(S, C, K, np.float64)
    d = sol.upload_system(s)
    v = [sol.new(sol.N), sol.new(S * K), sol.new(sol.N), sol.new(S * K)]
    for x in v:
        x.fill_(1.0)
    Gb, Cb = sol.new(sol.sizes["G_dense"]), sol.new(sol.sizes["C_dense"])
    Gv, Cv = sol.new(d[2].numel()), sol.new(d[5].numel())
    p = lambda x: ct.c_void_p(x.data_ptr()) if x is not None else None

    def blocks(*vv, G=Gb, Cc=Cb):
        _lib.check(L.gato_kkt_grad_blocks(sol._h, *[p(x) for x in vv], p(G), p(Cc), sol._stream()))

    def csr(*vv, G=Gv, Cc=Cv):
        _lib.check(L.gato_kkt_grad_csr(sol._h, p(d[0]), p(d[1]), Gv.numel(), p(d[3]), p(d[4]), Cv.numel(), *[p(x) for x in vv],
                                       p(G), p(Cc), sol._stream()))

    for fn in (blocks, csr):
        for i in range(4):
            with pytest.raises(_lib.GatoError) as e:
                fn(*[None if j == i else v[j] for j in range(4)])
            assert e.value.code == -1
        with pytest.raises(_lib.GatoError) as e:
            fn(*v, G=None, Cc=None)
        assert e.value.code == -1
    blocks(*v, G=None)                                                   # one output is enough
    csr(*v, Cc=None)
    _lib.check(L.gato_cluster_create(sol._h, 0, 1, None))
    for fn in (blocks, csr):
        with pytest.raises(_lib.GatoError) as e:
            fn(*v)
        assert e.value.code == -1
    _lib.check(L.gato_cluster_destroy(sol._h))
    # assembly_gen: +1 per whole solve, unchanged by a re-solve and by the gradient entries
    g0 = sol.get_option("assembly_gen")
    sol.linsys(*d, 1e-10, 300, s.rho, sol.new(S * K), sol.new(sol.N))
    torch.cuda.synchronize()
    assert sol.get_option("assembly_gen") == g0 + 1
    sol.solve_rhs(d[6], d[7], 1e-10, 300)
    blocks(*v)
    torch.cuda.synchronize()
    assert sol.get_option("assembly_gen") == g0 + 1
    sol.linsys(*d, 1e-10, 300, s.rho, sol.new(S * K), sol.new(sol.N))
    torch.cuda.synchronize()
    assert sol.get_option("assembly_gen") == g0 + 2
    sol.close()
