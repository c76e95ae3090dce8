"""GPU suite of the stage-cost cross term: gato_cross.hip's four kernels alone, whole solves and
re-solves against the dense KKT with the cross blocks in place, and the gradients of kkt_solve(M=...).

References: tests/cross_ref.py.  fp64 kernel outputs are held per block to 1e-11 relative against the longdouble restatement
(the assembly's bar), solutions to 1e-6 against the dense solve (the parity bar), the gradient kernel to 1e-14 against the
outer products; fp32 is measured beside the float32 restatement.  tests/test_cross_cpu.py asserts on the CPU that every cell
here is positive definite and conditioned well below what these bars would need."""
import ctypes as ct
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cross_ref as X                               # noqa: E402
from f32_parity import check_f32, rel               # noqa: E402
from gato_python_amd import _lib                    # noqa: E402
from oracle import gato_oracle as o                 # noqa: E402

LD = np.longdouble
TIGHT = dict(exit_tol=1e-20, max_iters=1000)        # tests/test_gpu_kkt_grad.py: the PCG runs to rounding
F32_KW = dict(exit_tol=1e-5, max_iters=100)         # the project's fp32 settings (tests/test_gpu_resolve.py: tol_mi)
# fp32 against the dense solve: run to rounding as well.  At the absolute threshold of F32_KW two orders of the sums stop an
# iteration apart (4/2/2: 3 iterations on the device, 4 in the oracle) and one CG iteration of a system this small moves the
# error a hundredfold, so the comparison would measure the stop rule; eta does fall below 1e-12 in float32 (at most 55 iterations here)
F32_TIGHT = dict(exit_tol=1e-12, max_iters=300)
BLOCK_BAR, SOLVE_BAR, GRAD_BAR = 1e-11, 1e-6, 1e-14
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = []                                       # fp32 whole solves: device error beside the restatement's, per cell


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()
    yield
    if len(ACCURACY) == sum(B for _, _, _, B in SOLVES):              # a whole run only: a selection does not replace the record
        try:
            with open(os.path.join(ROOT, "profiles", "cross_accuracy.json"), "w") as f:
                json.dump(dict(margin=10.0, truth="dense float64 solve, refined in longdouble, of the float32-rounded inputs",
                               cells=ACCURACY), f, indent=1)
        except OSError:                                                    # a read-only tree: the record stays as committed
            pass


def ag():
    from gato_python_amd import autograd
    return autograd


def solver(S, C, K, dt=np.float64, batch=1):
    from gato_python_amd.solver import Solver
    return Solver(S, C, K, dt, batch=batch)


def hip():
    return ct.CDLL("libamdhip64.so")


def rounded(cells, dt):
    """The cells with every value rounded to dt (kept in float64): what a device of that dtype is given."""
    r = lambda a: np.asarray(a).astype(dt).astype(np.float64)
    return [(tuple(r(b) for b in blocks), r(M)) for blocks, M in cells]


def dev_inputs(sol, cells, shift=0):
    """Stacked device inputs (G_blocks, M_blocks, C_blocks, g, c) of the cells in the solver's dtype.  shift = 1: every tensor is
    a view one element into its allocation, off the 16-byte grid."""
    packs = [X.pack(*blocks, M) for blocks, M in cells]
    out = []
    for i in (0, 4, 1, 2, 3):
        flat = np.concatenate([p[i] for p in packs]).astype(sol.np_dtype)
        buf = sol.new(flat.size + shift)
        buf[shift:].copy_(torch.from_numpy(flat))
        out.append(buf[shift:])
    return out


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def poison(sol):
    """Every byte of the four parts of the cross work area to 0xFF: NaN in both dtypes, so an entry no kernel writes shows."""
    torch.cuda.synchronize()
    n = dict(G=sol.sizes["G_dense"], C=sol.sizes["C_dense"], W=sol.M_size, g=sol.N)
    for name, per in n.items():
        if per:
            assert hip().hipMemset(ct.c_void_p(sol.cross_buffer_ptr(name)), 0xFF, ct.c_size_t(per * sol.batch * sol.np_dtype.itemsize)) == 0
    assert hip().hipDeviceSynchronize() == 0
    assert all(np.isnan(sol.read_cross(k)).all() for k, per in n.items() if per)


def prepared(sol, cells):
    """cross_prepare of the cells into a poisoned work area, from inputs off the 16-byte grid -> per system dicts of math-shaped
    Q2, R, A2, B, W, g (host arrays in the solver's dtype)."""
    S, C, K, B = sol.S, sol.C, sol.K, sol.batch
    Gb, Mb, Cb, g, _ = dev_inputs(sol, cells, shift=1)
    sol.cross_prepare(Gb, Mb, Cb, g, X.RHO)                               # the first call allocates the area
    poison(sol)
    sol.cross_prepare(Gb, Mb, Cb, g, X.RHO)
    parts = {k: sol.read_cross(k).reshape(B, sol.read_cross(k).size // B) for k in "GCWg"}
    out = []
    for b in range(B):
        Q2, R = o.unpack_G(parts["G"][b], S, C, K)
        A2, Bm = o.unpack_C(parts["C"][b], S, C, K) if K > 1 else (np.zeros((0, S, S)), np.zeros((0, S, C)))
        out.append(dict(Q2=Q2, R=R, A2=A2, B=Bm, W=X.unpack_W(parts["W"][b], S, C, K), g=parts["g"][b]))
    return out


def g_of(t, q2, r, S, C, K):
    """g' in the g layout from the restatement's q2 and the unchanged r."""
    return np.concatenate([np.concatenate([q2[k], r[k]]) for k in range(K - 1)] + [q2[K - 1]])


def blockwise(got, want, what):
    """max over the leading (knot) index of the per-block relative error; a block of zeros must be zeros."""
    worst = 0.0
    for k in range(want.shape[0]):
        assert np.all(np.isfinite(got[k])), (what, k)
        worst = max(worst, rel(got[k], want[k]) if np.abs(want[k]).max() > 0 else float(np.abs(got[k]).max()))
    return worst


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------
KERNEL_CELLS = [(S, C, K) for S, C in X.SHAPES for K in X.KERNEL_K]


@pytest.mark.parametrize("S,C,K", KERNEL_CELLS, ids=["%d-%d-%d" % c for c in KERNEL_CELLS])
def test_prepare_fp64_per_block(S, C, K):
    """W, Q'', A^', g' of three different systems per block against the longdouble restatement; R, B^, the last knot's Q and
    g_x and every g_u are copies, bit for bit; no entry of the poisoned work area is left unwritten."""
    prepare_fp64_case(S, C, K, X.batch_cells(S, C, K, 3, seed=K))


def prepare_fp64_case(S, C, K, cells):
    """The body of test_prepare_fp64_per_block on the given cells -> the worst per-block error of W, Q'', A^' and g'."""
    sol = solver(S, C, K, batch=len(cells))
    worst = 0.0
    for (blocks, M), got in zip(cells, prepared(sol, cells)):
        Q, R, A, B, q, r, c = blocks
        t = X.transform(Q, R, A, B, q, r, M, X.RHO, LD)
        for name, want in (("W", t["W"]), ("Q2", t["Q2"]), ("A2", t["A2"])):
            e = blockwise(got[name], want, name)
            print("prepare %d/%d/%d %s: %.3g" % (S, C, K, name, e))
            assert e < BLOCK_BAR, (name, e)
            worst = max(worst, e)
        n = S + C
        gw = g_of(t, t["q2"], r.astype(LD), S, C, K)
        knots = [slice(k * n, min((k + 1) * n, gw.size)) for k in range(K)]
        e = max(rel(got["g"][s], gw[s]) for s in knots)
        assert e < BLOCK_BAR, ("g'", e)
        worst = max(worst, e)
        assert np.array_equal(got["R"], R) and np.array_equal(got["B"], B) and np.array_equal(got["Q2"][K - 1], Q[K - 1])
        g0 = X.pack(*blocks)[2]
        assert np.array_equal(got["g"][(K - 1) * n:], g0[(K - 1) * n:])
        for k in range(K - 1):
            assert np.array_equal(got["g"][k * n + S:(k + 1) * n], r[k])
    sol.close()
    return worst


@pytest.mark.parametrize("S,C,K", KERNEL_CELLS, ids=["%d-%d-%d" % c for c in KERNEL_CELLS])
def test_prepare_fp32_beside_the_float32_restatement(S, C, K):
    """err_gpu <= 2 err_restatement32 + 5e-6 (tests/f32_parity.py) for W, Q'', A^' and g'; truth = the longdouble restatement
    on the float32-rounded inputs.  The copied blocks are copies."""
    prepare_fp32_case(S, C, K, rounded(X.batch_cells(S, C, K, 3, seed=K), np.float32))


def prepare_fp32_case(S, C, K, cells):
    """The body of test_prepare_fp32_beside_the_float32_restatement on the given (float32-rounded) cells."""
    sol = solver(S, C, K, np.float32, batch=len(cells))
    for b, ((blocks, M), got) in enumerate(zip(cells, prepared(sol, cells))):
        Q, R, A, B, q, r, c = blocks
        assert np.array_equal(got["R"], R.astype(np.float32)) and np.array_equal(got["B"], B.astype(np.float32))
        if K == 1:
            assert np.array_equal(got["Q2"], Q.astype(np.float32)) and np.array_equal(got["g"], q[0].astype(np.float32))
            continue
        truth = X.transform(Q, R, A, B, q, r, M, np.float64(np.float32(X.RHO)), LD)
        r32 = X.transform(Q, R, A, B, q, r, M, X.RHO, np.float32)
        for name in ("W", "Q2", "A2"):
            check_f32("cross prepare %s %d/%d/%d sys %d" % (name, S, C, K, b), got[name], r32[name], truth[name].astype(np.float64))
        check_f32("cross prepare g' %d/%d/%d sys %d" % (S, C, K, b), got["g"], g_of(r32, r32["q2"], r.astype(np.float32), S, C, K),
                  g_of(truth, truth["q2"], r.astype(LD), S, C, K).astype(np.float64))
    sol.close()


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("S,C,K", KERNEL_CELLS, ids=["%d-%d-%d" % c for c in KERNEL_CELLS])
def test_rhs_and_finish_alone(S, C, K, dt):
    """cross_rhs and cross_finish on R = 2 vectors per system from the W that cross_prepare stored, outputs one element off the
    16-byte grid, against the restatement on the device's own W (longdouble for fp64; the float32 restatement beside it for
    fp32).  x-parts and g_u pass through bit for bit."""
    rhs_and_finish_case(S, C, K, dt, rounded(X.batch_cells(S, C, K, 3, seed=K), dt))


def rhs_and_finish_case(S, C, K, dt, cells):
    """The body of test_rhs_and_finish_alone on the given cells (rounded to dt)."""
    B, R = len(cells), 2
    sol = solver(S, C, K, dt, batch=B)
    Gb, Mb, Cb, g, _ = dev_inputs(sol, cells)
    sol.cross_prepare(Gb, Mb, Cb, g, X.RHO)
    W = sol.read_cross("W").reshape(B, sol.M_size)
    rng = np.random.default_rng(S + K)
    N, n = sol.N, S + C
    vec = rng.standard_normal((B, R, N)).astype(dt)
    gin = sol.to_device(vec.reshape(-1))
    gp = sol.new(B * R * N + 1).fill_(float("nan"))[1:]
    sol.cross_rhs(gin, gp)
    dz = sol.new(B * R * N + 1)[1:]
    dz.copy_(gin)
    sol.cross_finish(dz)
    gp, dz = host(gp).reshape(B, R, N), host(dz).reshape(B, R, N)
    xs = np.array([k * n + i for k in range(K) for i in range(S)])
    us = np.array([k * n + S + j for k in range(K - 1) for j in range(C)], dtype=np.int64)
    for b in range(B):
        Wb = X.unpack_W(W[b], S, C, K)
        for r in range(R):
            assert np.array_equal(gp[b, r][us], vec[b, r][us]) and np.array_equal(dz[b, r][xs], vec[b, r][xs])
            if K == 1:
                assert np.array_equal(gp[b, r], vec[b, r]) and np.array_equal(dz[b, r], vec[b, r])
                continue
            tg, tf = X.transform_g(Wb.astype(LD), vec[b, r], S, C, K), X.finish(Wb.astype(LD), vec[b, r], S, C, K)
            if dt == np.float64:
                assert rel(gp[b, r], tg) < BLOCK_BAR and rel(dz[b, r], tf) < BLOCK_BAR, (rel(gp[b, r], tg), rel(dz[b, r], tf))
            else:
                check_f32("cross rhs %d/%d/%d" % (S, C, K), gp[b, r], X.transform_g(Wb, vec[b, r], S, C, K), tg.astype(np.float64))
                check_f32("cross finish %d/%d/%d" % (S, C, K), dz[b, r], X.finish(Wb, vec[b, r], S, C, K), tf.astype(np.float64))
    sol.close()


def test_second_pass_of_the_knot_stride():
    """2/1/8197: the grid has 8192 workgroups, so knots 8192 .. 8196 (the last one without M) are a workgroup's second knot.
    prepare, rhs and finish there, compared alone."""
    S, C, K = X.STRIDE_CELL
    (blocks, M), = X.batch_cells(S, C, K, 1, seed=7)
    Q, R, A, B, q, r, c = blocks
    sol = solver(S, C, K)
    got, = prepared(sol, [(blocks, M)])
    t = X.transform(Q, R, A, B, q, r, M, X.RHO, LD)
    lo = 8192
    assert blockwise(got["W"][lo:], t["W"][lo:], "W") < BLOCK_BAR and blockwise(got["A2"][lo:], t["A2"][lo:], "A2") < BLOCK_BAR
    assert blockwise(got["Q2"][lo:], t["Q2"][lo:], "Q2") < BLOCK_BAR and blockwise(got["Q2"][:lo], t["Q2"][:lo], "Q2") < BLOCK_BAR
    assert np.array_equal(got["Q2"][K - 1], Q[K - 1]) and np.array_equal(got["R"], R) and np.array_equal(got["B"], B)
    n = S + C
    gw = g_of(t, t["q2"], r.astype(LD), S, C, K)
    assert rel(got["g"][lo * n:], gw[lo * n:]) < BLOCK_BAR and rel(got["g"], gw) < BLOCK_BAR
    vec = np.random.default_rng(1).standard_normal(sol.N)
    gp, dz = sol.cross_rhs(sol.to_device(vec)), sol.cross_finish(sol.to_device(vec))
    tg, tf = X.transform_g(got["W"].astype(LD), vec, S, C, K), X.finish(got["W"].astype(LD), vec, S, C, K)
    gp, dz = host(gp), host(dz)
    assert rel(gp[lo * n:], tg[lo * n:]) < BLOCK_BAR and rel(dz[lo * n:], tf[lo * n:]) < BLOCK_BAR
    assert rel(gp, tg) < BLOCK_BAR and rel(dz, tf) < BLOCK_BAR
    sol.close()


# ---- 2. whole solves ---------------------------------------------------------------------------------------------------------
def cross_solve(sol, inp, kw, lam=None, dz=None):
    lam = sol.new(sol.batch * sol.sizes["sk"]) if lam is None else lam
    dz = sol.new(sol.batch * sol.N) if dz is None else dz
    sol.linsys_blocks_cross(*inp, kw["exit_tol"], kw["max_iters"], X.RHO, lam, dz)
    torch.cuda.synchronize()
    sol.check_status()
    return host(lam).reshape(sol.batch, -1), host(dz).reshape(sol.batch, -1)


SOLVES = [(S, C, K, B) for S, C, K in X.SOLVE_CELLS for B in (1, 3)]


@pytest.mark.parametrize("S,C,K,B", SOLVES, ids=["%d-%d-%d-B%d" % c for c in SOLVES])
def test_whole_solve_fp64_against_the_dense_cross_kkt(S, C, K, B):
    """lambda and dz of every system within 1e-6 of the dense solve with M and M^T in place; a second identical call repeats
    bit for bit; every system of a batch has the bits of its solo run; the caller's arrays are not written."""
    whole_solve_fp64_case(S, C, K, X.batch_cells(S, C, K, B, seed=20 + K), TIGHT)


def whole_solve_fp64_case(S, C, K, cells, pcg):
    """The body of test_whole_solve_fp64_against_the_dense_cross_kkt on the given cells at the PCG settings pcg (exit_tol,
    max_iters) -> the worst error of lambda and dz."""
    B = len(cells)
    sol = solver(S, C, K, batch=B)
    inp = dev_inputs(sol, cells)
    before = [host(t).copy() for t in inp]
    lam, dz = cross_solve(sol, inp, pcg)
    worst = 0.0
    for b, (blocks, M) in enumerate(cells):
        dz_w, lam_w = X.dense_solve(blocks, M)
        e = rel(lam[b], lam_w), rel(dz[b], dz_w)
        print("solve %d/%d/%d B%d sys %d: lam %.3g dz %.3g" % (S, C, K, B, b, *e))
        assert max(e) < SOLVE_BAR, (b, e)
        worst = max(worst, *e)
    lam2, dz2 = cross_solve(sol, inp, pcg)
    assert lam2.tobytes() == lam.tobytes() and dz2.tobytes() == dz.tobytes()
    assert all(np.array_equal(host(t), w) for t, w in zip(inp, before))
    if B > 1:
        for b in range(B):
            one = solver(S, C, K)
            l1, d1 = cross_solve(one, dev_inputs(one, cells[b:b + 1]), pcg)
            assert l1[0].tobytes() == lam[b].tobytes() and d1[0].tobytes() == dz[b].tobytes(), b
            one.close()
    sol.close()
    return worst


@pytest.mark.parametrize("S,C,K,B", SOLVES, ids=["%d-%d-%d-B%d" % c for c in SOLVES])
def test_whole_solve_fp32_beside_the_float32_restatement(S, C, K, B):
    """The device's error against the fp64 dense solve of the float32-rounded inputs is at most 10 x the error of the float32
    restatement (cross_ref.oracle32_solve: transform and finish in float32 around the oracle's float32 solve, same exit_tol
    and max_iters: F32_TIGHT, both run to rounding) - the margin of DESIGN.md section 3.14 for this comparison; it covers the order of the sums.  Both numbers
    go to profiles/cross_accuracy.json."""
    whole_solve_fp32_case(S, C, K, rounded(X.batch_cells(S, C, K, B, seed=20 + K), np.float32), ACCURACY)


def whole_solve_fp32_case(S, C, K, cells, log):
    """The body of test_whole_solve_fp32_beside_the_float32_restatement on the given (float32-rounded) cells; both errors of
    every system are appended to log."""
    B = len(cells)
    sol = solver(S, C, K, np.float32, batch=B)
    lam, dz = cross_solve(sol, dev_inputs(sol, cells), F32_TIGHT)
    rho32 = np.float64(np.float32(X.RHO))
    for b, (blocks, M) in enumerate(cells):
        dz_w, lam_w = X.dense_solve(blocks, M, rho=rho32)
        dz_r, lam_r = X.oracle32_solve(blocks, M, F32_TIGHT["exit_tol"], F32_TIGHT["max_iters"])
        eg, er = max(rel(lam[b], lam_w), rel(dz[b], dz_w)), max(rel(lam_r, lam_w), rel(dz_r, dz_w))
        log.append(dict(S=S, C=C, K=K, B=B, system=b, err_device=float(eg), err_restatement32=float(er)))
        print("fp32 %d/%d/%d B%d sys %d: device %.3g restatement %.3g" % (S, C, K, B, b, eg, er))
        assert eg <= 10.0 * er, (b, eg, er)
    sol.close()


def math_tensors(cells, dt=torch.float64, grad=False):
    """The stacked math-shaped blocks and M of the cells as device tensors (unbatched for one cell)."""
    stack = lambda arrs: np.stack(arrs) if len(arrs) > 1 else arrs[0]
    t = [torch.tensor(stack([blocks[i] for blocks, _ in cells]), dtype=dt, device="cuda:0", requires_grad=grad) for i in range(7)]
    return t, torch.tensor(stack([M for _, M in cells]), dtype=dt, device="cuda:0", requires_grad=grad)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_zero_M_has_the_bits_of_the_solve_without_M(dt):
    """M = 0: W = 0 and the transformed blocks are the caller's, so lambda and dz are those of kkt_solve without M, bit for bit;
    and a nonzero M does change them."""
    kw = dict(rho=X.RHO, **(TIGHT if dt == torch.float64 else F32_KW))
    for S, C, K, B in ((14, 7, 9, 1), (4, 2, 3, 3), (32, 16, 3, 1)):
        t, M = math_tensors(X.batch_cells(S, C, K, B, seed=3), dt)
        lam0, dz0 = ag().kkt_solve(*t, **kw)
        lam1, dz1 = ag().kkt_solve(*t, M=torch.zeros_like(M), **kw)
        assert host(lam1).tobytes() == host(lam0).tobytes() and host(dz1).tobytes() == host(dz0).tobytes(), (S, C, K, B)
        lam2, dz2 = ag().kkt_solve(*t, M=M, **kw)
        assert not torch.equal(dz2, dz0)


# ---- 3. re-solve ----------------------------------------------------------------------------------------------------------------
RESOLVES = [(S, C, K, R) for S, C, K in X.RESOLVE_CELLS for R in (1, 3)]


@pytest.mark.parametrize("S,C,K,R", RESOLVES, ids=["%d-%d-%d-R%d" % c for c in RESOLVES])
def test_solve_rhs_cross_against_the_dense_solve(S, C, K, R):
    """R right-hand sides for each of two systems: every one within 1e-6 of the dense cross solve; dz is the restatement's
    finish of what the plain re-solve (which solves the transformed system) gives for the device's g', lambda its lambda."""
    solve_rhs_cross_case(S, C, K, R, X.batch_cells(S, C, K, 2, seed=30 + K), TIGHT)


def solve_rhs_cross_case(S, C, K, R, cells, pcg):
    """The body of test_solve_rhs_cross_against_the_dense_solve on the given cells at the PCG settings pcg (exit_tol, max_iters)."""
    B = len(cells)
    sol = solver(S, C, K, batch=B)
    inp = dev_inputs(sol, cells)
    cross_solve(sol, inp, pcg)
    gen = sol.get_option("assembly_gen")
    rng = np.random.default_rng(R)
    g, c = rng.standard_normal((B, R, sol.N)), rng.standard_normal((B, R, S * K))
    gd, cd = sol.to_device(g.reshape(-1)), sol.to_device(c.reshape(-1))
    sol.reserve_rhs(R)
    lam, dz, its = sol.solve_rhs_cross(gd, cd, pcg["exit_tol"], pcg["max_iters"])
    sol.check_status()
    assert sol.get_option("assembly_gen") == gen
    lam_p, dz_p, _ = sol.solve_rhs(sol.cross_rhs(gd), cd, pcg["exit_tol"], pcg["max_iters"])
    W = sol.read_cross("W").reshape(B, sol.M_size)
    lam, dz, lam_p, dz_p = (host(t).reshape(B, R, -1) for t in (lam, dz, lam_p, dz_p))
    assert (host(its) > 0).all()
    for b, (blocks, M) in enumerate(cells):
        dz_w, lam_w = X.dense_solve(blocks, M, g=g[b], c=c[b])
        Wb = X.unpack_W(W[b], S, C, K).astype(LD)
        for r in range(R):
            e = rel(lam[b, r], lam_w[r]), rel(dz[b, r], dz_w[r])
            assert max(e) < SOLVE_BAR, (b, r, e)
            assert lam[b, r].tobytes() == lam_p[b, r].tobytes()
            assert rel(dz[b, r], X.finish(Wb, dz_p[b, r], S, C, K)) < BLOCK_BAR
    sol.close()


def test_solve_rhs_cross_needs_its_own_assembly():
    """After a plain linsys_blocks (or a cross_prepare alone, or nothing at all) the assembly is not a cross one: EINVAL with a
    reason; a cross solve makes it one again."""
    S, C, K = 4, 2, 3
    cells = X.batch_cells(S, C, K, 1, seed=2)
    sol = solver(S, C, K)
    Gb, Mb, Cb, g, c = inp = dev_inputs(sol, cells)
    lam, dz = sol.new(S * K), sol.new(sol.N)

    def refused():
        with pytest.raises(_lib.GatoError, match="not that of a cross solve") as e:
            sol.solve_rhs_cross(g, c, 1e-10, 100)
        assert e.value.code == -1

    refused()
    cross_solve(sol, inp, TIGHT)
    sol.solve_rhs_cross(g, c, 1e-10, 100)
    sol.linsys_blocks(Gb, Cb, g, c, 1e-10, 100, X.RHO, lam, dz)
    refused()
    cross_solve(sol, inp, TIGHT)
    sol.cross_prepare(Gb, Mb, Cb, g, X.RHO)
    refused()
    with pytest.raises(_lib.GatoError):                                      # and the plain re-solve has lost its C blocks too
        sol.solve_rhs(g, c, 1e-10, 100)
    sol.close()


def test_c_abi_refusals():
    S, C, K = 4, 2, 3
    sol = solver(S, C, K)
    Gb, Mb, Cb, g, c = dev_inputs(sol, X.batch_cells(S, C, K, 1))
    L, p = _lib.lib(), lambda t: ct.c_void_p(t.data_ptr()) if t is not None else None
    lam, dz = sol.new(S * K), sol.new(sol.N)
    for i in range(5):
        a = [None if j == i else t for j, t in enumerate((Gb, Mb, Cb, g, c))]
        assert L.gato_linsys_device_blocks_cross(sol._h, *map(p, a), 1e-10, 100, X.RHO, p(lam), p(dz), sol._stream()) == -1
        assert b"required" in L.gato_last_error()
    assert L.gato_cross_rhs(sol._h, 1, p(g), p(dz), sol._stream()) == -1 and b"no W yet" in L.gato_last_error()
    assert L.gato_linsys_device_blocks_cross(None, p(Gb), p(Mb), p(Cb), p(g), p(c), 1e-10, 100, X.RHO, p(lam), p(dz), None) == -1
    cross_solve(sol, (Gb, Mb, Cb, g, c), TIGHT)
    for R in (0, -1, 65536):
        assert L.gato_solve_rhs_cross(sol._h, R, p(g), p(c), 1e-10, 100, p(lam), p(dz), None, sol._stream()) == -1
        assert L.gato_cross_finish(sol._h, R, p(dz), sol._stream()) == -1
    assert L.gato_solve_rhs_cross(sol._h, 1, p(g), p(c), 1e-10, 100, None, p(dz), None, sol._stream()) == -1
    assert L.gato_kkt_grad_cross(sol._h, p(dz), None, p(Mb), sol._stream()) == -1
    with pytest.raises(ValueError, match="M_blocks"):
        sol.linsys_blocks_cross(Gb, Mb[:-1], Cb, g, c, 1e-10, 100, X.RHO)
    with pytest.raises(ValueError, match="Mbar"):
        sol.kkt_grad_cross(dz, dz, Mb.float())
    sol.close()


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------
NAMES = ("Q", "R", "A", "B", "q", "r", "c")


@pytest.mark.parametrize("S,C,K", X.GRADCHECK_CELLS, ids=["%d-%d-%d" % c for c in X.GRADCHECK_CELLS])
def test_gradcheck(S, C, K):
    """torch.autograd.gradcheck over (Q, R, A, B, M, q, r, c), the settings of tests/test_gpu_kkt_grad.py; Q and R enter
    symmetrised (their gradients are those of symmetric perturbations)."""
    (blocks, M), = X.batch_cells(S, C, K, 1, seed=30 + K)
    t, Mt = math_tensors([(blocks, M)], grad=True)
    kw = dict(rho=X.RHO, **TIGHT)

    def f(Q, R, A, B, M, q, r, c):
        return ag().kkt_solve(0.5 * (Q + Q.transpose(-1, -2)), 0.5 * (R + R.transpose(-1, -2)), A, B, q, r, c, M=M, **kw)

    assert torch.autograd.gradcheck(f, (t[0], t[1], t[2], t[3], Mt, t[4], t[5], t[6]), eps=1e-6, atol=1e-5, rtol=1e-4)


GRADS = [(S, C, K) for S, C in X.SHAPES for K in X.GRAD_K]


@pytest.mark.parametrize("S,C,K", GRADS, ids=["%d-%d-%d" % c for c in GRADS])
def test_grad_cross_kernel_against_the_outer_products(S, C, K):
    """M_bar of three systems from random (dz, a), into an output one element off the 16-byte grid: 1e-14 of the numpy outer
    products in fp64 (one rounding of two rounded products), 1e-6 in fp32."""
    B = 3
    for dt, bar in ((np.float64, GRAD_BAR), (np.float32, 1e-6)):
        sol = solver(S, C, K, dt, batch=B)
        rng = np.random.default_rng(K)
        dz, a = rng.standard_normal((B, sol.N)).astype(dt), rng.standard_normal((B, sol.N)).astype(dt)
        buf = sol.new(B * sol.M_size + 2).fill_(float("nan"))
        sol.kkt_grad_cross(sol.to_device(dz.reshape(-1)), sol.to_device(a.reshape(-1)), buf[1:-1])
        got = host(buf)
        assert np.isnan(got[0]) and np.isnan(got[-1])
        for b in range(B):
            want = X.pack_M(X.grad_M(dz[b], a[b], S, C, K))
            assert rel(got[1 + b * sol.M_size:1 + (b + 1) * sol.M_size], want) < bar, (dt, b)
        sol.close()


def loss_grads(cells, w1, w2, only=None, M_zero=False, **pcg):
    """kkt_solve(M=...) forward and the backward of L = w1 . dz + w2 . lam -> (tensors, M tensor); only: the one name that
    requires a gradient."""
    t, Mt = math_tensors(cells, grad=only is None)
    if only == "M":
        Mt.requires_grad_(True)
    lam, dz = ag().kkt_solve(*t, M=Mt, rho=X.RHO, **(pcg or TIGHT))
    dv = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    ((dz * dv(w1)).sum() + (lam * dv(w2)).sum()).backward()
    return t, Mt


@pytest.mark.parametrize("S,C,K", [(14, 7, 9), (32, 16, 3)], ids=["14-7-9", "32-16-3"])
def test_gradients_of_a_batch_against_the_dense_reference(S, C, K):
    """Every gradient of three systems within 1e-6 of the formulas on the dense forward and adjoint solves; the third system's
    upstream gradient is all zero: its gradients are exactly zero (no 0 / 0 of a PCG leaks out)."""
    gradients_of_a_batch_case(S, C, K, X.batch_cells(S, C, K, 3, seed=20 + K))


def gradients_of_a_batch_case(S, C, K, cells, **pcg):
    """The body of test_gradients_of_a_batch_against_the_dense_reference on three given cells (pcg: other PCG settings than
    TIGHT)."""
    B = 3
    rng = np.random.default_rng(5)
    N = (S + C) * K - C
    w1, w2 = rng.standard_normal((B, N)), rng.standard_normal((B, S * K))
    w1[2] = 0
    w2[2] = 0
    t, Mt = loss_grads(cells, w1, w2, **pcg)
    for b in range(2):
        want = X.dense_reference(*cells[b], w1[b], w2[b])
        for n, x in zip(NAMES + ("M",), t + [Mt]):
            assert rel(host(x.grad[b]), want[n]) < SOLVE_BAR, (b, n, rel(host(x.grad[b]), want[n]))
    for n, x in zip(NAMES + ("M",), t + [Mt]):
        assert bool((x.grad[2] == 0).all()), n


def test_stale_assembly_gives_the_same_gradients():
    """Another forward of the same shape between forward and backward: the backward rebuilds its assembly (one more assembly
    than the two forwards) and returns the bits of the undisturbed run."""
    S, C, K = 14, 7, 9
    c1, c2 = X.batch_cells(S, C, K, 1, seed=1), X.batch_cells(S, C, K, 1, seed=2)
    rng = np.random.default_rng(8)
    w1, w2 = rng.standard_normal((S + C) * K - C), rng.standard_normal(S * K)
    t0, M0 = loss_grads(c1, w1, w2)
    t, Mt = math_tensors(c1, grad=True)
    kw = dict(rho=X.RHO, **TIGHT)
    lam, dz = ag().kkt_solve(*t, M=Mt, **kw)
    sol = ag()._SOLVERS[(S, C, K, 1, torch.float64, 0)]
    gen = sol.get_option("assembly_gen")
    with torch.no_grad():
        t2, M2 = math_tensors(c2)
        ag().kkt_solve(*t2, M=M2, **kw)
        ag().kkt_solve(*t2, **kw)                                           # and a plain one: the assembly is not even a cross one
    assert sol.get_option("assembly_gen") == gen + 2
    dv = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    ((dz * dv(w1)).sum() + (lam * dv(w2)).sum()).backward()
    assert sol.get_option("assembly_gen") == gen + 3
    for n, x, y in zip(NAMES + ("M",), t + [Mt], t0 + [M0]):
        assert torch.equal(x.grad, y.grad), n


def test_only_M_requires_grad():
    S, C, K = 6, 3, 5
    cells = X.batch_cells(S, C, K, 1, seed=4)
    rng = np.random.default_rng(9)
    w1, w2 = rng.standard_normal((S + C) * K - C), rng.standard_normal(S * K)
    t, Mt = loss_grads(cells, w1, w2, only="M")
    assert all(x.grad is None for x in t)
    assert rel(host(Mt.grad), X.dense_reference(*cells[0], w1, w2)["M"]) < SOLVE_BAR
    t, Mt = math_tensors(cells)
    lam, dz = ag().kkt_solve(*t, M=Mt, rho=X.RHO, **TIGHT)
    assert not lam.requires_grad and lam.grad_fn is None


def test_forward_mode_with_M_is_not_built():
    import torch.autograd.forward_ad as fwad
    cells = X.batch_cells(4, 2, 3, 1)
    t, Mt = math_tensors(cells)
    kw = dict(rho=X.RHO, **TIGHT)
    with fwad.dual_level():
        q = fwad.make_dual(t[4], torch.ones_like(t[4]))
        with pytest.raises(NotImplementedError, match="forward mode with a cross term"):
            ag().kkt_solve(*t[:4], q, *t[5:], M=Mt, **kw)
        lam, _ = ag().kkt_solve(*t[:4], q, *t[5:], **kw)                    # without M forward mode is what it was
        assert fwad.unpack_dual(lam).tangent is not None


# ---- 5. K = 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", X.SHAPES, ids=["%d-%d" % s for s in X.SHAPES])
def test_one_knot_is_the_plain_solve(S, C):
    """K = 1 has no M: an empty M (kkt_solve) or a NULL one (the C entry) gives the plain solve bit for bit, the re-solve too."""
    cells = X.batch_cells(S, C, 1, 1, seed=6)
    t, Mt = math_tensors(cells)
    assert Mt.shape == (0, S, C)
    kw = dict(rho=X.RHO, **TIGHT)
    lam0, dz0 = ag().kkt_solve(*t, **kw)
    lam1, dz1 = ag().kkt_solve(*t, M=Mt, **kw)
    assert host(lam1).tobytes() == host(lam0).tobytes() and host(dz1).tobytes() == host(dz0).tobytes()
    sol = solver(S, C, 1)
    Gb, Mb, Cb, g, c = dev_inputs(sol, cells)
    lam, dz = cross_solve(sol, (Gb, None, None, g, c), TIGHT)
    assert lam[0].tobytes() == host(lam0).tobytes() and dz[0].tobytes() == host(dz0).tobytes()
    l2, d2, _ = sol.solve_rhs_cross(g, c, TIGHT["exit_tol"], TIGHT["max_iters"])
    l3, d3, _ = sol.solve_rhs(g, c, TIGHT["exit_tol"], TIGHT["max_iters"])
    assert host(l2).tobytes() == host(l3).tobytes() and host(d2).tobytes() == host(d3).tobytes()
    sol.close()
