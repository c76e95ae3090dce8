"""GPU suite of the CSR entry to the cross solve: cross_prepare_csr_kernel alone, whole solves through
Solver.linsys_cross, and the gradients through kkt_grad_csr_cross and kkt_solve_csr(cross=True).

The reference of the scatter is tests/cross_csr_ref.py (a loop over the entries in storage order).  The central comparison has no
tolerance: the work area after the fused launch equals, bit for bit, what cross_prepare leaves from the scattered blocks, and a
whole solve equals linsys_blocks_cross on them.  Solutions are also held to the dense solve of the CSR itself (synth.dense_kkt,
which knows nothing of the scatter) at the project's 1e-6; fp32 is measured beside the float32 restatement at section 3.15's
margin of 10."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cross_csr_ref as R                           # noqa: E402
import cross_hard_cells as H                        # noqa: E402
import cross_ref as X                               # noqa: E402
from f32_parity import rel                          # noqa: E402
from gato_python_amd import _lib, synth             # noqa: E402

TIGHT = dict(exit_tol=1e-20, max_iters=1000)        # tests/test_gpu_cross.py: the PCG runs to rounding
F32_KW = dict(exit_tol=1e-5, max_iters=100)
F32_TIGHT = dict(exit_tol=1e-12, max_iters=300)
SOLVE_BAR = 1e-6
PATTERN_K = 5
DTS = [np.float64, np.float32]
DT_IDS = ["f64", "f32"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def ag():
    from gato_python_amd import autograd
    return autograd


def solver(S, C, K, dt=np.float64, batch=1):
    from gato_python_amd.solver import Solver
    return Solver(S, C, K, dt, batch=batch)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def rounded(cells, dt):
    r = lambda a: np.asarray(a).astype(dt).astype(np.float64)
    return [(tuple(r(b) for b in blocks), r(M)) for blocks, M in cells]


def dev_csr(sol, systems, shift=0):
    """(G_row, G_col, G_val, C_row, C_col, C_val, g, c) of the systems of one pattern on the device, values in the solver's
    dtype [B nnz] flat.  shift = 1: every value array is a view one element into its allocation, off the 16-byte grid."""
    idx, vals = R.stacked(systems, sol.np_dtype)
    ti = [torch.from_numpy(a.copy()).to("cuda:%d" % sol.device) for a in idx]
    tv = []
    for v in vals:
        buf = sol.new(v.size + shift)
        buf[shift:].copy_(torch.from_numpy(v.reshape(-1)))
        tv.append(buf[shift:])
    return ti[0], ti[1], tv[0], ti[2], ti[3], tv[1], tv[2], tv[3]


def poison(sol):
    """Every byte of the cross work area to 0xFF (NaN in both dtypes): an entry no kernel writes shows."""
    torch.cuda.synchronize()
    hip = ct.CDLL("libamdhip64.so")
    for name, per in dict(G=sol.sizes["G_dense"], C=sol.sizes["C_dense"], W=sol.M_size, g=sol.N).items():
        if per:
            assert hip.hipMemset(ct.c_void_p(sol.cross_buffer_ptr(name)), 0xFF, ct.c_size_t(per * sol.batch * sol.np_dtype.itemsize)) == 0
    assert hip.hipDeviceSynchronize() == 0


def work_area(sol):
    return {k: sol.read_cross(k).copy() for k in "GCWg"}


def nan_outs(sol):
    B = sol.batch
    mk = lambda n: torch.full((B * n,), float("nan"), dtype=sol.dtype, device="cuda:%d" % sol.device)
    return mk(sol.sizes["G_dense"]), mk(sol.M_size), mk(sol.sizes["C_dense"])


def stage_case(S, C, K, systems, dt, knots_from=0):
    """The fused launch on the systems of one pattern, from value arrays off the 16-byte grid into a poisoned work area:
    the optional outputs are the reference scatter, exactly; the work area is, bit for bit, cross_prepare on those blocks; the
    caller's arrays are not written.  knots_from: also compare the knots from that one on alone."""
    B = len(systems)
    sol = solver(S, C, K, dt, batch=B)
    a = dev_csr(sol, systems, shift=1)
    before = [host(t).copy() for t in a]
    Go, Mo, Co = nan_outs(sol)
    sol.cross_prepare_csr(*a[:7], X.RHO, Go, Mo, Co)                       # the first call allocates the area
    poison(sol)
    Go, Mo, Co = nan_outs(sol)
    sol.cross_prepare_csr(*a[:7], X.RHO, Go, Mo, Co)
    got = work_area(sol)
    assert all(np.isfinite(v).all() for v in got.values())
    want = [R.scatter(s.astype(dt)) for s in systems]
    for name, t in (("G", Go), ("M", Mo), ("C", Co)):
        assert same(host(t), np.concatenate([w[name] for w in want])), name
    assert all(same(host(t), w) for t, w in zip(a, before))
    poison(sol)
    sol.cross_prepare(Go, Mo if K > 1 else None, Co if K > 1 else None, a[6], X.RHO)
    ref = work_area(sol)
    n, SS, CC, SC = S + C, S * S, C * C, S * C
    for k in "GCWg":
        assert same(got[k], ref[k]), k
        if knots_from:
            per = dict(G=SS + CC, C=SS + SC, W=SC, g=n)[k]
            assert same(got[k][knots_from * per:], ref[k][knots_from * per:]) and got[k][knots_from * per:].size > 0
    sol.close()
    return got


# ---- 1. the stage alone ------------------------------------------------------------------------------------------------------------
STAGE_CELLS = [(S, C, K) for S, C in X.SHAPES for K in X.KERNEL_K]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("S,C,K", STAGE_CELLS, ids=["%d-%d-%d" % c for c in STAGE_CELLS])
def test_stage_is_the_scatter_then_cross_prepare(S, C, K, dt):
    """Three different systems on one both-triangle pattern, K = 1 (no M at all) included."""
    stage_case(S, C, K, [R.csr_full(c) for c in rounded(X.batch_cells(S, C, K, 3, seed=K), dt)], dt)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(R.BUILDERS))
@pytest.mark.parametrize("S,C", X.SHAPES, ids=["%d-%d" % c for c in X.SHAPES])
def test_stage_on_every_pattern(S, C, name, dt):
    """Upper-only storage, shuffled rows with explicit zeros, duplicates (the last entry wins, M slots included), emptied rows,
    all three, a cross entry in the last knot (dropped) and one whose column lies in another knot (folded, wins its slot)."""
    stage_case(S, C, PATTERN_K, [R.BUILDERS[name](c) for c in rounded(X.batch_cells(S, C, PATTERN_K, 3, seed=PATTERN_K), dt)], dt)


def test_stage_on_the_hard_cells():
    """Dense R_k, graded blocks, A_k far from the identity (tests/cross_hard_cells.py): the Gauss-Jordan has real work."""
    for S, C, K in ((6, 3, 3), (14, 7, 2), (32, 16, 2)):
        stage_case(S, C, K, [R.csr_full(c) for c in H.hard_batch(S, C, K, 3, H.grade_of(np.float64))], np.float64)


@pytest.mark.parametrize("threads", [64, 256])
def test_the_bits_do_not_depend_on_the_workgroup_size(threads):
    S, C, K = 14, 7, 5
    systems = [R.csr_pattern(c, "combined") for c in X.batch_cells(S, C, K, 3, seed=1)]
    sol = solver(S, C, K, batch=3)
    a = dev_csr(sol, systems)
    sol.cross_prepare_csr(*a[:7], X.RHO)
    base = work_area(sol)
    sol.set_option("cross_csr_threads", threads)
    poison(sol)
    sol.cross_prepare_csr(*a[:7], X.RHO)
    got = work_area(sol)
    assert all(same(got[k], base[k]) for k in "GCWg")
    sol.close()


@pytest.mark.parametrize("skip", ["G_out", "M_out", "C_out"])
def test_each_optional_output_may_be_null(skip):
    S, C, K = 4, 2, 3
    systems = [R.csr_full(c) for c in X.batch_cells(S, C, K, 3, seed=2)]
    sol = solver(S, C, K, batch=3)
    a = dev_csr(sol, systems)
    outs = dict(zip(("G_out", "M_out", "C_out"), nan_outs(sol)))
    sol.cross_prepare_csr(*a[:7], X.RHO, **outs)
    full = work_area(sol)
    want = {k: host(t).copy() for k, t in outs.items()}
    outs = dict(zip(("G_out", "M_out", "C_out"), nan_outs(sol)))
    untouched = outs.pop(skip)
    poison(sol)
    sol.cross_prepare_csr(*a[:7], X.RHO, **outs)
    got = work_area(sol)
    assert all(same(got[k], full[k]) for k in "GCWg")
    assert all(same(host(t), want[k]) for k, t in outs.items()) and np.isnan(host(untouched)).all()
    sol.close()


def test_second_pass_of_the_knot_stride():
    """2/1/8197: the grid has 8192 workgroups, so knots 8192 .. 8196 (the last one without M) are a workgroup's second knot."""
    S, C, K = X.STRIDE_CELL
    stage_case(S, C, K, [R.csr_full(X.batch_cells(S, C, K, 1, seed=7)[0])], np.float64, knots_from=8192)


# ---- 2. whole solves -------------------------------------------------------------------------------------------------------------
def csr_solve(sol, a, kw):
    lam, dz = sol.new(sol.batch * sol.sizes["sk"]), sol.new(sol.batch * sol.N)
    sol.linsys_cross(*a, kw["exit_tol"], kw["max_iters"], X.RHO, lam, dz)
    torch.cuda.synchronize()
    sol.check_status()
    return host(lam).reshape(sol.batch, -1), host(dz).reshape(sol.batch, -1)


def blocks_solve(sol, systems, c, kw):
    """linsys_blocks_cross on the reference scatter's blocks of the systems."""
    sc = [R.scatter(s.astype(sol.np_dtype)) for s in systems]
    dev = lambda k: sol.to_device(np.concatenate([x[k] for x in sc]))
    g = sol.to_device(np.concatenate([s.g for s in systems]))
    lam, dz = sol.new(sol.batch * sol.sizes["sk"]), sol.new(sol.batch * sol.N)
    sol.linsys_blocks_cross(dev("G"), dev("M"), dev("C"), g, c, kw["exit_tol"], kw["max_iters"], X.RHO, lam, dz)
    torch.cuda.synchronize()
    sol.check_status()
    return host(lam).reshape(sol.batch, -1), host(dz).reshape(sol.batch, -1)


SOLVES = [(S, C, K, B) for S, C, K in X.SOLVE_CELLS for B in (1, 3)]


@pytest.mark.parametrize("S,C,K,B", SOLVES, ids=["%d-%d-%d-B%d" % c for c in SOLVES])
def test_whole_solve_fp64(S, C, K, B):
    """linsys_cross has the bits of linsys_blocks_cross on the scattered blocks; lambda and dz are within 1e-6 of the dense
    solve of synth.dense_kkt of the CSR; a second call repeats bit for bit; every system of a batch has the bits of its solo
    run; the caller's arrays are not written."""
    cells = X.batch_cells(S, C, K, B, seed=20 + K)
    systems = [R.csr_full(c) for c in cells]
    sol = solver(S, C, K, batch=B)
    a = dev_csr(sol, systems)
    before = [host(t).copy() for t in a]
    lam, dz = csr_solve(sol, a, TIGHT)
    for b, s in enumerate(systems):
        x = X.solve_refined(*synth.dense_kkt(s))
        e = rel(lam[b], x[s.N:]), rel(dz[b], x[:s.N])
        print("csr solve %d/%d/%d B%d sys %d: lam %.3g dz %.3g" % (S, C, K, B, b, *e))
        assert max(e) < SOLVE_BAR, (b, e)
    lam2, dz2 = csr_solve(sol, a, TIGHT)
    assert same(lam2, lam) and same(dz2, dz)
    assert all(same(host(t), w) for t, w in zip(a, before))
    lam_b, dz_b = blocks_solve(sol, systems, a[7], TIGHT)
    assert same(lam_b, lam) and same(dz_b, dz)
    if B > 1:
        for b in range(B):
            one = solver(S, C, K)
            l1, d1 = csr_solve(one, dev_csr(one, systems[b:b + 1]), TIGHT)
            assert same(l1[0], lam[b]) and same(d1[0], dz[b]), b
            one.close()
    sol.close()


@pytest.mark.parametrize("S,C,K,B", SOLVES, ids=["%d-%d-%d-B%d" % c for c in SOLVES])
def test_whole_solve_fp32(S, C, K, B):
    """The bits of linsys_blocks_cross on the scattered blocks, and the device's error against the fp64 dense solve of the
    float32-rounded inputs is at most 10 x the float32 restatement's (cross_ref.oracle32_solve; section 3.15's bar)."""
    cells = rounded(X.batch_cells(S, C, K, B, seed=20 + K), np.float32)
    systems = [R.csr_full(c) for c in cells]
    sol = solver(S, C, K, np.float32, batch=B)
    a = dev_csr(sol, systems)
    lam, dz = csr_solve(sol, a, F32_TIGHT)
    lam_b, dz_b = blocks_solve(sol, systems, a[7], F32_TIGHT)
    assert same(lam_b, lam) and same(dz_b, dz)
    rho32 = np.float64(np.float32(X.RHO))
    for b, (blocks, M) in enumerate(cells):
        dz_w, lam_w = X.dense_solve(blocks, M, rho=rho32)
        dz_r, lam_r = X.oracle32_solve(blocks, M, F32_TIGHT["exit_tol"], F32_TIGHT["max_iters"])
        eg, er = max(rel(lam[b], lam_w), rel(dz[b], dz_w)), max(rel(lam_r, lam_w), rel(dz_r, dz_w))
        print("csr fp32 %d/%d/%d B%d sys %d: device %.3g restatement %.3g" % (S, C, K, B, b, eg, er))
        assert eg <= 10.0 * er, (b, eg, er)
    sol.close()


@pytest.mark.parametrize("name", ["upper", "combined", "folded", "last_knot"])
def test_whole_solve_on_patterns(name):
    """A pattern's solve is linsys_blocks_cross on what the rule makes of it, and within 1e-6 of the dense solve of those blocks."""
    S, C, K, B = 6, 3, 5, 3
    systems = [R.BUILDERS[name](c) for c in X.batch_cells(S, C, K, B, seed=4)]
    sol = solver(S, C, K, batch=B)
    a = dev_csr(sol, systems)
    lam, dz = csr_solve(sol, a, TIGHT)
    lam_b, dz_b = blocks_solve(sol, systems, a[7], TIGHT)
    assert same(lam_b, lam) and same(dz_b, dz)
    if name in ("upper", "folded", "last_knot"):                            # the transformations that keep every G_k definite
        for b, s in enumerate(systems):
            dz_w, lam_w = X.dense_solve(*R.cell_of(R.scatter(s), s))
            assert max(rel(lam[b], lam_w), rel(dz[b], dz_w)) < SOLVE_BAR
    sol.close()


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_without_cross_entries_and_at_one_knot_it_is_the_plain_solve(dt):
    """A CSR that stores every diagonal entry and holds no cross entry, and any CSR at K = 1: the bits of Solver.linsys /
    linsys_batched (the rho rule coincides when every diagonal entry is stored)."""
    kw = TIGHT if dt == np.float64 else F32_KW
    for S, C, K, B in ((14, 7, 9, 1), (4, 2, 3, 3), (6, 3, 1, 1), (2, 1, 1, 3)):
        cells = rounded(X.batch_cells(S, C, K, B, seed=3), dt)
        systems = [R.csr_full((blocks, np.zeros_like(M))) for blocks, M in cells]
        if K > 1:                                                           # no cross entry at all, not explicit zeros
            n = S + C
            systems = [R._with_G(s, R.P.thin_rows(s.G_row, s.G_col, s.G_val, lambda r, c: (r % n < S) == (c % n < S))) for s in systems]
        sol = solver(S, C, K, dt, batch=B)
        a = dev_csr(sol, systems)
        lam, dz = csr_solve(sol, a, kw)
        assert sol.get_option("assembly_valid") == 1
        l0, d0 = sol.new(B * S * K), sol.new(B * sol.N)
        (sol.linsys if B == 1 else sol.linsys_batched)(*a, kw["exit_tol"], kw["max_iters"], X.RHO, l0, d0)
        assert same(host(l0).reshape(B, -1), lam) and same(host(d0).reshape(B, -1), dz), (S, C, K, B)
        sol.close()


def test_cross_false_solves_a_different_problem():
    """The silent drop the feature removes: the plain CSR path on the same arrays is off by more than 1e-3."""
    S, C, K = 14, 7, 9
    cell, = X.batch_cells(S, C, K, 1, seed=5)
    s = R.csr_both(cell)
    dev = lambda arr, dt: torch.tensor(arr, dtype=dt, device="cuda:0")
    args = (dev(s.G_row, torch.int32), dev(s.G_col, torch.int32), dev(s.G_val, torch.float64), dev(s.C_row, torch.int32),
            dev(s.C_col, torch.int32), dev(s.C_val, torch.float64), dev(s.g, torch.float64), dev(s.c, torch.float64))
    lam1, dz1 = ag().kkt_solve_csr(*args, cross=True, rho=X.RHO, **TIGHT)
    lam0, dz0 = ag().kkt_solve_csr(*args, rho=X.RHO, **TIGHT)
    dz_w, lam_w = X.dense_solve(*cell)
    assert rel(host(dz1), dz_w) < SOLVE_BAR and rel(host(lam1), lam_w) < SOLVE_BAR
    assert rel(host(dz0), dz_w) > 1e-3
    dz_n, lam_n = X.dense_solve(cell[0], None)
    assert rel(host(dz0), dz_n) < SOLVE_BAR


def test_the_cross_entries_that_follow_a_cross_solve():
    """solve_rhs_cross and tangents_cross work after linsys_cross as after linsys_blocks_cross (same bits), and refuse after a
    plain linsys."""
    S, C, K, B = 4, 2, 3, 2
    systems = [R.csr_full(c) for c in X.batch_cells(S, C, K, B, seed=6)]
    sol = solver(S, C, K, batch=B)
    a = dev_csr(sol, systems)
    rng = np.random.default_rng(0)
    g2, c2 = sol.to_device(rng.standard_normal(B * sol.N)), sol.to_device(rng.standard_normal(B * S * K))
    Mdot = sol.to_device(rng.standard_normal(B * sol.M_size))
    lam, dz = csr_solve(sol, a, TIGHT)
    x, l = sol.to_device(dz.reshape(-1)), sol.to_device(lam.reshape(-1))
    sol.reserve_rhs(1)
    r1 = [host(t).copy() for t in sol.solve_rhs_cross(g2, c2, 1e-20, 1000)[:2]]
    t1 = [host(t).copy() for t in sol.tangents_cross(1, x, l, 1e-20, 1000, M_dot=Mdot, g_dot=g2)]
    blocks_solve(sol, systems, a[7], TIGHT)
    r2 = [host(t).copy() for t in sol.solve_rhs_cross(g2, c2, 1e-20, 1000)[:2]]
    t2 = [host(t).copy() for t in sol.tangents_cross(1, x, l, 1e-20, 1000, M_dot=Mdot, g_dot=g2)]
    assert all(same(p, q) for p, q in zip(r1 + t1, r2 + t2))
    l0, d0 = sol.new(B * S * K), sol.new(B * sol.N)
    sol.linsys_batched(*a, 1e-20, 1000, X.RHO, l0, d0)
    with pytest.raises(_lib.GatoError, match="not that of a cross solve"):
        sol.solve_rhs_cross(g2, c2, 1e-20, 1000)
    with pytest.raises(_lib.GatoError, match="not that of a cross solve"):
        sol.tangents_cross(1, x, l, 1e-20, 1000, M_dot=Mdot)
    sol.close()


def test_c_abi_refusals():
    S, C, K = 4, 2, 3
    sol = solver(S, C, K)
    a = dev_csr(sol, [R.csr_full(X.batch_cells(S, C, K, 1)[0])])
    L, p = _lib.lib(), lambda t: ct.c_void_p(t.data_ptr()) if t is not None else None
    lam, dz = sol.new(S * K), sol.new(sol.N)
    nG, nC = a[1].numel(), a[4].numel()

    def call(v, nnzG=nG, nnzC=nC, h=sol._h):
        return L.gato_linsys_device_cross(h, p(v[0]), p(v[1]), p(v[2]), nnzG, p(v[3]), p(v[4]), p(v[5]), nnzC, p(v[6]), p(v[7]),
                                          1e-10, 100, X.RHO, p(lam), p(dz), sol._stream())
    for i in range(8):
        assert call([None if j == i else t for j, t in enumerate(a)]) == -1 and b"required" in L.gato_last_error()
    assert call(a, nnzG=0) == -1 and call(a, nnzC=-1) == -1 and b"positive" in L.gato_last_error()
    assert call(a, h=None) == -1
    assert L.gato_cross_prepare_csr(sol._h, p(a[0]), p(a[1]), None, nG, p(a[3]), p(a[4]), p(a[5]), nC, p(a[6]), X.RHO, None, None, None,
                                    sol._stream()) == -1
    assert L.gato_kkt_grad_csr_cross(sol._h, p(a[0]), p(a[1]), nG, p(a[3]), p(a[4]), nC, p(dz), p(lam), p(dz), p(lam), None, None,
                                     sol._stream()) == -1 and b"both outputs" in L.gato_last_error()
    assert L.gato_kkt_grad_csr_cross(sol._h, None, p(a[1]), nG, p(a[3]), p(a[4]), nC, p(dz), p(lam), p(dz), p(lam), p(a[2]), None,
                                     sol._stream()) == -1
    assert sol.get_option("assembly_valid") == 0                            # nothing ran
    with pytest.raises(ValueError, match="G_val"):
        sol.linsys_cross(a[0], a[1], a[2][:-1], *a[3:], 1e-10, 100, X.RHO)
    with pytest.raises(ValueError, match="G_row"):
        sol.linsys_cross(a[0].long(), *a[1:], 1e-10, 100, X.RHO)
    assert call(a) == 0
    torch.cuda.synchronize()
    sol.close()


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------
GRAD_CELLS = [(S, C, PATTERN_K) for S, C in X.SHAPES]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(R.BUILDERS))
@pytest.mark.parametrize("S,C,K", GRAD_CELLS, ids=["%d-%d-%d" % c for c in GRAD_CELLS])
def test_csr_gradient_is_the_block_gradient_of_its_slot(S, C, K, name, dt):
    """kkt_grad_csr_cross per entry: bit for bit kkt_grad_blocks / kkt_grad_cross at the slot of the reference's map, exactly 0
    where the map has none (a mirror entry, a cross entry of the last knot, an overwritten entry); on four vectors of 11
    systems (two groups of the kernel's eight), outputs one element off the 16-byte grid; and each output alone."""
    B = 11
    cell = X.batch_cells(S, C, K, 1, seed=K)[0]
    s = R.BUILDERS[name](cell)
    sc = R.scatter(s)
    sol = solver(S, C, K, dt, batch=B)
    rng = np.random.default_rng(S * 100 + K)
    dz, a_ = (sol.to_device(rng.standard_normal(B * sol.N)) for _ in range(2))
    lam, beta = (sol.to_device(rng.standard_normal(B * S * K)) for _ in range(2))
    idx = [torch.from_numpy(np.asarray(x, np.int32)).cuda() for x in (s.G_row, s.G_col, s.C_row, s.C_col)]
    nG, nC = len(s.G_col), len(s.C_col)
    Gbar, Cbar = sol.new(B * nG + 1)[1:].fill_(float("nan")), sol.new(B * nC + 1)[1:].fill_(float("nan"))
    sol.kkt_grad_csr_cross(*idx, dz, lam, a_, beta, Gbar, Cbar)
    Gb, Cb = sol.kkt_grad_blocks(dz, lam, a_, beta, sol.new(B * sol.sizes["G_dense"]), sol.new(B * sol.sizes["C_dense"]))
    Mb = sol.kkt_grad_cross(dz, a_)
    Gbar, Cbar, Gb, Cb, Mb = (host(t).reshape(B, -1) for t in (Gbar, Cbar, Gb, Cb, Mb))
    wantG, wantC = np.zeros_like(Gbar), np.zeros_like(Cbar)
    inG, inM, inC = sc["slotG"] >= 0, sc["slotM"] >= 0, sc["slotC"] >= 0
    wantG[:, inG], wantG[:, inM], wantC[:, inC] = Gb[:, sc["slotG"][inG]], Mb[:, sc["slotM"][inM]], Cb[:, sc["slotC"][inC]]
    assert same(Gbar, wantG) and same(Cbar, wantC)
    assert inM.sum() > 0 and (Gbar[:, inM] != 0).all() and (Gbar[:, ~(inG | inM)] == 0).all()
    G1 = sol.kkt_grad_csr_cross(*idx, dz, lam, a_, beta, sol.new(B * nG), None)[0]
    C1 = sol.kkt_grad_csr_cross(*idx, dz, lam, a_, beta, None, sol.new(B * nC))[1]
    assert same(host(G1).reshape(B, -1), Gbar) and same(host(C1).reshape(B, -1), Cbar)
    sol.close()


def csr_tensors(s, grad=True, batch=None):
    dev = lambda arr, dt: torch.tensor(np.asarray(arr), dtype=dt, device="cuda:0")
    idx = dev(s.G_row, torch.int32), dev(s.G_col, torch.int32), dev(s.C_row, torch.int32), dev(s.C_col, torch.int32)
    vals = [dev(x, torch.float64).requires_grad_(grad) for x in (s.G_val, s.C_val, s.g, s.c)]
    return idx, vals


def partner(s):
    """Per G entry the index of its transposed entry within the Q and R parts (itself where there is none or off them): the
    solver takes Q_k and R_k as symmetric, so finite differences perturb an entry together with its transpose."""
    n = s.S + s.C
    rows = np.repeat(np.arange(s.N), np.diff(s.G_row))
    where = {(int(r), int(c)): e for e, (r, c) in enumerate(zip(rows, s.G_col))}
    out = np.arange(len(s.G_col))
    for e, (r, c) in enumerate(zip(rows, s.G_col)):
        if (r % n < s.S) == (c % n < s.S):
            out[e] = where.get((int(c), int(r)), e)
    return torch.from_numpy(out).cuda()


@pytest.mark.parametrize("store", ["both", "upper"])
@pytest.mark.parametrize("S,C,K", X.GRADCHECK_CELLS, ids=["%d-%d-%d" % c for c in X.GRADCHECK_CELLS])
def test_gradcheck(S, C, K, store):
    """torch.autograd.gradcheck of kkt_solve_csr(cross=True) over (G_val, C_val, g, c), the settings of tests/test_gpu_cross.py.
    Q and R entries enter symmetrised; a cross entry enters as it is: the state-row entry IS M_k (and M_k^T), its mirror is
    not read and has a zero gradient - both exact statements about the function, so gradcheck holds them."""
    cell = X.cell(S, C, K, seed=30 + K, dense_q=True)
    s = R.csr_both(cell) if store == "both" else R.csr_upper(cell, R.csr_both)
    idx, vals = csr_tensors(s)
    perm = partner(s)
    kw = dict(cross=True, rho=X.RHO, **TIGHT)

    def f(Gv, Cv, g, c):
        return ag().kkt_solve_csr(idx[0], idx[1], 0.5 * (Gv + Gv[perm]), idx[2], idx[3], Cv, g, c, **kw)

    assert torch.autograd.gradcheck(f, tuple(vals), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_gradients_against_the_dense_reference_stale_zero_and_partial():
    """The gradients of a batch on the combined-free patterns against cross_ref.dense_reference at the slots; the same gradients
    after another forward replaced the assembly; a zero upstream gradient gives zeros; only G_val requiring a gradient."""
    S, C, K, B = 4, 2, 3, 3
    cells = X.batch_cells(S, C, K, B, seed=8)
    systems = [R.csr_folded(c) for c in cells]
    idx, _ = csr_tensors(systems[0])
    _, vals = R.stacked(systems, np.float64)
    kw = dict(cross=True, rho=X.RHO, **TIGHT)
    rng = np.random.default_rng(3)
    w_dz, w_lam = rng.standard_normal((B, systems[0].N)), rng.standard_normal((B, S * K))

    def run(stale=False, only_G=False):
        t = [torch.tensor(v, dtype=torch.float64, device="cuda:0", requires_grad=(i == 0 or not only_G)) for i, v in enumerate(vals)]
        lam, dz = ag().kkt_solve_csr(idx[0], idx[1], t[0], idx[2], idx[3], t[1], t[2], t[3], **kw)
        if stale:
            with torch.no_grad():
                ag().kkt_solve_csr(idx[0], idx[1], t[0] * 1.5, idx[2], idx[3], t[1], t[2], t[3], **kw)
        ((dz * torch.tensor(w_dz, device="cuda:0")).sum() + (lam * torch.tensor(w_lam, device="cuda:0")).sum()).backward()
        return [None if x.grad is None else host(x.grad) for x in t]

    base = run()
    for b, s in enumerate(systems):
        sc = R.scatter(s)
        ref = X.dense_reference(*R.cell_of(sc, s), w_dz[b], w_lam[b])
        Mw = X.pack_M(ref["M"])
        inM = sc["slotM"] >= 0
        assert rel(base[0][b][inM], Mw[sc["slotM"][inM]]) < 1e-6
        assert (base[0][b][(sc["kind"] == R.MIRROR) | (sc["kind"] == R.OVERWRITTEN)] == 0).all()
        assert rel(base[2][b], ref["a"]) < 1e-6 and rel(base[3][b], ref["beta"]) < 1e-6
    stale = run(stale=True)
    assert all(rel(p, q) < 1e-9 for p, q in zip(stale, base))
    part = run(only_G=True)
    assert same(part[0], base[0]) and part[1] is None and part[2] is None and part[3] is None
    t = [torch.tensor(v, dtype=torch.float64, device="cuda:0", requires_grad=True) for v in vals]
    lam, dz = ag().kkt_solve_csr(idx[0], idx[1], t[0], idx[2], idx[3], t[1], t[2], t[3], **kw)
    (0.0 * dz.sum() + 0.0 * lam.sum()).backward()
    assert all((host(x.grad) == 0).all() for x in t)


def test_forward_mode_is_not_built():
    import torch.autograd.forward_ad as fwd
    s = R.csr_both(X.cell(2, 1, 3, dense_q=True))
    idx, vals = csr_tensors(s, grad=False)
    with fwd.dual_level():
        Gv = fwd.make_dual(vals[0], torch.ones_like(vals[0]))
        with pytest.raises(NotImplementedError, match="cross=True"):
            ag().kkt_solve_csr(idx[0], idx[1], Gv, idx[2], idx[3], *vals[1:], cross=True, rho=X.RHO, **TIGHT)
