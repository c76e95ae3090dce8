"""GPU suite of the forward-mode sensitivities with a cross term: cross_tangent_rhs_kernel alone
(gato_tangent_cross.hip, Solver.kkt_tangent_rhs_cross), Solver.tangents_cross and kkt_solve_tangents(M=...) end to end, and the
pairing with the backward pass of kkt_solve(M=...).

References: tests/cross_tangent_ref.py.  The kernel is held per row to 4 (2 S + 2 C + 3) eps_T scale_i: a state row of g' has at
most 2 S + 2 C + 1 terms (g., S of Q., C of M., S of C.^T, C of W^T), (n + 1) eps sum|terms| bounds a sum of n products in any
order, and the factor 4 is section 3.13's allowance for fused against unfused products.  End to end in fp64, the PCG run to
rounding, the bar is the parity bar 1e-6; fp32 is measured beside the float32 restatement.  tests/test_cross_tangent_cpu.py
asserts on the CPU that every cell here keeps the conditioning limits of the cross suite."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cross_ref as X                               # noqa: E402
import cross_tangent_ref as CT                      # noqa: E402
from f32_parity import rel                          # noqa: E402
from gato_python_amd import _lib                    # noqa: E402
from test_gpu_cross import F32_TIGHT, SOLVE_BAR, TIGHT, dev_inputs, host, math_tensors, rounded, solver      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = dict(exit_tol=1e-6, max_iters=5)            # a cross solve only to record its assembly: the kernel reads W alone
ACCURACY = []                                       # fp32: device error beside the restatement's, per cell and direction
WORST = dict(float64=0.0, float32=0.0)              # the kernel's worst error / scale, in units of eps


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()
    yield
    print("kernel worst err / (eps scale):", WORST)
    if len(ACCURACY) == 3 * len(CT.PAIR_CELLS):                             # a whole run only
        try:
            with open(os.path.join(ROOT, "profiles", "cross_tangent_accuracy.json"), "w") as f:
                json.dump(dict(margin=10.0, truth="dense float64 tangent, refined in longdouble, of the float32-rounded inputs",
                               kernel_worst_err_over_eps_scale=WORST, cells=ACCURACY), f, indent=1)
        except OSError:                                                      # a read-only tree: the record stays as committed
            pass


def gpa():
    import gato_python_amd
    return gato_python_amd


def dev(a, dt=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
def kernel_case(S, C, K, B, R, dt, seed=0):
    """B systems (the second with dense Q) rounded to dt, a random point per system and a tangent of its own draw per (system,
    direction), Q. and R. not symmetric (the kernel takes them as given), everything rounded to dt."""
    r = lambda v: np.asarray(v).astype(dt).astype(np.float64)
    cells = rounded(CT.kernel_cells(S, C, K, B), dt)
    rng = np.random.default_rng([S, C, K, B, R, seed])
    N = (S + C) * K - C
    dots = [[{n: r(v) for n, v in CT.random_dots(S, C, K, 1000 * b + 10 * rr + seed, symmetric=False).items()} for rr in range(R)]
            for b in range(B)]
    return dict(cells=cells, x=r(rng.uniform(-2.0, 2.0, (B, N))), lam=r(rng.standard_normal((B, S * K))), dots=dots)


def cross_solver(S, C, K, dt, cells):
    """A solver whose current assembly is the cross solve of the cells."""
    sol = solver(S, C, K, dt, batch=len(cells))
    sol.linsys_blocks_cross(*dev_inputs(sol, cells), QUICK["exit_tol"], QUICK["max_iters"], X.RHO)
    return sol


def device_dots(sol, case, R, drop=()):
    """The tangents of the case in the device layouts, stacked [B][R][...]; the names in drop left out (NULL)."""
    B = sol.batch
    packs = [[CT.pack_dots(case["dots"][b][rr], sol.S, sol.C, sol.K) for rr in range(R)] for b in range(B)]
    return {k: sol.to_device(np.concatenate([packs[b][rr][k] for b in range(B) for rr in range(R)]))
            for k in packs[0][0] if k not in drop and packs[0][0][k].size}


def run_kernel(sol, case, R, drop=(), offset=0, which=("tg", "gp")):
    """Solver.kkt_tangent_rhs_cross on the case -> (tg, gp, tc) as [B, R, ...] host arrays (None where not asked for); the
    outputs `offset` elements into NaN-filled allocations, the elements in front untouched."""
    B, N, sk = sol.batch, sol.N, sol.sizes["sk"]
    d = lambda v: sol.to_device(np.ascontiguousarray(v).reshape(-1))
    base = dict(tg=sol.new(B * R * N + offset).fill_(float("nan")), gp=sol.new(B * R * N + offset).fill_(float("nan")),
                tc=sol.new(B * R * sk + offset).fill_(float("nan")))
    outs = {k: base[k][offset:] for k in which + ("tc",)}
    tg, gp, tc = sol.kkt_tangent_rhs_cross(R, d(case["x"]), d(case["lam"]), **device_dots(sol, case, R, drop), **outs)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[:offset]).all()) for t in base.values())
    view = lambda t, per: None if t is None else host(t).astype(np.float64).reshape(B, R, per)
    return view(tg, N), view(gp, N), view(tc, sk)


DROPS = dict(G_dot=("Q", "R"), M_dot=("M",), C_dot=("A", "B"), g_dot=("q", "r"), c_dot=("c",))


def check_kernel(sol, case, got, dt, drop=(), knots=None):
    """tg, tc within f eps scale_i and gp within f eps scale'_i (from the device's own stored W) of the float64 formulas; knots:
    compare those knots alone."""
    S, C, K, n = sol.S, sol.C, sol.K, sol.S + sol.C
    tg, gp, tc = got
    B, R = tc.shape[:2]
    f = 4 * (2 * S + 2 * C + 3)
    eps = float(np.finfo(dt).eps)
    W = sol.read_cross("W").reshape(B, sol.M_size).astype(np.float64)
    gone = {name for k in drop for name in DROPS[k]}
    worst = 0.0
    vs = slice(None) if knots is None else slice(knots.start * n, None)
    cs = slice(None) if knots is None else slice(knots.start * S, None)
    for b in range(B):
        Wb = X.unpack_W(W[b], S, C, K)
        for rr in range(R):
            dots = {k: v for k, v in case["dots"][b][rr].items() if k not in gone}
            wg, wc, sg, sc = CT.tangent_rhs(case["x"][b], case["lam"][b], S, C, K, dots)
            wp, sp = CT.transform_rhs(Wb, wg, sg, S, C, K)
            for name, g, w, s in (("tg", tg, wg[vs], sg[vs]), ("gp", gp, wp[vs], sp[vs]), ("tc", tc, wc[cs], sc[cs])):
                if g is None:
                    continue
                e = np.abs(g[b, rr][cs if name == "tc" else vs] - w)
                assert np.all(np.isfinite(e)) and np.all(e <= f * eps * s), (name, b, rr, drop, float((e / np.maximum(s, 1e-300)).max() / eps))
                worst = max(worst, float((e[s > 0] / s[s > 0]).max(initial=0.0)) / eps)
                assert drop or np.abs(w).max() > 0
    WORST[np.dtype(dt).name] = max(WORST[np.dtype(dt).name], worst)
    print("%d/%d/%d %s B%d R%d: worst err / (eps scale) %.3g, bar %d" % (S, C, K, np.dtype(dt).name, B, R, worst, f))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("K", CT.KERNEL_K)
@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_cross_tangent_rhs_kernel(shape, K, dt):
    """All six shapes, K = 2 and 3 (every knot a first or a last one) and 9, both precisions, B = 1 with R = 1 and B = 3 with R = 3
    (each direction its own draw: a stride slip shows), the tangent blocks staged through LDS.  gp is cross_rhs of the same
    call's tg value for value, a repeat gives the same bits, and so do the form that reads the blocks in place and the entry's
    own choice between the two."""
    S, C = shape
    for B, R in ((1, 1), (3, 3)):
        case = kernel_case(S, C, K, B, R, dt)
        sol = cross_solver(S, C, K, dt, case["cells"])
        sol.set_option("cross_tangent_form", 1)                              # staged through LDS, whatever the launch's size
        got = run_kernel(sol, case, R)
        check_kernel(sol, case, got, dt)
        fused = host(sol.cross_rhs(sol.to_device(got[0].astype(dt).reshape(-1)))).astype(np.float64).reshape(got[1].shape)
        assert fused.tobytes() == got[1].tobytes()
        again = run_kernel(sol, case, R)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
        for form in (2, 0):                                                  # in place; the form the entry picks by itself
            sol.set_option("cross_tangent_form", form)
            other = run_kernel(sol, case, R)
            assert all(a.tobytes() == g.tobytes() for a, g in zip(other, got)), form
        sol.close()


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape,K", [((6, 3), 3), ((14, 7), 9)], ids=["6-3-3", "14-7-9"])
def test_null_pointers_either_output_and_unaligned_outputs(shape, K, dt):
    """Each tangent pointer NULL in turn (the reference with that tangent zero; the result differs from the whole one, so the
    tangent was read when given), all NULL (exact zeros), tg alone and gp alone (the bits of the call with both), outputs one
    element off the 16-byte grid.  B = R = 3."""
    S, C = shape
    B = R = 3
    case = kernel_case(S, C, K, B, R, dt, seed=1)
    sol = cross_solver(S, C, K, dt, case["cells"])
    sol.set_option("cross_tangent_form", 1)
    whole = run_kernel(sol, case, R)
    for name in DROPS:
        got = run_kernel(sol, case, R, drop=(name,))
        check_kernel(sol, case, got, dt, drop=(name,))
        assert any(g.tobytes() != w.tobytes() for g, w in zip(got, whole)), name
        sol.set_option("cross_tangent_form", 2)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(run_kernel(sol, case, R, drop=(name,)), got)), name
        sol.set_option("cross_tangent_form", 1)
    tg, gp, tc = run_kernel(sol, case, R, drop=tuple(DROPS))
    assert not tg.any() and not gp.any() and not tc.any()
    only_tg, only_gp = run_kernel(sol, case, R, which=("tg",)), run_kernel(sol, case, R, which=("gp",))
    assert only_tg[1] is None and only_gp[0] is None
    assert only_tg[0].tobytes() == whole[0].tobytes() and only_gp[1].tobytes() == whole[1].tobytes()
    assert only_tg[2].tobytes() == whole[2].tobytes() and only_gp[2].tobytes() == whole[2].tobytes()
    shifted = run_kernel(sol, case, R, offset=1)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(shifted, whole))
    sol.close()


def test_second_pass_of_the_knot_stride():
    """2/1/8197: the grid has 8192 workgroups, so knots 8192 .. 8196 (the last one without M) are a workgroup's second knot;
    they are compared alone, then all."""
    S, C, K = X.STRIDE_CELL
    case = kernel_case(S, C, K, 1, 1, np.float64, seed=2)
    sol = cross_solver(S, C, K, np.float64, case["cells"])
    sol.set_option("cross_tangent_form", 1)
    got = run_kernel(sol, case, 1)
    check_kernel(sol, case, got, np.float64, knots=slice(8192, None))
    check_kernel(sol, case, got, np.float64)
    sol.set_option("cross_tangent_form", 2)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(run_kernel(sol, case, 1), got))
    sol.close()


@pytest.mark.parametrize("shape", [(4, 2), (14, 7)], ids=["4-2", "14-7"])
def test_one_knot_is_the_plain_right_hand_side(shape):
    """K = 1 has no M and no C: a NULL M_dot, gp = tg = g. - Q. x and tc = c., the values of the kernel without a cross term."""
    S, C = shape
    case = kernel_case(S, C, 1, 2, 2, np.float64, seed=3)
    sol = solver(S, C, 1, np.float64, batch=2)
    Gb, _, _, g, c = dev_inputs(sol, case["cells"])
    sol.linsys_blocks_cross(Gb, None, None, g, c, QUICK["exit_tol"], QUICK["max_iters"], X.RHO)
    d = lambda v: sol.to_device(np.ascontiguousarray(v).reshape(-1))
    dots = device_dots(sol, case, 2)
    assert "M_dot" not in dots and "C_dot" not in dots
    tg, gp, tc = sol.kkt_tangent_rhs_cross(2, d(case["x"]), d(case["lam"]), **dots)
    tg0, tc0 = sol.kkt_tangent_rhs(2, d(case["x"]), d(case["lam"]), **dots)
    assert torch.equal(tg, tg0) and torch.equal(gp, tg0) and torch.equal(tc, tc0) and torch.equal(tc, dots["c_dot"])
    for b in range(2):
        for rr in range(2):
            wg = CT.tangent_rhs(case["x"][b], case["lam"][b], S, C, 1, case["dots"][b][rr])[0]
            assert rel(host(tg).reshape(2, 2, S)[b, rr], wg) < 1e-13
    sol.close()


def test_the_entry_needs_the_cross_assembly_and_checks_its_arguments():
    """After nothing at all, a plain linsys_blocks or a cross_prepare alone the assembly is not a cross one: EINVAL with the
    reason of solve_rhs_cross; a cross solve makes it one again.  R < 1, no output, a missing point: refused."""
    S, C, K = 4, 2, 3
    cells = CT.kernel_cells(S, C, K, 1)
    sol = solver(S, C, K)
    Gb, Mb, Cb, g, c = inp = dev_inputs(sol, cells)
    lam, dz = sol.new(S * K), sol.new(sol.N)
    gen = lambda: sol.get_option("assembly_gen")

    def refused():
        with pytest.raises(_lib.GatoError, match="not that of a cross solve") as e:
            sol.kkt_tangent_rhs_cross(1, dz, lam, g_dot=g)
        assert e.value.code == -1
        with pytest.raises(_lib.GatoError, match="not that of a cross solve"):
            sol.tangents_cross(1, dz, lam, 1e-10, 100, g_dot=g)

    refused()
    sol.linsys_blocks_cross(*inp, 1e-10, 100, X.RHO, lam, dz)
    before = gen()
    sol.kkt_tangent_rhs_cross(1, dz, lam, g_dot=g)
    assert gen() == before                                                   # no solver state is written
    sol.linsys_blocks(Gb, Cb, g, c, 1e-10, 100, X.RHO, lam, dz)
    refused()
    sol.linsys_blocks_cross(*inp, 1e-10, 100, X.RHO, lam, dz)
    sol.cross_prepare(Gb, Mb, Cb, g, X.RHO)
    refused()
    sol.linsys_blocks_cross(*inp, 1e-10, 100, X.RHO, lam, dz)
    L, p = _lib.lib(), lambda t: None if t is None else int(t.data_ptr())
    out = sol.new(sol.N)
    for R, x_, lam_, tg_, gp_, tc_, word in ((0, dz, lam, out, None, lam, b"at least one"), (1, None, lam, out, None, lam, b"required"),
                                           (1, dz, None, out, None, lam, b"required"), (1, dz, lam, None, None, lam, b"required"),
                                           (1, dz, lam, out, out, None, b"required")):
        assert L.gato_kkt_tangent_rhs_cross(sol._h, R, None, None, None, p(g), None, p(x_), p(lam_), p(tg_), p(gp_), p(tc_), sol._stream()) == -1
        assert word in L.gato_last_error()
    assert L.gato_kkt_tangent_rhs_cross(None, 1, None, None, None, None, None, p(dz), p(lam), p(out), None, p(lam), None) == -1
    with pytest.raises(ValueError, match="M_dot"):
        sol.kkt_tangent_rhs_cross(2, dz, lam, M_dot=Mb)                      # R = 2 needs B R (K-1) S C entries
    with pytest.raises(ValueError, match="at least one"):
        sol.kkt_tangent_rhs_cross(0, dz, lam)
    sol.close()


# ---- 2. end to end in fp64 ---------------------------------------------------------------------------------------------------------
def stacked_dots(dots, B, R, names, dt=torch.float64):
    """dots[b][rr] (math-shaped) -> the tangents argument: name -> [B, R, ...] (B = 1: [R, ...])."""
    out = {}
    for n in names:
        a = np.stack([np.stack([dots[b][rr][n] for rr in range(R)]) for b in range(B)])
        out[n] = dev(a if B > 1 else a[0], dt)
    return out


def pick(t, b, B):
    return host(t[b] if B > 1 else t).astype(np.float64)


ENDS = [(S, C, K, B) for S, C, K in CT.SOLVE_CELLS for B in (1, 3)]


@pytest.mark.parametrize("S,C,K,B", ENDS, ids=["%d-%d-%d-B%d" % c for c in ENDS])
def test_kkt_solve_tangents_with_M_against_the_dense_reference(S, C, K, B):
    """R = 1 and R = 3 directions over all eight inputs: the point and every tangent within 1e-6 of the dense cross solves; two
    calls in a row give the same bits; the inputs are not written; nothing carries a grad_fn."""
    tangents_case(S, C, K, CT.solve_cells(S, C, K, B), (1, 3), TIGHT)


def tangents_case(S, C, K, cells, Rs, pcg):
    """The body of test_kkt_solve_tangents_with_M_against_the_dense_reference on the given cells, for every R of Rs, at the PCG
    settings pcg (exit_tol, max_iters) -> the worst error."""
    B = len(cells)
    t, Mt = math_tensors(cells)
    kw = dict(rho=X.RHO, **pcg)
    worst = 0.0
    for R in Rs:
        dots = [[CT.random_dots(S, C, K, 100 * b + rr + R) for rr in range(R)] for b in range(B)]
        tan = stacked_dots(dots, B, R, CT.NAMES)
        keep = [x.clone() for x in t + [Mt] + list(tan.values())]
        lam, dz, lam_d, dz_d = gpa().kkt_solve_tangents(*t, tan, M=Mt, **kw)
        N, sk = (S + C) * K - C, S * K
        lead = (B,) if B > 1 else ()
        assert lam_d.shape == lead + (R, sk) and dz_d.shape == lead + (R, N) and dz_d.grad_fn is None and lam.grad_fn is None
        for b, (blocks, M) in enumerate(cells):
            for rr in range(R):
                x_w, lam_w, xd_w, lamd_w = CT.dense_tangent(blocks, M, dots[b][rr])
                e = (rel(pick(dz, b, B), x_w), rel(pick(lam, b, B), lam_w), rel(pick(dz_d, b, B)[rr], xd_w), rel(pick(lam_d, b, B)[rr], lamd_w))
                print("%d/%d/%d B%d R%d sys %d dir %d: dz %.3g lam %.3g dz. %.3g lam. %.3g" % (S, C, K, B, R, b, rr, *e))
                assert max(e) < SOLVE_BAR, (b, rr, e)
                worst = max(worst, *e)
        again = gpa().kkt_solve_tangents(*t, tan, M=Mt, **kw)
        assert all(torch.equal(a, g) for a, g in zip(again, (lam, dz, lam_d, dz_d)))
        assert all(torch.equal(a, g) for a, g in zip(keep, t + [Mt] + list(tan.values())))
    return worst


def test_a_zero_direction_among_nonzero_ones_is_exactly_zero():
    """The 0/0 rule per (system, direction): direction 1 of system 0 and every direction of system 2 are zero tangents (M.
    included); they come back as exact zeros, the others as the reference's."""
    S, C, K, B, R = 6, 3, 3, 3, 3
    cells = CT.solve_cells(S, C, K, B)
    names = ("q", "c", "A", "M")
    dots = [[CT.random_dots(S, C, K, 7 * b + rr, names) for rr in range(R)] for b in range(B)]
    for b, rr in ((0, 1), (2, 0), (2, 1), (2, 2)):
        dots[b][rr] = {n: 0.0 * v for n, v in dots[b][rr].items()}
    t, Mt = math_tensors(cells)
    lam, dz, lam_d, dz_d = gpa().kkt_solve_tangents(*t, stacked_dots(dots, B, R, names), M=Mt, rho=X.RHO, **TIGHT)
    assert torch.isfinite(lam_d).all() and torch.isfinite(dz_d).all()
    for b, (blocks, M) in enumerate(cells):
        for rr in range(R):
            if not any(v.any() for v in dots[b][rr].values()):
                assert not dz_d[b, rr].any() and not lam_d[b, rr].any(), (b, rr)
            else:
                _, _, xd_w, lamd_w = CT.dense_tangent(blocks, M, dots[b][rr])
                assert rel(host(dz_d[b, rr]), xd_w) < SOLVE_BAR and rel(host(lam_d[b, rr]), lamd_w) < SOLVE_BAR, (b, rr)


def test_zero_M_agrees_with_the_call_without_M():
    """M = 0 and no M.: W = 0, and the point and tangents agree with kkt_solve_tangents without M to the parity bar; M = None
    with a tangent named M is refused; K = 1 with an empty M is the plain path bit for bit."""
    S, C, K, B, R = 14, 7, 9, 3, 2
    cells = CT.solve_cells(S, C, K, B)
    t, Mt = math_tensors(cells)
    names = CT.NAMES[:7]
    dots = [[CT.random_dots(S, C, K, 30 + 5 * b + rr, names) for rr in range(R)] for b in range(B)]
    tan = stacked_dots(dots, B, R, names)
    kw = dict(rho=X.RHO, **TIGHT)
    plain = gpa().kkt_solve_tangents(*t, tan, **kw)
    zero = gpa().kkt_solve_tangents(*t, tan, M=torch.zeros_like(Mt), **kw)
    for a, g in zip(zero, plain):
        assert rel(host(a), host(g)) < SOLVE_BAR
    with pytest.raises(ValueError, match="tangent of M needs"):
        gpa().kkt_solve_tangents(*t, dict(tan, M=torch.zeros((B, R) + tuple(Mt.shape[1:]), dtype=Mt.dtype, device=Mt.device)), **kw)
    one = CT.solve_cells(4, 2, 1, 1)
    t1, M1 = math_tensors(one)
    assert M1.shape == (0, 4, 2)
    d1 = stacked_dots([[CT.random_dots(4, 2, 1, 3, ("Q", "q", "c"))]], 1, 1, ("Q", "q", "c"))
    a = gpa().kkt_solve_tangents(*t1, d1, **kw)
    b = gpa().kkt_solve_tangents(*t1, d1, M=M1, **kw)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_tangents_cross_after_another_solve_raises_and_repeats_on_its_own_assembly():
    """Solver.tangents_cross re-solves the CURRENT assembly and leaves it the cross one: a second call gives the same bits; after
    a plain solve of the same solver it raises."""
    S, C, K = 4, 2, 3
    cells = CT.solve_cells(S, C, K, 1)
    sol = solver(S, C, K)
    Gb, Mb, Cb, g, c = inp = dev_inputs(sol, cells)
    lam, dz = sol.new(S * K), sol.new(sol.N)
    sol.linsys_blocks_cross(*inp, TIGHT["exit_tol"], TIGHT["max_iters"], X.RHO, lam, dz)
    gen = sol.get_option("assembly_gen")
    dots = {k: sol.to_device(v) for k, v in CT.pack_dots(CT.random_dots(S, C, K, 5), S, C, K).items()}
    l1, x1 = sol.tangents_cross(1, dz, lam, TIGHT["exit_tol"], TIGHT["max_iters"], **dots)
    l2, x2 = sol.tangents_cross(1, dz, lam, TIGHT["exit_tol"], TIGHT["max_iters"], **dots)
    assert torch.equal(l1, l2) and torch.equal(x1, x2) and sol.get_option("assembly_gen") == gen
    _, _, xd_w, lamd_w = CT.dense_tangent(*cells[0], CT.random_dots(S, C, K, 5))
    assert rel(host(x1[0, 0]), xd_w) < SOLVE_BAR and rel(host(l1[0, 0]), lamd_w) < SOLVE_BAR
    sol.linsys_blocks(Gb, Cb, g, c, 1e-10, 100, X.RHO)
    with pytest.raises(_lib.GatoError, match="not that of a cross solve"):
        sol.tangents_cross(1, dz, lam, TIGHT["exit_tol"], TIGHT["max_iters"], **dots)
    sol.close()


# ---- 3. the pairing with the existing backward pass ----------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", CT.PAIR_CELLS, ids=["%d-%d-%d" % c for c in CT.PAIR_CELLS])
def test_pairing_with_the_backward_of_kkt_solve(S, C, K):
    """|<v, J u> - <J^T v, u>| <= 1e-6 (|v|_1 max(1, |J u|_inf) + |u|_1 max(1, |J^T v|_inf)), section 3.13's pairing bar: J u from
    kkt_solve_tangents(M=...), J^T v from kkt_solve(M=...).backward, u over all eight inputs (Q., R. symmetric).  M. enters the
    forward as M_bar leaves the backward: M_k and M_k^T together."""
    (blocks, M), = CT.solve_cells(S, C, K, 1)
    u = CT.random_dots(S, C, K, 21)
    t, Mt = math_tensors([(blocks, M)])
    kw = dict(rho=X.RHO, **TIGHT)
    _, _, lam_d, dz_d = gpa().kkt_solve_tangents(*t, {n: dev(u[n][None]) for n in CT.NAMES}, M=Mt, **kw)
    Ju = [host(lam_d[0]).astype(np.float64), host(dz_d[0]).astype(np.float64)]
    rng = np.random.default_rng(22)
    v = [rng.standard_normal(a.shape) for a in Ju]
    tg, Mg = math_tensors([(blocks, M)], grad=True)
    lam, dz = gpa().kkt_solve(*tg, M=Mg, **kw)
    ((lam * dev(v[0])).sum() + (dz * dev(v[1])).sum()).backward()
    JTv = {n: host(x.grad).astype(np.float64) for n, x in zip(CT.NAMES, tg + [Mg])}
    lhs = sum(float((a * b).sum()) for a, b in zip(v, Ju))
    rhs = sum(float((JTv[n] * u[n]).sum()) for n in CT.NAMES)
    only_M = float((JTv["M"] * u["M"]).sum())
    l1 = lambda xs: sum(float(np.abs(x).sum()) for x in xs)
    linf = lambda xs: max(float(np.abs(x).max()) for x in xs)
    bar = 1e-6 * (l1(v) * max(1.0, linf(Ju)) + l1(list(u.values())) * max(1.0, linf(list(JTv.values()))))
    print("<v, J u>", lhs, "<J^T v, u>", rhs, "of which M", only_M, "difference", abs(lhs - rhs), "bar", bar)
    assert np.isfinite(lhs) and abs(lhs) > 0 and abs(only_M) > 0 and abs(lhs - rhs) <= bar
    # M. alone: the pairing then rests on M_bar only
    _, _, lam_m, dz_m = gpa().kkt_solve_tangents(*t, {"M": dev(u["M"][None])}, M=Mt, **kw)
    lhs_m = float((v[0] * host(lam_m[0])).sum() + (v[1] * host(dz_m[0])).sum())
    bar_m = 1e-6 * (l1(v) * max(1.0, float(max(lam_m.abs().max(), dz_m.abs().max()))) + l1([u["M"]]) * max(1.0, linf([JTv["M"]])))
    print("M alone: <v, J u>", lhs_m, "<M_bar, M.>", only_M, "bar", bar_m)
    assert abs(lhs_m - only_M) <= bar_m


# ---- 4. fp32 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,K", CT.PAIR_CELLS, ids=["%d-%d-%d" % c for c in CT.PAIR_CELLS])
def test_fp32_beside_the_float32_restatement(S, C, K):
    """Three directions of one system at F32_TIGHT (both sides run to rounding): the device's error against the dense float64
    tangent of the float32-rounded inputs is at most 10 x the error of the float32 restatement (cross_tangent_ref.restatement32),
    the margin of DESIGN.md section 3.15 for this comparison.  Both numbers go to profiles/cross_tangent_accuracy.json."""
    R = 3
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    cells = rounded(CT.solve_cells(S, C, K, 1), np.float32)
    (blocks, M), = cells
    dots = [{n: f32(v) for n, v in CT.random_dots(S, C, K, 40 + rr).items()} for rr in range(R)]
    t, Mt = math_tensors(cells, torch.float32)
    lam, dz, lam_d, dz_d = gpa().kkt_solve_tangents(*t, stacked_dots([dots], 1, R, CT.NAMES, torch.float32), M=Mt, rho=X.RHO, **F32_TIGHT)
    rho32 = np.float64(np.float32(X.RHO))
    for rr in range(R):
        _, _, xd_w, lamd_w = CT.dense_tangent(blocks, M, dots[rr], rho=rho32)
        xd_r, lamd_r = CT.restatement32(blocks, M, dots[rr], F32_TIGHT["exit_tol"], F32_TIGHT["max_iters"])
        eg = max(rel(host(dz_d[rr]), xd_w), rel(host(lam_d[rr]), lamd_w))
        er = max(rel(xd_r, xd_w), rel(lamd_r, lamd_w))
        ACCURACY.append(dict(S=S, C=C, K=K, direction=rr, err_device=float(eg), err_restatement32=float(er)))
        print("fp32 %d/%d/%d dir %d: device %.3g restatement %.3g" % (S, C, K, rr, eg, er))
        assert eg <= 10.0 * er, (rr, eg, er)
