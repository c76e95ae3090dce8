"""Forward-mode sensitivities on the device (gato_kkt_tangent_rhs in gato_tangent.hip, Solver.kkt_tangent_rhs / tangents, the jvp
of kkt_solve and box_qp_layer, kkt_solve_tangents, box_qp_layer_tangents) against tests/kkt_tangent_ref.py.

The kernel alone is held per row to 4 (3 S + C + 6) eps_T scale_i, scale_i the sum of the absolute values of the row's terms: a
row has at most 3 S + C + 5 terms, (n + 1) eps sum|terms| bounds a sum of n products in any order, and the factor 4 covers fused
against unfused products.  Rows of t_g on the hard-active set are not compared (the reduced system ignores them).  End to end,
fp64 with the PCG run to rounding, the bar is that of the gradients: 1e-6 max(1, |want|)."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

pytestmark = pytest.mark.gpu

import box_qp_linesearch_ref as L                 # noqa: E402
import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_polish_ref as P                     # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
import kkt_tangent_ref as T                       # noqa: E402
from box_qp_device import CAP, SENTINEL, dev_inputs, solver      # noqa: E402
from f32_parity import check_f32                   # noqa: E402
from gato_python_amd import _lib, synth            # noqa: E402
from oracle import gato_oracle as o                # noqa: E402
from test_gpu_kkt_grad import TIGHT                # noqa: E402
from test_gpu_resolve import tol_mi                # noqa: E402

BAR = 1e-6
FORMS = ("hard", "soft", "capped")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def gpa():
    import gato_python_amd
    return gato_python_amd


def dev(a, dt=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


def close(got, want, what):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(what, "max err", float(err.max()), "of", float(np.abs(want).max()))
    assert np.isfinite(got).all() and err.max() <= BAR, (what, float(err.max()))


# ---- 1. the kernel as a function of its arrays ---------------------------------------------------------------------------------
def kernel_case(S, C, K, B, R, dt, form):
    """Per system, everything rounded to dt and of its own draw (the recipe of the bound-gradient kernels' array tests): a
    dense-block system, a point, a box with a tenth of the sides infinite and a few lo == hi, weights on about half the variables
    (soft, capped), finite caps on about half of those (capped), a random legal act - 0 on x_0 and where the bound of its side is
    infinite, -1 where lo == hi, +-2 only on a weighted variable with a finite cap - with a hard-active and a soft-active variable
    forced among the states of the last knot and of knot 1 and among the controls of knot 0 (the soft control saturated where
    capped; 2/1 has one control: soft or saturated in system 0, hard in the others), and a third, saturated state in the last
    knot where S >= 4.  Every tangent is random everywhere and differs per (system, direction)."""
    rng = np.random.default_rng([S, C, K, B, R, FORMS.index(form), 29])
    n = S + C
    r = lambda v: np.asarray(v, dt).astype(np.float64)
    systems = [P.constructed_system(S, C, K, 60 + b).astype(dt).astype(np.float64) for b in range(B)]
    N, sk = systems[0].N, S * K
    lo, hi = r(-rng.uniform(0.5, 1.5, (B, N))), r(rng.uniform(0.5, 1.5, (B, N)))
    lo[rng.random((B, N)) < 0.1] = -np.inf
    hi[rng.random((B, N)) < 0.1] = np.inf
    eq = (rng.random((B, N)) < 0.05) & np.isfinite(lo)
    hi[eq] = lo[eq]
    w = r(np.where(rng.random((B, N)) < 0.5, 10.0 ** rng.uniform(0.0, 3.0, (B, N)), 0.0))
    m = r(np.where(rng.random((B, N)) < 0.5, 10.0 ** rng.uniform(-1.0, 1.0, (B, N)), np.inf))
    act = rng.integers(-1, 2, (B, N)).astype(np.int8)
    act = np.where(rng.random((B, N)) < 0.5, 2 * act, act).astype(np.int8)
    last = (K - 1) * n
    forced = [(last, 1, "soft"), (last + 1, -1, "hard")] + ([(last + 2, -1, "sat")] if S >= 4 else [])
    if K > 2:
        forced += [(n, -1, "soft"), (n + 1, 1, "hard")]
    for b in range(B):
        ctl = [(S, 1, "sat"), (S + 1, -1, "hard")] if C > 1 else [(S, 1, "sat" if b == 0 else "hard")]
        for j, ai, kind in forced + ctl:
            lo[b, j], hi[b, j] = r(-0.75 - 0.01 * b), r(0.8 + 0.01 * b)
            act[b, j] = (ai if b % 2 == 0 else -ai) * (2 if kind == "sat" else 1)
            w[b, j] = 0.0 if kind == "hard" else r(7.0 + 3.0 * b)
            m[b, j] = r(0.5 + 0.1 * b) if kind == "sat" else np.inf
    if form == "hard":
        w = None
    if form != "capped":
        m = None
    ok2 = (w > 0) & np.isfinite(m) if form == "capped" else np.zeros((B, N), bool)
    act = np.where((np.abs(act) == 2) & ~ok2, np.sign(act), act).astype(np.int8)
    act[lo == hi] = -1
    act[(act > 0) & ~np.isfinite(hi)] = 0
    act[(act < 0) & ~np.isfinite(lo)] = 0
    act[:, :S] = 0
    case = dict(systems=systems, act=act, w=w, m=m, lo=lo, hi=hi, x=r(rng.uniform(-2.0, 2.0, (B, N))), lam=r(rng.standard_normal((B, sk))))
    sizes = dict(G_dot=systems[0].K * (S * S + C * C) - C * C, C_dot=(K - 1) * (S * S + S * C), c_dot=sk)
    for name in T.DOTS:
        case[name] = r(rng.standard_normal((B, R, sizes.get(name, N))))
    return case


def run_kernel(sol, case, R, drop=(), offset=0):
    """Solver.kkt_tangent_rhs on the case with the tangents in `drop` passed as NULL, the outputs `offset` elements into their
    allocations behind a sentinel -> (t_g [B, R, N], t_c [B, R, S K]) as fp64."""
    B, N, sk = sol.batch, sol.N, sol.sizes["sk"]
    inf = np.full(N, np.inf)
    Gb, Cb = dev_inputs(sol, case["systems"], [(-inf, inf)] * B)[:2]
    d = lambda v: None if v is None else sol.to_device(np.ascontiguousarray(v).reshape(-1))
    dots = {k: d(case[k]) for k in T.DOTS if k not in drop}
    base = [sol.new(B * R * per + offset).fill_(SENTINEL) for per in (N, sk)]
    tg, tc = sol.kkt_tangent_rhs(R, d(case["x"]), d(case["lam"]), Gb=Gb, Cb=Cb, act=sol.to_device(case["act"].reshape(-1), np.int8),
                                 soft_weight=d(case["w"]), soft_cap=d(case["m"]), lo=d(case["lo"]), hi=d(case["hi"]),
                                 tg=base[0][offset:], tc=base[1][offset:], **dots)
    torch.cuda.synchronize()
    assert all(float(t[i]) == SENTINEL for t in base for i in range(offset))
    return npy(tg).reshape(B, R, N), npy(tc).reshape(B, R, sk)


def kernel_reference(case, b, rr, S, C, K, drop=(), sparse=False):
    s = case["systems"][b]
    Gd, Cd = o.convert(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, S, C, K, 0.0)
    dots = {k: case[k][b, rr] for k in T.DOTS if k not in drop}
    if "G_dot" in dots:
        dots["G_dot"] = T.dense_G(dots["G_dot"], S, C, K, sparse)
    if "C_dot" in dots:
        dots["C_dot"] = T.dense_C(dots["C_dot"], S, C, K, False, sparse)
    pick = lambda k: None if case[k] is None else case[k][b]
    return T.tangent_rhs(T.dense_G(Gd, S, C, K, sparse), T.dense_C(Cd, S, C, K, True, sparse), case["x"][b], case["lam"][b],
                         case["act"][b], pick("w"), case["lo"][b], case["hi"][b], **dots)


def check_kernel(case, got, S, C, K, dt, drop=(), sparse=False, tail=None):
    tg, tc = got
    B, R = tg.shape[:2]
    factor = 4 * (3 * S + C + 6) * np.finfo(dt).eps
    worst = 0.0
    for b in range(B):
        hard = T.sets(case["act"][b], None if case["w"] is None else case["w"][b])[0]
        for rr in range(R):
            wg, wc, sg, sc = kernel_reference(case, b, rr, S, C, K, drop, sparse)
            eg, ec = np.abs(tg[b, rr] - wg)[~hard], np.abs(tc[b, rr] - wc)
            assert np.all(eg <= factor * sg[~hard]) and np.all(ec <= factor * sc), (b, rr, drop)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, np.nanmax(eg / sg[~hard], initial=0.0), np.nanmax(ec / sc, initial=0.0))
            assert np.abs(wg[~hard]).max() > 0 and np.abs(wc).max() > 0
            if tail is not None:
                assert np.abs(wg[tail][~hard[tail]]).max() > 0
    print("worst err / scale", worst, "bar", factor)


def cover(case, S, C, K):
    """Some knot of some system holds a hard-active variable and a soft-active one (soft, capped) and a saturated one (capped)."""
    n = S + C
    found = False
    for b in range(case["act"].shape[0]):
        hard, soft, sat = T.sets(case["act"][b], None if case["w"] is None else case["w"][b])
        knot = np.arange(len(hard)) // n
        ks = set(knot[hard])
        if case["w"] is not None:
            ks &= set(knot[soft])
        if case["m"] is not None and S >= 4:
            ks &= set(knot[sat])
        found |= bool(ks)
    return found


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("K", [2, 3, 9])
@pytest.mark.parametrize("shape", P.SWEEP_SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_tangent_rhs_kernel(shape, K, dt, form):
    """All six shapes, K = 2 and 3 (every knot a first or a last one) and 9, both precisions, the three forms of the bounds, B =
    1 with R = 1 and B = 3 with R = 3 (each direction its own draw: a stride slip shows); a repeat gives the same bits."""
    S, C = shape
    for B, R in ((1, 1), (3, 3)):
        case = kernel_case(S, C, K, B, R, dt, form)
        assert cover(case, S, C, K) or B == 1
        sol = solver(S, C, K, dt, batch=B)
        got = run_kernel(sol, case, R)
        check_kernel(case, got, S, C, K, dt)
        again = run_kernel(sol, case, R)
        assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
        sol.close()


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape,K", [((6, 3), 3), ((14, 7), 9)], ids=["6-3-3", "14-7-9"])
def test_tangent_rhs_null_pointers_and_unaligned_outputs(shape, K, dt):
    """Each tangent pointer NULL in turn (the reference with that tangent zero), all NULL (exact zeros), outputs one element
    into their allocations (no 16-byte alignment) with the element in front untouched.  B = R = 3, capped."""
    S, C = shape
    B = R = 3
    case = kernel_case(S, C, K, B, R, dt, "capped")
    sol = solver(S, C, K, dt, batch=B)
    whole = run_kernel(sol, case, R)
    for name in T.DOTS:
        got = run_kernel(sol, case, R, drop=(name,))
        check_kernel(case, got, S, C, K, dt, drop=(name,))
        assert any(g.tobytes() != w.tobytes() for g, w in zip(got, whole)), name      # the tangent was read when given
    tg, tc = run_kernel(sol, case, R, drop=T.DOTS)
    assert not tg.any() and not tc.any()
    shifted = run_kernel(sol, case, R, offset=1)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(shifted, whole))
    # without an act (a plain solve) the bound, weight and cap tangents are not read and the blocks may be NULL
    d = lambda v: sol.to_device(np.ascontiguousarray(v).reshape(-1))
    tg, tc = sol.kkt_tangent_rhs(R, d(case["x"]), d(case["lam"]), **{k: d(case[k]) for k in T.DOTS[:4]})
    torch.cuda.synchronize()
    plain = dict(case, act=np.zeros_like(case["act"]), w=None, m=None)
    check_kernel(plain, (npy(tg).reshape(B, R, -1), npy(tc).reshape(B, R, -1)), S, C, K, dt)
    sol.close()


def test_tangent_rhs_past_the_grid_cap():
    """2/1/8197: the knots from 8192 on are a second pass of the knot loop."""
    S, C, K = P.SWEEP_LONG
    case = kernel_case(S, C, K, 1, 1, np.float64, "capped")
    sol = solver(S, C, K, np.float64)
    got = run_kernel(sol, case, 1)
    check_kernel(case, got, S, C, K, np.float64, sparse=True, tail=slice(CAP * (S + C), None))
    sol.close()


def test_tangent_rhs_refusals():
    sol = solver(6, 3, 3, np.float64, batch=2)
    x, lam = sol.new(2 * sol.N).zero_(), sol.new(2 * sol.sizes["sk"]).zero_()
    with pytest.raises(ValueError, match="g_dot"):
        sol.kkt_tangent_rhs(2, x, lam, g_dot=sol.new(2 * sol.N))               # R = 2 needs B R N entries
    with pytest.raises(ValueError, match="at least one"):
        sol.kkt_tangent_rhs(0, x, lam)
    with pytest.raises(ValueError, match="Gb"):
        sol.kkt_tangent_rhs(1, x, lam, act=torch.zeros(2 * sol.N, dtype=torch.int8, device="cuda"))
    L_ = _lib.lib()
    assert L_.gato_kkt_tangent_rhs(sol._h, 1, *([None] * 8), None, None, *([None] * 7), None, None, None) != 0
    assert "required" in L_.gato_last_error().decode()
    sol.close()


# ---- 2. kkt_solve end to end ---------------------------------------------------------------------------------------------------
KKT_SHAPES = [(2, 1, 5), (6, 3, 3), (14, 7, 9)]


def kkt_system(S, C, K, b=0):
    """(math dict, rho): the pendulum literals at 2/1/5 (system b > 0: their right-hand sides scaled and Q shifted), seeded
    dense-Q blocks elsewhere."""
    if (S, C, K) == (2, 1, 5):
        s = synth.pendulum_system()
        blocks = [np.array(t) for t in kgr.blocks_of(s)]
        blocks[0] = blocks[0] + 0.01 * b * np.eye(S)
        for i in (4, 5, 6):
            blocks[i] = blocks[i] * (1 + 0.1 * b)
        return dict(zip(T.BLOCKS, blocks)), s.rho
    return dict(zip(T.BLOCKS, synth.make_blocks(S, C, K, seed=70 + b, dense_q=True))), 1e-3


@pytest.mark.parametrize("shape", KKT_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_kkt_solve_forward_ad_against_the_dense_reference(shape):
    """A dual input through kkt_solve yields a tangent (without the feature this raises), every input dual, R = 1; and
    kkt_solve_tangents with R = 1 of the same direction gives the same bits."""
    math, rho = kkt_system(*shape)
    dots = T.random_math_tangents(math, 11)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(dev(math[n]), dev(dots[n])) for n in T.BLOCKS]
        lam, dz = gpa().kkt_solve(*duals, rho=rho, **TIGHT)
        (lam_p, lam_t), (dz_p, dz_t) = fwAD.unpack_dual(lam), fwAD.unpack_dual(dz)
        assert lam_t is not None and dz_t is not None
        lam_t, dz_t, lam_p, dz_p = lam_t.clone(), dz_t.clone(), lam_p.clone(), dz_p.clone()
    x, lm, x_dot, lam_dot = T.reference_tangents(math, rho, **dots)
    close(npy(dz_p), x, "dz")
    close(npy(lam_p), lm, "lam")
    close(npy(dz_t), x_dot, "dz.")
    close(npy(lam_t), lam_dot, "lam.")
    lam2, dz2, lam_d, dz_d = gpa().kkt_solve_tangents(*(dev(math[n]) for n in T.BLOCKS), {n: dev(dots[n][None]) for n in T.BLOCKS},
                                                    rho=rho, **TIGHT)
    assert lam_d.shape == (1,) + lam_t.shape and dz_d.shape == (1,) + dz_t.shape
    assert torch.equal(lam2, lam_p) and torch.equal(dz2, dz_p) and torch.equal(lam_d[0], lam_t) and torch.equal(dz_d[0], dz_t)
    # one dual input alone: the others arrive as None
    with fwAD.dual_level():
        ts = [dev(math[n]) for n in T.BLOCKS]
        ts[6] = fwAD.make_dual(ts[6], dev(dots["c"]))
        lam, dz = gpa().kkt_solve(*ts, rho=rho, **TIGHT)
        dz_c = npy(fwAD.unpack_dual(dz).tangent)
    close(dz_c, T.reference_tangents(math, rho, c=dots["c"])[2], "dz. of c alone")


@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("shape", KKT_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_kkt_solve_tangents_against_the_dense_reference(shape, Bn):
    """R = 3 directions, unbatched (Bn = 1) and a batch of three systems; a subset of the names: the others are zero."""
    R = 3
    per = [kkt_system(*shape, b) for b in range(Bn)]
    rho = per[0][1]
    names = ("Q", "A", "B", "r", "c")
    dots = [[T.random_math_tangents(m, 100 * b + rr, names) for rr in range(R)] for b, (m, _) in enumerate(per)]
    stack = lambda f: np.stack([f(b) for b in range(Bn)]) if Bn > 1 else f(0)
    ins = [dev(stack(lambda b: per[b][0][n])) for n in T.BLOCKS]
    tan = {n: dev(stack(lambda b: np.stack([dots[b][rr][n] for rr in range(R)]))) for n in names}
    lam, dz, lam_d, dz_d = gpa().kkt_solve_tangents(*ins, tan, rho=rho, **TIGHT)
    N, sk = dz.shape[-1], lam.shape[-1]
    assert lam_d.shape == lam.shape[:-1] + (R, sk) and dz_d.shape == dz.shape[:-1] + (R, N) and dz_d.grad_fn is None
    for b in range(Bn):
        for rr in range(R):
            x, lm, x_dot, lam_dot = T.reference_tangents(per[b][0], rho, **dots[b][rr])
            pick = (lambda t: npy(t[b, rr])) if Bn > 1 else (lambda t: npy(t[rr]))
            close(pick(dz_d), x_dot, "dz. system %d direction %d" % (b, rr))
            close(pick(lam_d), lam_dot, "lam. system %d direction %d" % (b, rr))
    with pytest.raises(ValueError, match="share one R"):
        gpa().kkt_solve_tangents(*ins, dict(tan, q=tan["c"][..., :2, :, :]), rho=rho, **TIGHT)
    with pytest.raises(ValueError, match="names"):
        gpa().kkt_solve_tangents(*ins, dict(x_lo=tan["c"]), rho=rho, **TIGHT)


def test_a_zero_direction_among_nonzero_ones_is_exactly_zero():
    """The 0/0 rule per (system, direction): direction 1 of system 0 and every direction of system 2 are zero tangents; they come
    back as exact zeros, the others as the reference's."""
    S, C, K, R = 6, 3, 3, 3
    per = [kkt_system(S, C, K, b) for b in range(3)]
    dots = [[T.random_math_tangents(m, 7 * b + rr, ("q", "c", "A")) for rr in range(R)] for b, (m, _) in enumerate(per)]
    for b, rr in ((0, 1), (2, 0), (2, 1), (2, 2)):
        dots[b][rr] = {n: 0.0 * v for n, v in dots[b][rr].items()}
    ins = [dev(np.stack([m[n] for m, _ in per])) for n in T.BLOCKS]
    tan = {n: dev(np.stack([np.stack([dots[b][rr][n] for rr in range(R)]) for b in range(3)])) for n in ("q", "c", "A")}
    lam, dz, lam_d, dz_d = gpa().kkt_solve_tangents(*ins, tan, rho=per[0][1], **TIGHT)
    assert torch.isfinite(lam_d).all() and torch.isfinite(dz_d).all()
    for b in range(3):
        for rr in range(R):
            if not any(v.any() for v in dots[b][rr].values()):
                assert not dz_d[b, rr].any() and not lam_d[b, rr].any(), (b, rr)
            else:
                _, _, x_dot, lam_dot = T.reference_tangents(per[b][0], per[b][1], **dots[b][rr])
                close(npy(dz_d[b, rr]), x_dot, "dz. system %d direction %d" % (b, rr))
                close(npy(lam_d[b, rr]), lam_dot, "lam. system %d direction %d" % (b, rr))


def test_kkt_solve_tangents_fp32_beside_the_fp32_oracle():
    """14/7/9 by check_f32 (err_gpu <= 2 err_oracle32 + 5e-6): truth = the dense fp64 reference on the fp32-rounded inputs; the
    oracle side = the formulas on oracle.linsys_solve(float32), for the forward and for the tangent right-hand side."""
    S, C, K = 14, 7, 9
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    math = {n: f32(v) for n, v in kkt_system(S, C, K)[0].items()}
    rho = float(np.float32(1e-3))
    dots = {n: f32(v) for n, v in T.random_math_tangents(math, 13).items()}
    tol, mi = tol_mi(np.float32)
    lam, dz, lam_d, dz_d = gpa().kkt_solve_tangents(*(dev(math[n], torch.float32) for n in T.BLOCKS),
                                                  {n: dev(dots[n][None], torch.float32) for n in T.BLOCKS}, rho=rho, exit_tol=tol,
                                                  max_iters=mi)
    _, _, x_dot, lam_dot = T.reference_tangents(math, rho, **dots)
    s = synth.blocks_to_csr(*(math[n] for n in T.BLOCKS), rho=rho, dense_q=True)
    lam_o, dz_o, _ = o.linsys_solve(*s.csr_args(), S, C, K, tol, mi, s.rho, dtype=np.float32)
    H, Cm, _, _ = P.dense_from_blocks(*(math[n] for n in T.BLOCKS), 0.0)
    t_g, t_c, _, _ = T.tangent_rhs(H, Cm, np.asarray(dz_o, np.float64), np.asarray(lam_o, np.float64), **T.dots_from_math(S, C, K, **dots))
    lamd_o, dzd_o, _ = o.linsys_solve(s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, t_g.astype(np.float32),
                                      t_c.astype(np.float32), S, C, K, tol, mi, s.rho, dtype=np.float32)
    check_f32("kkt tangent dz. 14/7/9", npy(dz_d[0]), dzd_o, x_dot)
    check_f32("kkt tangent lam. 14/7/9", npy(lam_d[0]), lamd_o, lam_dot)


def test_a_tangent_after_another_solve_raises():
    """The jvp runs straight after its forward, so the check cannot fire there; Solver.tangents re-solves the CURRENT assembly,
    and _fresh refuses a generation that is not the forward's."""
    from gato_python_amd import autograd
    math, rho = kkt_system(6, 3, 3)
    gpa().kkt_solve(*(dev(math[n]) for n in T.BLOCKS), rho=rho, **TIGHT)
    sol = autograd._SOLVERS[(6, 3, 3, 1, torch.float64, 0)]
    gen = sol.get_option("assembly_gen")
    autograd._fresh(sol, gen, "kkt_solve")
    with pytest.raises(RuntimeError, match="replaced"):
        autograd._fresh(sol, gen - 1, "kkt_solve")


# ---- 3. the pairing with the existing backward pass ----------------------------------------------------------------------------------
def pairing(call, math, seed):
    """|<v, J u> - <J^T v, u>| <= 1e-6 (|v|_1 max(1, |J u|_inf) + |u|_1 max(1, |J^T v|_inf)) for random u (Q, R symmetric) and v:
    what a forward tangent within 1e-6 max(1, |J u|) and a gradient within 1e-6 max(1, |J^T v|) imply."""
    names = list(math)
    u = T.random_math_tangents(math, seed)
    with fwAD.dual_level():
        outs = call(*(fwAD.make_dual(dev(math[n]), dev(u[n])) for n in names))
        Ju = [npy(fwAD.unpack_dual(t).tangent) for t in outs]
    rng = np.random.default_rng(seed + 1)
    v = [rng.standard_normal(t.shape) for t in Ju]
    ts = [dev(math[n]).requires_grad_() for n in names]
    outs = call(*ts)
    sum((t * dev(vi)).sum() for t, vi in zip(outs, v)).backward()
    JTv = [npy(t.grad) for t in ts]
    lhs = sum(float((a * b).sum()) for a, b in zip(v, Ju))
    rhs = sum(float((a * u[n]).sum()) for a, n in zip(JTv, names))
    l1 = lambda xs: sum(float(np.abs(x).sum()) for x in xs)
    linf = lambda xs: max(float(np.abs(x).max()) for x in xs)
    bar = 1e-6 * (l1(v) * max(1.0, linf(Ju)) + l1(list(u.values())) * max(1.0, linf(JTv)))
    print("<v, J u>", lhs, "<J^T v, u>", rhs, "difference", abs(lhs - rhs), "bar", bar)
    assert np.isfinite(lhs) and abs(lhs) > 0 and abs(lhs - rhs) <= bar


@pytest.mark.parametrize("shape", KKT_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_pairing_kkt_solve(shape):
    math, rho = kkt_system(*shape)
    pairing(lambda *t: gpa().kkt_solve(*t, rho=rho, **TIGHT), math, 21)


def layer_call(p, **more):
    keys = list(T.math_of(p))
    extra = keys[11:]

    def call(*t):
        x, lam, info = gpa().box_qp_layer(*t[:11], rho=p["s"].rho, method="pdas", **dict(zip(extra, t[11:])), **TIGHT, **more)
        assert int(info.polished) == _lib.POLISH_ACCEPTED and np.array_equal(info.act.cpu().numpy(), T.act_of(p))
        return x, lam
    return call


@pytest.mark.parametrize("case", T.LAYER_CASES)
def test_pairing_layer(case):
    """Hard bounds (constructed 6/3/9), soft and mixed (mixed_box 6/3/9 and 14/7/3), capped with a saturated variable (huber)."""
    p = T.layer_problem(case)
    hard, soft, sat = T.sets(T.act_of(p), p.get("w"))
    assert hard.any() and (soft.any() or "w" not in p) and (sat.any() or "m" not in p)
    pairing(layer_call(p), T.math_of(p), 31)


# ---- 4. the layer end to end ---------------------------------------------------------------------------------------------------------
def layer_tangents(p, dots, R, **more):
    """box_qp_layer_tangents on problem p with the per-direction math-shaped tangents dots[rr] -> (x, lam, info, x_dot, lam_dot)."""
    math = T.math_of(p)
    keys = list(math)
    tan = {n: dev(np.stack([dots[rr][n] for rr in range(R)])) for n in dots[0]}
    soft = {n: dev(math[n]) for n in keys[11:]}
    return gpa().box_qp_layer_tangents(*(dev(math[n]) for n in keys[:11]), tan, rho=p["s"].rho, method="pdas", **soft, **TIGHT, **more)


@pytest.mark.parametrize("case", T.FD_CASES)
def test_layer_tangents_against_the_reference(case):
    """The three forms of the bounds, R = 3 directions over every input, unbatched; and forward_ad (R = 1) gives direction 0."""
    p = T.layer_problem(case)
    math, act, R = T.math_of(p), T.act_of(p), 3
    dots = [T.random_math_tangents(math, 40 + rr) for rr in range(R)]
    x, lam, info, x_d, lam_d = layer_tangents(p, dots, R)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and np.array_equal(info.act.cpu().numpy(), act)
    assert x_d.shape == (R, p["s"].N) and lam_d.shape == (R, p["s"].S * p["s"].K) and x_d.grad_fn is None
    for rr in range(R):
        xr, lr, x_dot, lam_dot = T.reference_tangents(math, p["s"].rho, act, **dots[rr])
        close(npy(x), xr, "x")
        close(npy(x_d[rr]), x_dot, "x. direction %d" % rr)
        close(npy(lam_d[rr]), lam_dot, "lam. direction %d" % rr)
    hard = T.sets(act, p.get("w"))[0]
    d0 = T.dots_from_math(p["s"].S, p["s"].C, p["s"].K, **dots[0])
    assert np.array_equal(npy(x_d[0])[hard], T.b_dot_of(act, d0["lo_dot"], d0["hi_dot"])[hard])       # b. itself, bit for bit
    with fwAD.dual_level():
        xx, ll = layer_call(p)(*(fwAD.make_dual(dev(math[n]), dev(dots[0][n])) for n in math))
        xt, lt = npy(fwAD.unpack_dual(xx).tangent), npy(fwAD.unpack_dual(ll).tangent)
    _, _, x_dot, lam_dot = T.reference_tangents(math, p["s"].rho, act, **dots[0])
    close(xt, x_dot, "x. by forward_ad")
    close(lt, lam_dot, "lam. by forward_ad")


def test_layer_batch_with_a_system_that_does_not_converge():
    """Three double integrators, the middle one's second reduced system singular: zero tangents on it give zeros, the good
    systems' tangents are the reference's; a nonzero tangent on it raises RuntimeError."""
    ps = D.di_trio()
    R = 2
    maths = [T.math_of(p) for p in ps]
    keys = list(maths[0])
    dots = [[T.random_math_tangents(m, 60 + 10 * b + rr) for rr in range(R)] for b, m in enumerate(maths)]
    for rr in range(R):
        dots[1][rr] = {n: 0.0 * v for n, v in dots[1][rr].items()}
    ins = [dev(np.stack([m[n] for m in maths])) for n in keys]
    tan = {n: dev(np.stack([np.stack([dots[b][rr][n] for rr in range(R)]) for b in range(3)])) for n in keys}
    x, lam, info, x_d, lam_d = gpa().box_qp_layer_tangents(*ins, tan, rho=ps[0]["s"].rho, method="pdas", **TIGHT)
    print("status", info.status.tolist())
    assert int(info.polished[1]) != _lib.POLISH_ACCEPTED and int(info.polished[0]) == int(info.polished[2]) == _lib.POLISH_ACCEPTED
    assert not x_d[1].any() and not lam_d[1].any() and torch.isfinite(x_d).all() and torch.isfinite(lam_d).all()
    for b in (0, 2):
        for rr in range(R):
            _, _, x_dot, lam_dot = T.reference_tangents(maths[b], ps[b]["s"].rho, T.act_of(ps[b]), **dots[b][rr])
            close(npy(x_d[b, rr]), x_dot, "x. system %d direction %d" % (b, rr))
            close(npy(lam_d[b, rr]), lam_dot, "lam. system %d direction %d" % (b, rr))
    tan["q"][1, 0, 0, 0] = 1.0
    with pytest.raises(RuntimeError, match=r"systems \[1\]"):
        gpa().box_qp_layer_tangents(*ins, tan, rho=ps[0]["s"].rho, method="pdas", **TIGHT)


def test_layer_tangents_given_as_numbers_broadcast_like_the_bounds():
    """u_hi. = 1 and u_lo. = a [C] vector against the full-shaped tangents."""
    p = T.layer_problem("constructed 6/3/9")
    math, s = T.math_of(p), p["s"]
    keys, R = list(math), 2
    rng = np.random.default_rng(3)
    vec = rng.standard_normal(s.C)
    full = [dict(q=rng.standard_normal(math["q"].shape), u_hi=np.ones(math["u_hi"].shape), u_lo=np.broadcast_to(vec, math["u_lo"].shape))
            for _ in range(R)]
    tan = dict(q=dev(np.stack([f["q"] for f in full])), u_hi=1.0, u_lo=dev(vec))
    x, lam, info, x_d, lam_d = gpa().box_qp_layer_tangents(*(dev(math[n]) for n in keys), tan, rho=s.rho, method="pdas", **TIGHT)
    for rr in range(R):
        _, _, x_dot, lam_dot = T.reference_tangents(math, s.rho, T.act_of(p), **full[rr])
        close(npy(x_d[rr]), x_dot, "x. direction %d" % rr)
        close(npy(lam_d[rr]), lam_dot, "lam. direction %d" % rr)


def test_layer_tangents_admm():
    """method="admm" (ADMM, the active set, the polish) on pendulum_box(0.2): the tangents of the polish's act."""
    s, lo, hi, arho = P.problem("pendulum")
    act = P.exact_active("pendulum")[0]
    assert (act != 0).any()
    math = dict(zip(D.KEYS, D.math_arrays(s, lo, hi)))
    R = 2
    dots = [T.random_math_tangents(math, 80 + rr) for rr in range(R)]
    tan = {n: dev(np.stack([d[n] for d in dots])) for n in math}
    x, lam, info, x_d, lam_d = gpa().box_qp_layer_tangents(*(dev(math[n]) for n in math), tan, rho=s.rho, admm_rho=arho, **TIGHT)
    assert int(info.polished) == _lib.POLISH_ACCEPTED
    for rr in range(R):
        _, _, x_dot, lam_dot = T.reference_tangents(math, s.rho, act, **dots[rr])
        close(npy(x_d[rr]), x_dot, "x. direction %d" % rr)
        close(npy(lam_d[rr]), lam_dot, "lam. direction %d" % rr)


def test_layer_tangents_with_the_line_search():
    """line_search=True on an all-soft capped case the undamped iteration cycles on: the tangents of the same final act."""
    p = L.ls_box(6, 3, 9, L.CAPPED)[0]
    math, act = T.math_of(p), T.act_of(p)
    dots = [T.random_math_tangents(math, 90)]
    x, lam, info, x_d, lam_d = layer_tangents(p, dots, 1, line_search=True)
    assert int(info.polished) == _lib.POLISH_ACCEPTED and np.array_equal(info.act.cpu().numpy(), act)
    _, _, x_dot, lam_dot = T.reference_tangents(math, p["s"].rho, act, **dots[0])
    close(npy(x_d[0]), x_dot, "x.")
    close(npy(lam_d[0]), lam_dot, "lam.")
