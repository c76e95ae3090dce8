"""The box-QP, polish and bound-gradient kernels (gato_qp.hip, gato_polish.hip) at every compiled shape and at the knot edges:
active states through the masked inversion, K = 2 and 3 (every knot a first or a last one), K past the 8192-workgroup cap of
the grid (a second pass of every knot loop), the order of the active-set rule, and the bound gradients as a function of
their six arrays.  Every case is named and deterministic; the problems with active states come from
box_qp_polish_ref.constructed_problem, whose conditions tests/test_box_qp_polish_cpu.py checks on the CPU.
Bars: those of tests/test_gpu_box_qp.py and tests/test_gpu_box_qp_polish.py (fp64 iterates 1e-8, polished points 1e-6 and
qp_kkt_residuals <= 1e-7, fp32 by tests/f32_parity.py); long horizons 1e-6 relative (README: the fp64 parity bar)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_polish_ref as P                     # noqa: E402
import box_qp_ref as ref                          # noqa: E402
from f32_parity import check_f32                  # noqa: E402
from gato_python_amd import _lib, synth           # noqa: E402
from box_qp_device import (CAP, PARITY, admm, admm_host, admm_run, bits, check_polished, dev_inputs, g_and_c, host, polish,   # noqa: E402
                           rel, solver)

SHAPES = P.SWEEP_SHAPES
SHORT_K = P.SWEEP_SHORT_K
LONG = P.SWEEP_LONG


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()


def parts_of(p):
    return (None, p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"])


def active_states(p):
    n = p["s"].S + p["s"].C
    return int(((p["act"] != 0) & (np.arange(len(p["act"])) % n < p["s"].S)).sum())


# ---- a. polish on a constructed active set (active states at every shape) -----------------------------------------------
POLISH_CASES = [(S, C, K, np.float64) for S, C in SHAPES for K in SHORT_K] + [(S, C, K, np.float32) for S, C, K in P.SWEEP_F32]


@pytest.mark.parametrize("S,C,K,dt", POLISH_CASES, ids=["%d-%d-%d-%s" % (S, C, K, np.dtype(dt).name) for S, C, K, dt in POLISH_CASES])
def test_polish_constructed_active_set(S, C, K, dt):
    """fp64: ACCEPTED and check_polished (1e-6 parity, qp_kkt_residuals <= 1e-7, x_A the bounds bit for bit).  fp32: the
    inputs rounded to fp32; the truth the fp64 dense reduced solve on them, the oracle the reduced stage path restated in
    fp32 (box_qp_polish_ref.reduced_stage_solve); err_gpu <= 2 err_oracle + 5e-6."""
    f64 = dt == np.float64
    p = P.constructed(S, C, K)[0] if f64 else P.rounded(P.constructed(S, C, K, extra=P.f32_ok, tag="f32")[0])
    s, act, lo, hi = p["s"], p["act"], p["lo"], p["hi"]
    print("seed", p["seed"], "cond", p["figures"]["cond"], "active", int((act != 0).sum()), "states", active_states(p))
    if K >= 3:
        assert active_states(p) >= 1
    sol = solver(S, C, K, dt)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, max_admm_iters=1)
    if f64:
        codes = polish(sol, inp, act, r, s.rho)
        assert codes.tolist() == [_lib.POLISH_ACCEPTED]
        check_polished(sol, r, 0, parts_of(p), act)
        return
    x_o, lam_o, its = P.reduced_stage_solve(s, lo, hi, act, np.float32, exit_tol=1e-8, max_iters=1000)
    codes = polish(sol, inp, act, r, s.rho, eps=P.F32_EPS, exit_tol=1e-8, max_iters=1000)
    x, lam = r.x.cpu().numpy(), r.lam.cpu().numpy()
    print("oracle pcg iterations", its, "codes", codes.tolist())
    assert codes.tolist() == [_lib.POLISH_ACCEPTED]
    on = act != 0
    assert np.array_equal(x[on], P.bound_values(act, lo, hi)[on].astype(np.float32))
    check_f32("polish x %d/%d/%d constructed" % (S, C, K), x, x_o, p["x"])
    check_f32("polish lam %d/%d/%d constructed" % (S, C, K), lam, lam_o, p["lam"])


# ---- b. one wrong sign: rejected, nothing written -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_polish_wrong_sign_is_rejected(shape):
    S, C = shape
    K = 9
    p = P.constructed(S, C, K)[0]
    s = p["s"]
    flipped, j = P.wrong_sign(p)
    zero = np.zeros(s.N)
    want = P.polish(p["H"], p["Cm"], p["g"], p["c"], p["lo"], p["hi"], zero, zero, S, act=flipped)
    assert want["decision"] == P.REJECTED
    sol = solver(S, C, K, np.float64)
    inp = dev_inputs(sol, [s], [(p["lo"], p["hi"])])
    r = admm(sol, inp, s.rho, max_admm_iters=1)
    before = bits(r)
    codes = polish(sol, inp, flipped, r, s.rho)
    assert codes.tolist() == [_lib.POLISH_REJECTED]
    assert bits(r) == before


# ---- c. the active-set rule at its edges ------------------------------------------------------------------------------------
#            lo       hi       z      y       act      what
PATTERNS = [(-1.0,    1.0,     0.9,   0.5,    1),    # upper only
            (-1.0,    1.0,    -0.9,  -0.5,   -1),    # lower only
            (1.0,    -1.0,     0.0,   0.0,   -1),    # both inequalities hold (only a crossed box can): lower wins
            (-1.0,    1.0,     0.5,   0.5,    0),    # tie hi - z == y: free
            (-1.0,    1.0,    -0.5,  -0.5,    0),    # tie z - lo == -y: free
            (0.25,    0.25,    0.25,  2.0,   -1),    # lo == hi, y > 0 (the upper test alone says +1)
            (0.25,    0.25,    0.25, -2.0,   -1),    # lo == hi, y < 0
            (-1.0,    np.inf,  3.0,   1e6,    0),    # hi = +inf, large positive y: never active
            (-np.inf, 1.0,    -3.0,  -1e6,    0),    # lo = -inf, large negative y
            (-1.0,    1.0,     1e-8,  1.0,    None)] # hi - z rounds to 1 in fp32 (free), is below 1 in fp64 (upper)


def pattern_arrays(which, dt):
    t = np.array([row[:4] for row in PATTERNS], np.float64)[which]
    want = np.array([(1 if dt == np.float64 else 0) if row[4] is None else row[4] for row in PATTERNS], np.int8)[which]
    lo, hi, z, y = (np.ascontiguousarray(t[..., i]).astype(dt) for i in range(4))
    return lo, hi, z, y, want


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_active_set_rule_edges(shape, dt):
    """Hand-made (z, y, lo, hi), K = 3, three systems: over the len(PATTERNS) rotations every variable of every knot - the
    S-only last knot included - meets every pattern.  Every value is exact in fp32."""
    S, C = shape
    K, B = 3, 3
    sol = solver(S, C, K, dt, batch=B)
    N, n = sol.N, S + C
    flat = np.arange(B * N).reshape(B, N)
    seen_x0_active = False
    for rot in range(len(PATTERNS)):
        which = (flat + rot + np.arange(B)[:, None]) % len(PATTERNS)
        lo, hi, z, y, table = pattern_arrays(which, dt)
        want = P.active_set(z, y, lo, hi, S)                     # on arrays of the solver's dtype: fp32 compares in fp32
        assert want.dtype == np.int8 and np.array_equal(want[:, S:], table[:, S:]) and not want[:, :S].any()
        seen_x0_active |= bool(table[:, :S].any())
        d = lambda a: sol.to_device(a.reshape(-1))
        got = sol.box_qp_active_set(d(z), d(y), d(lo), d(hi))
        torch.cuda.synchronize()
        got = got.cpu().numpy().reshape(B, N)
        assert got.dtype == np.int8 and np.array_equal(got, want), (rot, np.argwhere(got != want)[:5])
    assert seen_x0_active                                        # x_0 carried patterns that are active anywhere else


def test_active_set_rule_long_horizon():
    """2/1/8197: random patterns and random continuous points; the whole vector, and the knots of the second grid pass."""
    S, C, K = LONG
    sol = solver(S, C, K, np.float64)
    N, n = sol.N, S + C
    rng = np.random.default_rng(5)
    lo, hi, z, y, _ = pattern_arrays(rng.integers(0, len(PATTERNS), N), np.float64)
    cont = rng.random(N) < 0.5                                   # half the variables: a continuous point near a box
    lo[cont], hi[cont] = -rng.uniform(0.5, 1.5, cont.sum()), rng.uniform(0.5, 1.5, cont.sum())
    z[cont], y[cont] = rng.uniform(-1.6, 1.6, cont.sum()), 0.3 * rng.standard_normal(cont.sum())
    want = P.active_set(z, y, lo, hi, S)
    got = sol.box_qp_active_set(*(sol.to_device(a) for a in (z, y, lo, hi)))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert (want == 1).sum() > N // 10 and (want == -1).sum() > N // 10 and (want == 0).sum() > N // 10
    assert np.array_equal(got, want)
    assert N - CAP * n == (K - CAP) * n - C and np.array_equal(got[CAP * n:], want[CAP * n:]) and want[CAP * n:].any()


# ---- d. the bound gradients as a function of their six arrays ------------------------------------------------------------
def bound_grad_case(S, C, K, B, dt, sparse=False):
    """Per system: a dense-block system, a legal random act (0 on x_0), random xbar and beta, a random a with a_A = 0 (the
    kernel's contract); everything rounded to dt.  -> (systems, act, xbar, a, beta [B, .] in fp64)."""
    rng = np.random.default_rng([S, C, K, 17])
    systems = [P.constructed_system(S, C, K, 30 + b).astype(dt).astype(np.float64) for b in range(B)]
    N, sk = systems[0].N, S * K
    act = rng.integers(-1, 2, (B, N)).astype(np.int8)
    act[:, :S] = 0
    act[:, S], act[:, N - 1] = 1, -1                # the first control and the last state of the last knot: always active
    r = lambda *shape: rng.standard_normal(shape).astype(dt).astype(np.float64)
    xbar, beta = r(B, N), r(B, sk)
    a = np.where(act != 0, 0.0, r(B, N))
    return systems, act, xbar, a, beta


def run_bound_grad(sol, systems, act, xbar, a, beta):
    inf = np.full(systems[0].N, np.inf)
    inp = dev_inputs(sol, systems, [(-inf, inf)] * len(systems))
    d = lambda v, dt=None: sol.to_device(v.reshape(-1), dt)
    lo_bar, hi_bar = sol.box_qp_bound_grad(inp[0], inp[1], d(act, np.int8), d(xbar), d(a), d(beta))
    torch.cuda.synchronize()
    B = len(systems)
    return host(lo_bar, B, sol.N), host(hi_bar, B, sol.N)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("K", [2, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "%d-%d" % sh)
def test_bound_grad_direct(shape, K, dt):
    """fp64: 1e-12 of max(1, |want|) - a handful of fmas per entry.  fp32: against the fp64 formula on the fp32-rounded
    inputs, held to twice the error of the same formula evaluated in numpy fp32 plus 5e-6 relative (check_f32's constants)."""
    S, C = shape
    B = 2
    systems, act, xbar, a, beta = bound_grad_case(S, C, K, B, dt)
    sol = solver(S, C, K, dt, batch=B)
    lo_bar, hi_bar = run_bound_grad(sol, systems, act, xbar, a, beta)
    assert not lo_bar[act >= 0].any() and not hi_bar[act <= 0].any()
    for b, s in enumerate(systems):
        H, Cm = (m.toarray() for m in g_and_c(s))
        want = P.bound_grads(H, Cm, act[b], xbar[b], a[b], beta[b])
        assert want[0].any() and want[1].any()
        for name, got, w in (("lo_bar", lo_bar[b], want[0]), ("hi_bar", hi_bar[b], want[1])):
            if dt == np.float64:
                err = np.abs(got - w).max()
                assert err <= 1e-12 * max(1.0, np.abs(w).max()), (b, name, err)
            else:
                f = lambda v: np.asarray(v, np.float32)
                o32 = np.where(act[b] != 0, f(xbar[b]) - (f(H) @ f(a[b]) + f(Cm).T @ f(beta[b])), np.float32(0))
                o32 = np.where(act[b] < 0 if name == "lo_bar" else act[b] > 0, o32, np.float32(0))
                assert o32.dtype == np.float32
                check_f32("bound grad %s %d/%d/%d system %d" % (name, S, C, K, b), got, o32, w)


def test_bound_grad_long_horizon():
    S, C, K = LONG
    n = S + C
    systems, act, xbar, a, beta = bound_grad_case(S, C, K, 1, np.float64)
    sol = solver(S, C, K, np.float64)
    lo_bar, hi_bar = run_bound_grad(sol, systems, act, xbar, a, beta)
    assert not lo_bar[act >= 0].any() and not hi_bar[act <= 0].any()
    s = systems[0]
    want = P.bound_grads(*g_and_c(s), act[0], xbar[0], a[0], beta[0])
    for got, w in ((lo_bar[0], want[0]), (hi_bar[0], want[1])):
        assert np.abs(got - w).max() <= 1e-12 * max(1.0, np.abs(w).max())
        tail = slice(CAP * n, None)
        assert w[tail].any() and np.abs(got[tail] - w[tail]).max() <= 1e-12 * max(1.0, np.abs(w[tail]).max())


# ---- e. ADMM iterates at the shapes and the short horizons test_iterates_match_reference leaves out -----------------------
ADMM_CASES = [((6, 3), 9), ((12, 6), 9), ((32, 16), 9)] + [(sh, K) for sh in SHAPES for K in (2, 3)]


@pytest.mark.parametrize("shape,K", ADMM_CASES, ids=["%d-%d-%d" % (sh + (K,)) for sh, K in ADMM_CASES])
def test_admm_iterates_every_shape(shape, K):
    """K = 2, 3: every knot is a first or a last one.  P.boxes() fixes a control of knot K // 2, which K = 2 does not have:
    there the box comes without the lo == hi control."""
    S, C = shape
    s = synth.make_system(S, C, K, seed=2)
    lo, hi = P.boxes(s, 3, eq=K > 2)
    sol = solver(S, C, K, np.float64)
    r = admm_run(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, **PARITY)
    got = admm_host(r, 0, sol)
    H, Cm, g, c = ref.parts(s)
    want = ref.admm(H, Cm, g, c, lo, hi, eps_abs=0.0, eps_rel=0.0, max_admm_iters=25)
    assert got["status"] == want["status"] == ref.MAX_ITERS and got["iters"] == want["iters"] == 25
    assert np.any(want["y"] != 0)
    rels = {k: rel(got[k], want[k]) for k in ("x", "z", "y", "lam")}
    print(shape, K, rels)
    for k, v in rels.items():
        assert v <= 1e-8, (k, v)


# ---- f. K past the grid cap: the second pass of every knot loop -----------------------------------------------------------
def tail_of(v, S, C, per_knot):
    """The entries of knots >= CAP of a dz-layout (per_knot = S + C) or a lambda-layout (per_knot = S) vector."""
    return np.asarray(v)[CAP * per_knot:]


def long_horizon_admm(S, C, K):
    """Ten ADMM iterations against the sparse reference, whole vectors and the knots >= 8192 alone: 1e-6 relative, the
    project's fp64 parity bar (the sparse reference's own residual at this size is 6e-15; a knot skipped or read from a
    stale LDS block errs at order 1)."""
    s = synth.make_system(S, C, K, seed=2)
    H, Cm, g, c = ref.sparse_parts(s)
    dz = ref.kkt_solver(H, Cm)(np.concatenate([g, c]))[:s.N]
    lo, hi = P.boxes(s, 3, dz=dz)
    want = ref.admm(H, Cm, g, c, lo, hi, eps_abs=0.0, eps_rel=0.0, max_admm_iters=10)
    sol = solver(S, C, K, np.float64)
    r = admm(sol, dev_inputs(sol, [s], [(lo, hi)]), s.rho, eps_abs=0.0, eps_rel=0.0, max_admm_iters=10)
    got = admm_host(r, 0, sol)
    print("pcg iterations of the x-steps", sol.box_qp_pcg_iters().tolist())
    assert got["status"] == want["status"] == ref.MAX_ITERS and got["iters"] == want["iters"] == 10
    n = S + C
    assert np.any(tail_of(want["y"], S, C, n) != 0)
    for k in ("x", "z", "y", "lam"):
        per = S if k == "lam" else n
        whole, tail = rel(got[k], want[k]), rel(tail_of(got[k], S, C, per), tail_of(want[k], S, C, per))
        print("long-K rel", (S, C, K), k, "whole", whole, "knots >= 8192", tail)
        assert whole <= 1e-6 and tail <= 1e-6, (k, whole, tail)


def last_pcg_iters(sol):
    """PCG iterations of the solver's latest whole solve, per system (the solver's own counter, buffer 8)."""
    import ctypes as ct
    out = np.zeros(sol.batch, np.int32)
    torch.cuda.synchronize()
    rc = ct.CDLL("libamdhip64.so").hipMemcpy(out.ctypes.data_as(ct.c_void_p), ct.c_void_p(sol.buffer_ptr(8)),
                                             ct.c_size_t(out.nbytes), 2)
    assert rc == 0
    return out.tolist()


LONG_POLISH_MAX_ITERS = 20000


def long_horizon_polish():
    """The constructed problem through the sparse path (box_qp_polish_ref.LONG_KNOBS).  Its reduced Schur system, 16394
    unknowns with 3800 of the states fixed, takes the PCG 5438 iterations at exit_tol 1e-20 - the oracle's fp64 PCG needs
    the same, and stopped at the other files' max_iters = 1000 both are 1.46 away in x - so this case alone gives the PCG
    20000."""
    S, C, K = LONG
    n = S + C
    p = P.constructed(S, C, K, **P.LONG_KNOBS)[0]
    s, act, lo, hi = p["s"], p["act"], p["lo"], p["hi"]
    on = act != 0
    assert (np.flatnonzero(on) // n >= CAP).any()
    sol = solver(S, C, K, np.float64)
    inp = dev_inputs(sol, [s], [(lo, hi)])
    r = admm(sol, inp, s.rho, max_admm_iters=1)
    codes = polish(sol, inp, act, r, s.rho, max_iters=LONG_POLISH_MAX_ITERS)
    its = last_pcg_iters(sol)
    print("pcg iterations of the reduced solve", its)
    assert its[0] < LONG_POLISH_MAX_ITERS
    assert codes.tolist() == [_lib.POLISH_ACCEPTED]
    x, y, lam = host(r.x, 1, sol.N)[0], host(r.y, 1, sol.N)[0], host(r.lam, 1, sol.sizes["sk"])[0]
    ex, el = np.abs(x - p["x"]).max(), np.abs(lam - p["lam"]).max()
    kk = ref.qp_kkt_residuals(p["H"], p["Cm"], p["g"], p["c"], lo, hi, x, y, lam)
    print("seed", p["seed"], "x err", ex, "of", np.abs(p["x"]).max(), "lam err", el, "of", np.abs(p["lam"]).max(), "kkt", kk)
    assert ex <= 1e-6 * max(1.0, np.abs(p["x"]).max()) and el <= 1e-6 * max(1.0, np.abs(p["lam"]).max())
    for v, w, per in ((x, p["x"], n), (lam, p["lam"], S)):
        assert np.abs(tail_of(v, S, C, per) - tail_of(w, S, C, per)).max() <= 1e-6 * max(1.0, np.abs(tail_of(w, S, C, per)).max())
    assert max(kk.values()) <= 1e-7, kk
    assert np.array_equal(x[on], P.bound_values(act, lo, hi)[on])
    assert int(r.status[0]) == _lib.QP_CONVERGED


@pytest.mark.parametrize("part,shape", [("admm", LONG), ("admm", (4, 2, 8200)), ("polish", LONG)],
                         ids=["admm-2-1-8197", "admm-4-2-8200", "polish-2-1-8197"])
def test_long_horizon_second_grid_pass(part, shape):
    if part == "admm":
        long_horizon_admm(*shape)
    else:
        long_horizon_polish()


# ---- g. a batch of constructed problems ---------------------------------------------------------------------------------------
def test_batch_of_constructed_problems():
    """Five constructed 14/7/9 problems of five seeds, the last with one sign flipped: four accepted and checked, one
    rejected and left bit for bit, in the given order and in a permuted one; permuted systems give permuted bits."""
    S, C, K, B = P.SWEEP_BATCH
    ps = P.constructed(S, C, K, count=B)
    assert len({p["seed"] for p in ps}) == B
    acts = [p["act"] for p in ps[:-1]] + [P.wrong_sign(ps[-1])[0]]
    want = [_lib.POLISH_ACCEPTED] * (B - 1) + [_lib.POLISH_REJECTED]
    outs = []
    for perm in (list(range(B)), [3, 4, 0, 2, 1]):
        sol = solver(S, C, K, np.float64, batch=B)
        inp = dev_inputs(sol, [ps[i]["s"] for i in perm], [(ps[i]["lo"], ps[i]["hi"]) for i in perm])
        r = admm(sol, inp, ps[0]["s"].rho, max_admm_iters=1)
        fields = lambda: [t.cpu().numpy().reshape(B, -1).copy() for t in (r.x, r.z, r.y, r.lam, r.iters, r.status, r.res_prim, r.res_dual)]
        before = fields()
        codes = polish(sol, inp, np.stack([acts[i] for i in perm]), r, ps[0]["s"].rho)
        assert codes.tolist() == [want[i] for i in perm]
        after = fields()
        for j, i in enumerate(perm):
            if want[i] == _lib.POLISH_REJECTED:
                assert all(a[j].tobytes() == b[j].tobytes() for a, b in zip(after, before))
            else:
                check_polished(sol, r, j, parts_of(ps[i]), acts[i])
        outs.append((perm, after))
    (p0, o0), (p1, o1) = outs
    for j, i in enumerate(p1):
        for t0, t1 in zip(o0, o1):
            assert t0[p0.index(i)].tobytes() == t1[j].tobytes()
