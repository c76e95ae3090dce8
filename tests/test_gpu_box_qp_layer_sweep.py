"""box_qp_layer(method="pdas"), with and without soft bounds, where its backward pass branches (gato_python_amd/qp.py,
_BoxQPLayer without and with weights; DESIGN.md sections 3.8 - 3.10): batches whose systems freeze at different solves, assemblies
another call replaced before the backward pass, one system of a batch that does not converge, subsets of the inputs and of the
outputs, and bounds and weights that broadcast.  Every gradient is compared with the numpy references - box_qp_polish_ref.grads
for hard bounds, box_qp_soft_ref.soft_grads for soft ones - on the reference run's final act and the device's x and lam; the bar
is the fp64 layer bar, err < 1e-6 max(1, |want|max) per input.  tests/test_box_qp_layer_cases_cpu.py proves from the reference
alone that every input used here has the property its test needs.  (No fp32 section: the references cast to float64 inside
adjoint(), grads_math() and bound_grads(), so they cannot be evaluated in float32 without being rewritten.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_qp_pdas_ref as D                       # noqa: E402
import box_qp_soft_ref as R                       # noqa: E402
import kkt_grad_ref as kgr                        # noqa: E402
from gato_python_amd import _lib                  # noqa: E402
from box_qp_device import F64                     # noqa: E402

BAR = 1e-6
WORST = {}                                        # section -> (largest err, its bar, input): printed when the module ends


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()
    yield
    for sec in sorted(WORST):
        print("layer sweep section %s: largest err %.3e (bar %.3e, %s)" % ((sec,) + WORST[sec]))


def ag():
    from gato_python_amd import autograd
    return autograd


def npy(t):
    return t.detach().cpu().numpy()


def dev(a, requires_grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda().requires_grad_(requires_grad)


def scalar(v):
    """A 0-d fp64 device tensor that requires a gradient."""
    return torch.tensor(float(v), dtype=torch.float64, device="cuda", requires_grad=True)


def keys_of(soft):
    return R.SOFT_KEYS if soft else D.KEYS


def tensors(ps, soft, batched, requires_grad=True):
    """The layer's inputs of the problems (one problem unbatched, or all stacked), in keys_of(soft)'s order; requires_grad: a
    bool or the names that get it."""
    arrs = [R.soft_math_arrays(p) if soft else D.math_arrays(p["s"], p["lo"], p["hi"]) for p in ps]
    arrs = D.batched(arrs) if batched else arrs[0]
    want = (lambda k: requires_grad) if isinstance(requires_grad, bool) else (lambda k: k in requires_grad)
    return [dev(a, want(k)) for k, a in zip(keys_of(soft), arrs)]


def layer(ts, soft, rho, **kw):
    import gato_python_amd
    if soft:
        return gato_python_amd.box_qp_layer(*ts[:11], rho=rho, method="pdas", x_soft=ts[11], u_soft=ts[12], **F64, **kw)
    return gato_python_amd.box_qp_layer(*ts[:11], rho=rho, method="pdas", **F64, **kw)


def solver_of(ps, batch):
    """The cached Solver every call of the problems' shape, batch and fp64 shares."""
    s = ps[0]["s"]
    return ag()._SOLVERS[(s.S, s.C, s.K, batch, torch.float64, torch.cuda.current_device())]


def upstream(seed, x, lam):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(tuple(x.shape)), rng.standard_normal(tuple(lam.shape))


def loss_of(x, lam, xbar, lbar):
    return (x * dev(xbar)).sum() + (lam * dev(lbar)).sum()


def note(section, err, bar, what):
    if section not in WORST or err / bar > WORST[section][0] / WORST[section][1]:
        WORST[section] = (float(err), float(bar), what)


def check_forward(ps, info, systems=None):
    """iters, act and the ACCEPTED code of the systems against their reference runs."""
    B = len(ps)
    iters, codes, act = npy(info.iters).reshape(B), npy(info.polished).reshape(B), npy(info.act).reshape(B, -1)
    for b in range(B) if systems is None else systems:
        run = ps[b]["run"]
        assert int(codes[b]) == _lib.POLISH_ACCEPTED and int(iters[b]) == run["iters"], (b, int(codes[b]), int(iters[b]), run["iters"])
        assert np.array_equal(act[b], run["act"]), (b, np.flatnonzero(act[b] != run["act"])[:5])


def check_grads(section, ps, soft, ts, x, lam, xbar, lbar, systems=None, factor=1.0):
    """t.grad / factor of every input against the reference of each system, at the bar."""
    B = len(ps)
    batched = x.dim() == 2
    xs, ls = npy(x).reshape(B, -1), npy(lam).reshape(B, -1)
    xb, lb = np.asarray(xbar, np.float64).reshape(B, -1), np.asarray(lbar, np.float64).reshape(B, -1)
    for b in range(B) if systems is None else systems:
        want = R.reference_grads(ps[b], xs[b], ls[b], xb[b], lb[b])
        for k, t in zip(keys_of(soft), ts):
            assert t.grad is not None, k
            got = npy(t.grad) / factor
            got = got[b] if batched else got
            err, bar = np.abs(got - want[k]).max(), BAR * max(1.0, np.abs(want[k]).max())
            print(section, "system", b, k, "err", err, "bar", bar)
            note(section, err, bar, "%s of system %d" % (k, b))
            assert np.isfinite(got).all() and err < bar, (b, k, err, bar)


# ---- 1. batches whose systems freeze at different solves ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.LAYER_BATCHES)
def test_batch_of_systems_that_freeze_at_different_solves(kind):
    """One batched call; every system's solves, act and gradients are those of its own reference run, the upstream gradients
    random per system."""
    ps, soft = R.layer_batch(kind)
    want = [p["run"]["iters"] for p in ps]
    assert len(ps) == 5 and len(set(want)) >= 2
    ts = tensors(ps, soft, True)
    x, lam, info = layer(ts, soft, ps[0]["s"].rho)
    print(kind, "solves", info.iters.tolist(), "want", want)
    assert info.iters.tolist() == want and info.polished.tolist() == [_lib.POLISH_ACCEPTED] * 5
    check_forward(ps, info)
    xbar, lbar = upstream(21, x, lam)
    loss_of(x, lam, xbar, lbar).backward()
    check_grads("1", ps, soft, ts, x, lam, xbar, lbar)


# ---- 2. stale assemblies ------------------------------------------------------------------------------------------------------------
def stale_problems(kind, n, first=0):
    """n problems at 6/3/9 from the fifth-long lists of section 1, starting at `first`: constructed (hard) or mixed (soft)."""
    ps, soft = R.layer_batch("constructed" if kind == "hard" else "mixed")
    return [ps[(first + i) % len(ps)] for i in range(n)], soft


def forward(kind, n, first=0, requires_grad=True, seed=31):
    """A forward pass of the kind's layer on n problems (n = 1: unbatched) -> dict ps, soft, ts, x, lam, xbar, lbar, loss, sol."""
    ps, soft = stale_problems(kind, n, first)
    ts = tensors(ps, soft, n > 1, requires_grad)
    x, lam, info = layer(ts, soft, ps[0]["s"].rho)
    check_forward(ps, info)
    xbar, lbar = upstream(seed, x, lam)
    return dict(ps=ps, soft=soft, ts=ts, x=x, lam=lam, xbar=xbar, lbar=lbar, loss=loss_of(x, lam, xbar, lbar), sol=solver_of(ps, n))


def check(section, f, factor=1.0):
    check_grads(section, f["ps"], f["soft"], f["ts"], f["x"], f["lam"], f["xbar"], f["lbar"], factor=factor)


def intrude(which, kind, n):
    """One call that replaces (a - d) or invalidates (e) the assembly of the cached solver of 6/3/9, batch n, fp64.  c returns
    what checks the intruder's own backward pass afterwards."""
    import gato_python_amd
    other = dict(hard="soft", soft="hard")[kind]
    if which in "ab":
        forward(kind if which == "a" else other, n, first=3, requires_grad=False)
        return None
    ps, _ = stale_problems("hard", n, first=3)
    ts = tensors(ps, False, n > 1, which == "c")
    rho = ps[0]["s"].rho
    if which == "c":
        lam, dz = gato_python_amd.kkt_solve(*ts[:7], rho=rho, **F64)
        dbar, lbar = upstream(33, dz, lam)
        loss = (dz * dev(dbar)).sum() + (lam * dev(lbar)).sum()

        def later():
            loss.backward()
            for b, p in enumerate(ps):
                want = kgr.dense_reference(p["s"], dbar.reshape(n, -1)[b], lbar.reshape(n, -1)[b])
                for k, t in zip(D.KEYS[:7], ts):
                    got = npy(t.grad)[b] if n > 1 else npy(t.grad)
                    err, bar = np.abs(got - want[k]).max(), BAR * max(1.0, np.abs(want[k]).max())
                    note("2 kkt_solve", err, bar, "%s of system %d" % (k, b))
                    assert err < bar, ("kkt_solve", b, k, err, bar)
        return later
    if which == "d":
        res = gato_python_amd.box_qp(*ts, rho=rho, method="admm", max_admm_iters=50, **F64)
        assert res.x.shape[-1] == ps[0]["s"].N
        return None
    assert which == "e"
    with torch.no_grad():
        lo, hi = ts[9].view(n, -1), ts[10].view(n, -1)
        lo[n - 1, 0], hi[n - 1, 0] = 1.0, -1.0                     # lo > hi in one control of the last system
    with pytest.raises(ValueError, match="BAD_BOUNDS"):
        gato_python_amd.box_qp(*ts, rho=rho, method="pdas", **F64)
    return None


STALE = [(kind, n, which) for kind in ("hard", "soft") for n in (1, 3) for which in "abcde"]


@pytest.mark.parametrize("kind,n,which", STALE, ids=["%s-%d-%s" % c for c in STALE])
def test_backward_after_an_intruder(kind, n, which):
    """Forward 1, another call on the same cached solver, then the backward pass of forward 1: it rebuilds its assembly with
    exactly one assembly and gives the reference's gradients."""
    f = forward(kind, n)
    sol = f["sol"]
    gen = sol.get_option("assembly_gen")
    later = intrude(which, kind, n)
    assert solver_of(f["ps"], n) is sol
    if which == "e":
        assert sol.get_option("assembly_valid") == 0
    else:
        assert sol.get_option("assembly_gen") != gen and sol.get_option("assembly_valid") == 1
    gen = sol.get_option("assembly_gen")
    f["loss"].backward()
    assert sol.get_option("assembly_gen") == gen + 1 and sol.get_option("assembly_valid") == 1
    check("2", f)
    if later is not None:
        later()                                                    # its assembly was replaced by the layer's rebuild


ORDER = [(a, b, n) for a in ("hard", "soft") for b in ("hard", "soft") for n in (1, 3)]


@pytest.mark.parametrize("kind_a,kind_b,n", ORDER, ids=["%s-%s-%d" % c for c in ORDER])
def test_forward_a_forward_b_backward_b_backward_a(kind_a, kind_b, n):
    fa = forward(kind_a, n)
    fb = forward(kind_b, n, first=3, seed=32)
    sol = fa["sol"]
    assert fb["sol"] is sol
    gen = sol.get_option("assembly_gen")
    fb["loss"].backward()
    assert sol.get_option("assembly_gen") == gen                   # B's assembly is the solver's: no rebuild
    fa["loss"].backward()
    assert sol.get_option("assembly_gen") == gen + 1
    check("2", fb)
    check("2", fa)


RETAIN = [(kind, n, stale) for kind in ("hard", "soft") for n in (1, 3) for stale in (False, True)]


@pytest.mark.parametrize("kind,n,stale", RETAIN, ids=["%s-%d-%s" % (k, n, "stale" if s else "fresh") for k, n, s in RETAIN])
def test_backward_twice_doubles_every_grad(kind, n, stale):
    """backward(retain_graph=True) twice: .grad is twice the first pass's.  Bar of the doubling: the two passes run the same
    launches on the same operands; if a sum in them is ordered differently the adjoints differ by the rounding of a solve whose
    matrix has cond <= 1e8 (the seed walks' COND_CAP), 1e8 * 2^-53 = 1.1e-8 relative."""
    f = forward(kind, n)
    if stale:
        intrude("a", kind, n)
    f["loss"].backward(retain_graph=True)
    once = [t.grad.clone() for t in f["ts"]]
    check("2", f)
    f["loss"].backward()
    for k, t, g in zip(keys_of(f["soft"]), f["ts"], once):
        err = float((t.grad - 2 * g).abs().max())
        assert err <= 1.1e-8 * max(1.0, float(g.abs().max())), (k, err)
    check("2", f, factor=2.0)


# ---- 3. one system of a batch that does not converge -------------------------------------------------------------------------------
def trio(kind):
    return (D.di_trio(), False) if kind == "hard" else (R.di_soft_trio(), True)


def trio_forward(kind):
    ps, soft = trio(kind)
    ts = tensors(ps, soft, True)
    x, lam, info = layer(ts, soft, ps[0]["s"].rho)
    print(kind, "status", info.status.tolist(), "iters", info.iters.tolist())
    assert int(info.status[1]) in (_lib.QP_MAX_ITERS, _lib.QP_NONFINITE) and int(info.polished[1]) != _lib.POLISH_ACCEPTED
    assert not info.x[1].any() and not info.lam[1].any() and not x[1].any() and not lam[1].any()
    check_forward(ps, info, systems=(0, 2))
    return ps, soft, ts, x, lam


@pytest.mark.parametrize("stale", (False, True), ids=("fresh", "stale"))
@pytest.mark.parametrize("kind", ("hard", "soft"))
def test_batch_with_a_system_that_does_not_converge(kind, stale):
    """A loss over the two good systems: their gradients are the reference's, the bad system's are exactly zero - nothing of
    its singular re-solve leaks - also when the rebuild re-assembles the singular system."""
    ps, soft, ts, x, lam = trio_forward(kind)
    xbar, lbar = upstream(41, x, lam)
    xbar[1], lbar[1] = 0.0, 0.0
    loss = loss_of(x, lam, xbar, lbar)
    sol = solver_of(ps, 3)
    if stale:
        gen = sol.get_option("assembly_gen")
        with torch.no_grad():
            ts2 = [t.detach().clone() for t in ts]
            ts2[6].mul_(0.5)                                        # another c: other right-hand sides, the same matrices
        layer(ts2, soft, ps[0]["s"].rho)
        assert solver_of(ps, 3) is sol and sol.get_option("assembly_gen") != gen
    gen = sol.get_option("assembly_gen")
    loss.backward()
    assert sol.get_option("assembly_gen") == gen + (1 if stale else 0)
    check_grads("3", ps, soft, ts, x, lam, xbar, lbar, systems=(0, 2))
    for k, t in zip(keys_of(soft), ts):
        g = npy(t.grad)
        assert np.isfinite(g).all() and not g[1].any(), k


@pytest.mark.parametrize("kind", ("hard", "soft"))
def test_loss_on_the_system_that_did_not_converge_raises(kind):
    ps, soft, ts, x, lam = trio_forward(kind)
    xbar, lbar = upstream(42, x, lam)
    with pytest.raises(RuntimeError, match=r"systems \[1\]"):
        loss_of(x, lam, xbar, lbar).backward()
    assert all(t.grad is None for t in ts)


# ---- 4. subsets of inputs and of outputs -----------------------------------------------------------------------------------------
_ALL = {}


def single(kind):
    ps, soft = R.layer_batch("constructed" if kind == "hard" else "mixed", count=1)
    return ps, soft


def all_inputs(kind):
    """The unbatched 6/3/9 run with every input requiring a gradient and both outputs in the loss -> (xbar, lbar, {name: grad})."""
    if kind not in _ALL:
        ps, soft = single(kind)
        ts = tensors(ps, soft, False)
        x, lam, info = layer(ts, soft, ps[0]["s"].rho)
        check_forward(ps, info)
        xbar, lbar = upstream(51, x, lam)
        loss_of(x, lam, xbar, lbar).backward()
        check_grads("4", ps, soft, ts, x, lam, xbar, lbar)
        _ALL[kind] = (xbar, lbar, {k: t.grad.clone() for k, t in zip(keys_of(soft), ts)})
    return _ALL[kind]


SUBSETS = [("q",), ("c",), ("Q",), ("B",), ("x_lo", "u_hi"), ("x_soft",), ("u_soft", "R")]
INPUTS = [(kind, sub) for kind in ("hard", "soft") for sub in SUBSETS if kind == "soft" or all(k in D.KEYS for k in sub)]


@pytest.mark.parametrize("kind,subset", INPUTS, ids=["%s-%s" % (k, "+".join(s)) for k, s in INPUTS])
def test_subset_of_inputs(kind, subset):
    """Only `subset` requires a gradient: its grads are those of the all-inputs run byte for byte (the same kernels see the
    same operands) and every other input's .grad stays None."""
    xbar, lbar, full = all_inputs(kind)
    ps, soft = single(kind)
    ts = tensors(ps, soft, False, requires_grad=subset)
    x, lam, _ = layer(ts, soft, ps[0]["s"].rho)
    loss_of(x, lam, xbar, lbar).backward()
    for k, t in zip(keys_of(soft), ts):
        if k in subset:
            assert t.grad is not None and npy(t.grad).tobytes() == npy(full[k]).tobytes(), k
        else:
            assert t.grad is None, k


OUTPUTS = ("x", "lam", "x_strided", "x_expanded")


@pytest.mark.parametrize("mode", OUTPUTS)
@pytest.mark.parametrize("kind", ("hard", "soft"))
def test_subset_of_outputs(kind, mode):
    """A loss of x alone (lam_bar is None), of lam alone (x_bar is None), of every other entry of x, and x.sum() (an expanded
    x_bar): the reference with the missing upstream gradient zero."""
    ps, soft = single(kind)
    ts = tensors(ps, soft, False)
    x, lam, _ = layer(ts, soft, ps[0]["s"].rho)
    xbar, lbar = upstream(52, x, lam)
    if mode == "x":
        loss, lbar = (x * dev(xbar)).sum(), np.zeros_like(lbar)
    elif mode == "lam":
        loss, xbar = (lam * dev(lbar)).sum(), np.zeros_like(xbar)
    elif mode == "x_strided":
        loss, lbar = (x[::2] * dev(xbar[::2])).sum(), np.zeros_like(lbar)
        xbar[1::2] = 0.0
    else:
        loss, xbar, lbar = x.sum(), np.ones_like(xbar), np.zeros_like(lbar)
    loss.backward()
    check_grads("4", ps, soft, ts, x, lam, xbar, lbar)


@pytest.mark.parametrize("kind", ("hard", "soft"))
def test_zero_loss_gives_zero_grads_without_a_re_solve(kind):
    ps, soft = single(kind)
    ts = tensors(ps, soft, False)
    x, lam, _ = layer(ts, soft, ps[0]["s"].rho)
    sol = solver_of(ps, 1)
    ag().kkt_solve(*(t.detach() for t in ts[:7]), rho=ps[0]["s"].rho, **F64)      # a re-solve would now have to rebuild first
    gen = sol.get_option("assembly_gen")
    (0.0 * x.sum()).backward()
    assert sol.get_option("assembly_gen") == gen
    for k, t in zip(keys_of(soft), ts):
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any(), k


# ---- 5. broadcast bounds and weights ----------------------------------------------------------------------------------------------
def check_summed(ts, wants, names):
    """t.grad of each named argument against the full-shaped reference gradients (one per system) summed over the broadcast
    dimensions (box_qp_pdas_ref.sum_to)."""
    for k, t in zip(names, ts):
        full = np.stack([w[k] for w in wants]) if len(wants) > 1 else wants[0][k]
        want = D.sum_to(full, tuple(t.shape))
        assert t.grad is not None and t.grad.shape == t.shape, k
        err, bar = np.abs(npy(t.grad) - want).max(), BAR * max(1.0, np.abs(want).max())
        print("5", k, tuple(t.shape), "err", err, "bar", bar, "want", np.abs(want).max())
        note("5", err, bar, "%s %s" % (k, tuple(t.shape)))
        assert err < bar, (k, err, bar)


def test_hard_bounds_as_numbers_and_0d_tensors():
    p = D.di_broadcast()
    s = p["s"]
    blocks = tensors([p], False, False)[:7]
    u_lo, u_hi = scalar(-0.5), scalar(0.5)
    assert u_lo.dim() == 0 and u_hi.dim() == 0 and np.all(p["lo"][np.isfinite(p["lo"])] == -0.5) and np.all(p["hi"][np.isfinite(p["hi"])] == 0.5)
    import gato_python_amd
    x, lam, info = gato_python_amd.box_qp_layer(*blocks, -np.inf, np.inf, u_lo, u_hi, rho=s.rho, method="pdas", **F64)
    check_forward([p], info)
    xbar, lbar = upstream(61, x, lam)
    loss_of(x, lam, xbar, lbar).backward()
    want = R.reference_grads(p, npy(x), npy(lam), xbar, lbar)
    assert np.count_nonzero(want["u_lo"]) + np.count_nonzero(want["u_hi"]) == 7 and np.count_nonzero(want["u_hi"]) >= 1
    check_summed(blocks + [u_lo, u_hi], [want], D.KEYS[:7] + ("u_lo", "u_hi"))


def test_soft_bounds_per_state_per_control_and_a_0d_weight():
    p = R.di_soft_trio()[0]
    s = p["s"]
    S, C, K = s.S, s.C, s.K
    arrs = R.soft_math_arrays(p)
    blocks = [dev(a, True) for a in arrs[:7]]
    x_lo, x_hi = dev(arrs[7][1], True), dev(arrs[8][1], True)                    # [S]: the position infinite, the velocity +-0.57
    u_lo, u_hi = dev(arrs[9][:1], True), dev(arrs[10][:1], True)                 # [1, C]
    x_soft = scalar(R.WEIGHT)
    for full, t in zip(arrs[7:12], (x_lo, x_hi, u_lo, u_hi, x_soft)):
        assert np.array_equal(np.broadcast_to(npy(t), full.shape), full)
    assert x_lo.shape == (S,) and u_lo.shape == (1, C) and x_soft.dim() == 0 and np.isinf(npy(x_lo)[0]) and not arrs[12].any()
    import gato_python_amd
    x, lam, info = gato_python_amd.box_qp_layer(*blocks, x_lo, x_hi, u_lo, u_hi, rho=s.rho, method="pdas", x_soft=x_soft,
                                                u_soft=0.0, **F64)
    check_forward([p], info)
    xbar, lbar = upstream(62, x, lam)
    loss_of(x, lam, xbar, lbar).backward()
    want = R.reference_grads(p, npy(x), npy(lam), xbar, lbar)
    assert np.count_nonzero(want["x_soft"]) == 6 and np.count_nonzero(want["u_lo"]) + np.count_nonzero(want["u_hi"]) == 14
    check_summed(blocks + [x_lo, x_hi, u_lo, u_hi, x_soft], [want], R.SOFT_KEYS[:12])
    assert npy(x_lo.grad)[0] == 0.0 and npy(x_hi.grad)[0] == 0.0                 # the infinite position bounds


def test_bounds_and_weights_shared_by_a_batch():
    """B = 2: x_lo, x_hi, x_soft of shape [K, S] and u_lo, u_hi of shape [K-1, C], one tensor for both systems: the gradient is
    the sum over the batch."""
    ps = R.di_soft_pair()
    s = ps[0]["s"]
    arrs = [R.soft_math_arrays(p) for p in ps]
    for a, b in zip(arrs[0][7:], arrs[1][7:]):
        assert np.array_equal(a, b)
    blocks = [dev(a, True) for a in D.batched(arrs)[:7]]
    shared = [dev(a, True) for a in arrs[0][7:12]]
    assert shared[0].shape == (s.K, s.S) and shared[2].shape == (s.K - 1, s.C)
    import gato_python_amd
    x, lam, info = gato_python_amd.box_qp_layer(*blocks, *shared[:4], rho=s.rho, method="pdas", x_soft=shared[4], u_soft=0.0, **F64)
    check_forward(ps, info)
    xbar, lbar = upstream(63, x, lam)
    loss_of(x, lam, xbar, lbar).backward()
    wants = [R.reference_grads(p, npy(x)[b], npy(lam)[b], xbar[b], lbar[b]) for b, p in enumerate(ps)]
    for b, w in enumerate(wants):
        for k, t in zip(D.KEYS[:7], blocks):
            err, bar = np.abs(npy(t.grad)[b] - w[k]).max(), BAR * max(1.0, np.abs(w[k]).max())
            note("5", err, bar, "%s of system %d" % (k, b))
            assert err < bar, (b, k, err, bar)
    assert all(np.count_nonzero(w["x_soft"]) >= 1 for w in wants)
    check_summed(shared, wants, R.SOFT_KEYS[7:12])
