"""The inputs of tests/test_gpu_box_qp_layer_sweep.py on the CPU: from the numpy references alone, that every batch holds systems
with different solve counts and every run meets the seed rule, that the double-integrator trios end as the GPU tests assume,
that the broadcast cases are what they are said to be, and that the gradient of a broadcast bound or weight is the full-shaped
reference gradient summed - against central differences of the reference solution on the fixed final act, without torch."""
import numpy as np
import pytest

import box_qp_active_ref as AS
import box_qp_pdas_ref as D
import box_qp_polish_ref as P
import box_qp_ref as ref
import box_qp_soft_ref as R

SOLVES = dict(control=[8, 11, 17, 13, 8], constructed=[4, 4, 5, 3, 5], soft=[6, 9, 7, 7, 9], mixed=[18, 9, 11, 8, 9])


def ok(p):
    run = p["run"]
    return AS.walk_ok(run, p["H"], p["Cm"], p.get("w"), R.soft_active_on_the_way(p) if "w" in p else None)


@pytest.mark.parametrize("kind", R.LAYER_BATCHES)
def test_batches_hold_systems_with_different_solve_counts(kind):
    """Five problems per generator, at least two distinct solve counts (the counts are pinned: a change of a generator shows
    here, not as a uniform batch on the GPU), every run within the seed rule and within the layer's default of 30 solves, one rho."""
    ps, soft = R.layer_batch(kind)
    got = [p["run"]["iters"] for p in ps]
    print(kind, got, [p["seed"] for p in ps])
    assert len(ps) == 5 and got == SOLVES[kind] and len(set(got)) >= 2 and max(got) <= 30
    assert all(ok(p) for p in ps) and all(("w" in p) == soft for p in ps)
    assert len({p["s"].rho for p in ps}) == 1 and len({(p["s"].S, p["s"].C, p["s"].K) for p in ps}) == 1
    if kind in ("constructed", "mixed"):                       # the 6/3/9 problems of the stale-assembly and subset tests
        assert (ps[0]["s"].S, ps[0]["s"].C, ps[0]["s"].K) == R.LAYER_SHAPE
        assert all((p["run"]["act"] != 0).any() for p in ps)
    if kind == "mixed":
        for p in ps[:3]:
            sa = P.soft_set(p["run"]["act"], p["w"])
            assert sa.any() and ((p["run"]["act"] != 0) & ~sa).any()        # soft-active and hard-active at the end


def test_math_arrays_are_the_problem():
    """math_arrays / soft_math_arrays give back H, C, g, c, lo, hi and w of the problem, and batched() stacks them."""
    for p in (R.layer_batch("constructed", count=1)[0][0], R.layer_batch("mixed", count=1)[0][0], D.di_broadcast()):
        s = p["s"]
        arrs = R.soft_math_arrays(p)
        H, Cm, g, c = P.dense_from_blocks(*arrs[:7], s.rho)
        for got, want in ((H, p["H"]), (Cm, p["Cm"]), (g, p["g"]), (c, p["c"])):
            assert np.array_equal(got, want)
        assert np.array_equal(ref.dz_layout(arrs[7], arrs[9], s.S, s.C, s.K), p["lo"])
        assert np.array_equal(ref.dz_layout(arrs[8], arrs[10], s.S, s.C, s.K), p["hi"])
        assert np.array_equal(ref.dz_layout(arrs[11], arrs[12], s.S, s.C, s.K), p["w"] if "w" in p else np.zeros(s.N))
        assert [a.tobytes() for a in arrs[:11]] == [a.tobytes() for a in D.math_arrays(s, p["lo"], p["hi"])]
    two = D.batched([arrs, arrs])
    assert all(t.shape == (2,) + a.shape and np.array_equal(t[1], a) for t, a in zip(two, arrs))


def test_sum_to():
    full = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    assert D.sum_to(full, ()) == full.sum() and D.sum_to(full, ()).shape == ()
    assert np.array_equal(D.sum_to(full, (4,)), full.sum((0, 1)))
    assert np.array_equal(D.sum_to(full, (1, 4)), full.sum((0, 1))[None])
    assert np.array_equal(D.sum_to(full, (3, 4)), full.sum(0))
    assert np.array_equal(D.sum_to(full, (3, 1)), full.sum((0, 2))[:, None])
    assert np.array_equal(D.sum_to(full, (2, 3, 4)), full)


def test_hard_trio_outcomes():
    good0, bad, good1 = D.di_trio()
    assert bad["run"]["status"] == AS.NONFINITE and bad["run"]["iters"] == 2
    for p in (good0, good1):
        assert AS.walk_ok(p["run"], p["H"], p["Cm"]) and p["run"]["iters"] <= 30 and (p["run"]["act"] != 0).any()
    assert not np.array_equal(good0["c"], good1["c"]) and len({p["s"].rho for p in (good0, bad, good1)}) == 1


def test_soft_trio_outcomes():
    soft, bad, good = R.di_soft_trio()
    run = soft["run"]
    sa = P.soft_set(run["act"], soft["w"])
    n = soft["s"].S + soft["s"].C
    ctl = np.arange(soft["s"].N) % n >= soft["s"].S
    assert run["status"] == AS.CONVERGED and run["iters"] == 11 and ok(soft)
    assert int(sa.sum()) == 6 and not sa[ctl].any() and int(((run["act"] != 0) & ~sa).sum()) == 14 and ctl[(run["act"] != 0) & ~sa].all()
    assert np.array_equal(soft["w"], R.state_weights(soft["s"], 100.0))
    hard_bad, hard_good = D.di_trio()[1], D.di_trio()[2]
    assert not bad["w"].any() and bad["run"]["status"] == AS.NONFINITE and bad["run"]["iters"] == 2
    assert np.array_equal(bad["run"]["act"], hard_bad["run"]["act"])
    assert not good["w"].any() and good["run"]["status"] == AS.CONVERGED and good["run"]["iters"] == hard_good["run"]["iters"] <= 30
    assert np.array_equal(good["run"]["act"], hard_good["run"]["act"]) and AS.walk_ok(good["run"], good["H"], good["Cm"])


def loss_on_act(p, xbar, lbar, lo=None, hi=None, w=None):
    """xbar . x + lbar . lam of the reduced solution on p's final act with some of lo, hi, w replaced."""
    lo, hi = p["lo"] if lo is None else lo, p["hi"] if hi is None else hi
    act = p["run"]["act"]
    if "w" in p:
        x, _, lam = P.reduced_solve(p["H"], p["Cm"], p["g"], p["c"], lo, hi, act, p["w"] if w is None else w)
    else:
        x, _, lam = P.reduced_solve(p["H"], p["Cm"], p["g"], p["c"], lo, hi, act)
    return float(xbar @ x + lbar @ lam)


def test_hard_broadcast_case_and_the_summed_gradient_of_a_0d_bound():
    """double_integrator(K=8, u_max=0.5): 7 solves, 7 active controls, margin 0.039, every control bound the one number; the sum
    of the reference's u_hi (u_lo) gradient is the derivative of the loss along that number, by central differences."""
    p = D.di_broadcast()
    s, run = p["s"], p["run"]
    n = s.S + s.C
    ctl = np.arange(s.N) % n >= s.S
    assert run["status"] == AS.CONVERGED and run["iters"] == 7 and AS.walk_ok(run, p["H"], p["Cm"])
    assert int((run["act"] != 0).sum()) == 7 and ctl[run["act"] != 0].all() and 0.038 < AS.min_margin(run) < 0.040
    assert np.all(p["hi"][ctl] == 0.5) and np.all(p["lo"][ctl] == -0.5) and np.all(np.isinf(p["lo"][~ctl])) and np.all(np.isinf(p["hi"][~ctl]))
    assert (run["act"] > 0).any()
    rng = np.random.default_rng(61)
    xbar, lbar = rng.standard_normal(s.N), rng.standard_normal(s.S * s.K)
    want = R.reference_grads(p, run["x"], run["lam"], xbar, lbar)
    assert np.count_nonzero(want["u_lo"]) + np.count_nonzero(want["u_hi"]) == 7
    h = 1e-3                                                    # the reduced solution is linear in the bounds: any step is exact
    for key, name, b in (("u_hi", "hi", 0.5), ("u_lo", "lo", -0.5)):
        at = lambda t: {name: np.where(ctl, t, p[name])}
        fd = (loss_on_act(p, xbar, lbar, **at(b + h)) - loss_on_act(p, xbar, lbar, **at(b - h))) / (2 * h)
        an = float(D.sum_to(want[key], ()))
        print(key, fd, an)
        assert abs(fd - an) <= 1e-8 * max(1.0, abs(an)), (key, fd, an)


def test_soft_broadcast_cases_and_the_summed_gradient_of_a_0d_weight():
    """The weight-100 velocity-bounded double integrator: one [S] row of state bounds, one [1, C] row of control bounds, one
    weight for every state; the sum of the reference's x_soft gradient against central differences along that weight.  The pair
    of the batched test shares its box and weights, and each system has a soft-active state at the end."""
    p = R.di_soft_trio()[0]
    s, run = p["s"], p["run"]
    arrs = R.soft_math_arrays(p)
    for a in arrs[7:12]:
        assert np.array_equal(a, np.broadcast_to(a[:1], a.shape))
    assert np.isinf(arrs[7][0, 0]) and np.isinf(arrs[8][0, 0]) and arrs[8][0, 1] == 0.57 and np.all(arrs[11] == 100.0) and not arrs[12].any()
    rng = np.random.default_rng(62)
    xbar, lbar = rng.standard_normal(s.N), rng.standard_normal(s.S * s.K)
    want = R.reference_grads(p, run["x"], run["lam"], xbar, lbar)
    assert np.count_nonzero(want["x_soft"]) == 6 and np.count_nonzero(want["u_lo"]) + np.count_nonzero(want["u_hi"]) == 14
    assert not want["x_lo"][:, 0].any() and not want["x_hi"][:, 0].any()
    an = float(D.sum_to(want["x_soft"], ()))
    h = 1e-2                                                    # central differences: error h^2 f''' / 6, f a rational function of w = 100
    fd = (loss_on_act(p, xbar, lbar, w=R.state_weights(s, 100.0 + h)) - loss_on_act(p, xbar, lbar, w=R.state_weights(s, 100.0 - h))) / (2 * h)
    print("x_soft", fd, an)
    assert an != 0 and abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (fd, an)
    pair = R.di_soft_pair()
    for q in pair:
        assert ok(q) and q["run"]["iters"] <= 30 and P.soft_set(q["run"]["act"], q["w"]).any()
    a, b = pair
    assert all(np.array_equal(a[k], b[k]) for k in ("lo", "hi", "w")) and not np.array_equal(a["c"], b["c"])
    assert not np.array_equal(a["run"]["act"], b["run"]["act"])
