"""CPU suite of the CSR entry to the cross solve: the reference scatter of tests/cross_csr_ref.py against
the blocks its CSRs were built from and against an independent dense statement of what such a CSR means, the entry kinds every
pattern of tests/test_gpu_cross_csr.py promises, the unchanged defaults of the producers, and the refusals of
kkt_solve_csr(cross=True) that need no GPU."""
import numpy as np
import pytest
import torch

import cross_csr_ref as R
import cross_ref as X
from gato_python_amd import kkt, synth

CELLS = [(2, 1, 3), (4, 2, 5), (6, 3, 2), (14, 7, 3)]
PATTERN_K = 5                                       # the knots of the pattern cells of the GPU suite


@pytest.mark.parametrize("S,C,K", CELLS, ids=["%d-%d-%d" % c for c in CELLS])
@pytest.mark.parametrize("base", [R.csr_both, R.csr_full], ids=["csr_matrix", "full"])
def test_scatter_reproduces_the_blocks(S, C, K, base):
    """Both-triangle CSR -> exactly the G_dense, C_dense and M_blocks it was built from, every kept entry at its own slot."""
    for cell in X.batch_cells(S, C, K, 3, seed=K):
        s = base(cell)
        sc = R.scatter(s)
        Gd, Cd, _, _, Mb = X.pack(*cell[0], cell[1])
        assert np.array_equal(sc["G"], Gd) and np.array_equal(sc["C"], Cd) and np.array_equal(sc["M"], Mb)
        kept = sc["slotM"] >= 0
        assert np.array_equal(sc["M"][sc["slotM"][kept]], s.G_val[kept]) and kept.sum() == (sc["kind"] == R.KEPT).sum()
        cnt = R.counts(sc)
        assert cnt[R.KEPT] == cnt[R.MIRROR] > 0 and cnt[R.OVERWRITTEN] == cnt[R.DROPPED] == cnt[R.LOST] == 0


@pytest.mark.parametrize("S,C,K", CELLS, ids=["%d-%d-%d" % c for c in CELLS])
def test_dense_meaning_of_the_csr(S, C, K):
    """synth.dense_kkt of the both-triangle CSR (scipy sums the entries into a dense symmetric G) solved densely is
    cross_ref.dense_solve on the blocks with M: the CSR means the problem with the cross term."""
    for cell in X.batch_cells(S, C, K, 3, seed=K):
        s = R.csr_both(cell)
        A, rhs = synth.dense_kkt(s)
        assert np.array_equal(A, A.T)
        x = X.solve_refined(A, rhs)
        dz, lam = X.dense_solve(*cell)
        assert np.abs(x[:s.N] - dz).max() <= 1e-11 * np.abs(dz).max()
        assert np.abs(x[s.N:] - lam).max() <= 1e-11 * np.abs(lam).max()
        # and the scatter's own blocks state the same problem
        dz2, lam2 = X.dense_solve(*R.cell_of(R.scatter(s), s))
        assert np.array_equal(dz2, dz) and np.array_equal(lam2, lam)


@pytest.mark.parametrize("name", sorted(R.BUILDERS))
@pytest.mark.parametrize("S,C", X.SHAPES, ids=["%d-%d" % c for c in X.SHAPES])
def test_patterns_hold_the_kinds_they_promise(S, C, name):
    cells = X.batch_cells(S, C, PATTERN_K, 3, seed=PATTERN_K)
    systems = [R.BUILDERS[name](cell) for cell in cells]
    R.stacked(systems, np.float64)                                          # one set of index arrays for the batch
    cnt = R.counts(R.scatter(systems[0]))
    for k in R.PROMISES[name]:
        assert cnt[k] > 0, (name, k, cnt)
    if name == "upper":
        assert cnt[R.MIRROR] == 0
    if name == "shuffled":
        assert (systems[0].G_val == 0).sum() > 0


def test_upper_storage_states_the_same_problem():
    S, C, K = 4, 2, 3
    cell = X.batch_cells(S, C, K, 1)[0]
    a, b = R.scatter(R.csr_both(cell)), R.scatter(R.csr_upper(cell, R.csr_both))
    assert all(np.array_equal(a[k], b[k]) for k in "GMC")


def test_defaults_give_unchanged_arrays():
    """blocks_to_csr / make_system / get_kkt without M emit what they always did: entry for entry the arrays of a restatement
    that knows nothing of M (scipy's csr_matrix of the dense block-diagonal G), and nothing between the Q and R parts."""
    from scipy import sparse
    for S, C, K, dense_q in ((2, 1, 5, False), (4, 2, 3, True)):
        blocks = synth.make_blocks(S, C, K, seed=3, dense_q=dense_q)
        s = synth.blocks_to_csr(*blocks, dense_q=dense_q)
        s2 = synth.make_system(S, C, K, seed=3, dense_q=dense_q)
        for a, b in zip(s.csr_args(), s2.csr_args()):
            assert np.array_equal(a, b)
        n = S + C
        rows = np.repeat(np.arange(s.N), np.diff(s.G_row))
        assert not np.any((rows % n < S) != (s.G_col % n < S))
        G = sparse.csr_matrix(X.dense_kkt(*blocks[:4], None, 0.0)[:s.N, :s.N])
        assert np.array_equal(G.indptr, s.G_row) and np.array_equal(G.indices, s.G_col) and np.array_equal(G.data, s.G_val)
    p = kkt.pendulum_problem()
    ref = synth.pendulum_system()
    assert np.array_equal(p.G_row, ref.G_row) and np.array_equal(p.G_col, ref.G_col) and np.array_equal(p.C_col, ref.C_col)


def test_producers_with_M_emit_both_triangles_like_csr_matrix():
    from scipy import sparse
    S, C, K = 4, 2, 3
    blocks, M = X.cell(S, C, K, seed=2, dense_q=True)
    s = synth.blocks_to_csr(*blocks, M=M)
    G = sparse.csr_matrix(X.dense_kkt(*blocks[:4], M, 0.0)[:s.N, :s.N])
    assert np.array_equal(G.indptr, s.G_row) and np.array_equal(G.indices, s.G_col) and np.array_equal(G.data, s.G_val)
    s2 = synth.make_system(S, C, K, seed=2, dense_q=True, cross_scale=0.5)
    assert all(np.array_equal(a, b) for a, b in zip(s.csr_args(), s2.csr_args()))
    # get_kkt: a constant M, the gradient terms M u and M' (x - xg)
    rng = np.random.default_rng(0)
    plant = kkt.LinearPlant(np.eye(S) + 0.1 * rng.standard_normal((S, S)), rng.standard_normal((S, C)))
    x, u = rng.standard_normal((K, S)), rng.standard_normal((K - 1, C))
    xg = rng.standard_normal(S)
    Q, Rr, Mc = 2.0 * np.eye(S), 0.5 * np.eye(C), 0.1 * rng.standard_normal((S, C))
    p0 = kkt.get_kkt(plant, x, u, x[0], xg, 0.1, Q, Rr, Q)
    p1 = kkt.get_kkt(plant, x, u, x[0], xg, 0.1, Q, Rr, Q, M=Mc)
    sc = R.scatter(p1)
    assert np.array_equal(R.blocks_of(sc, p1)[4], np.stack([Mc] * (K - 1)))
    assert np.array_equal(R.scatter(p0)["G"], sc["G"]) and np.array_equal(p0.C_val, p1.C_val) and np.array_equal(p0.c, p1.c)
    n = S + C
    for k in range(K - 1):
        assert np.allclose(p1.g[k * n:k * n + S] - p0.g[k * n:k * n + S], Mc @ u[k], rtol=0, atol=1e-15)
        assert np.allclose(p1.g[k * n + S:(k + 1) * n] - p0.g[k * n + S:(k + 1) * n], Mc.T @ (x[k] - xg), rtol=0, atol=1e-15)
    assert np.array_equal(p1.g[(K - 1) * n:], p0.g[(K - 1) * n:])
    A, _ = synth.dense_kkt(p1, with_rho=False)
    assert np.array_equal(A, A.T)


# ---- refusals of kkt_solve_csr(cross=True) that arrive without a GPU -------------------------------------------------------------
def _args(s, dt=torch.float64):
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    return (t(s.G_row, torch.int32), t(s.G_col, torch.int32), t(s.G_val, dt), t(s.C_row, torch.int32), t(s.C_col, torch.int32),
            t(s.C_val, dt), t(s.g, dt), t(s.c, dt))


KW = dict(rho=1e-3, exit_tol=1e-8, max_iters=100)


def test_a_mirror_entry_without_its_partner_is_refused_on_the_host():
    from gato_python_amd.autograd import kkt_solve_csr
    S, C, K = 4, 2, 3
    cell = X.cell(S, C, K, dense_q=True)
    n = S + C
    s = R.csr_both(cell)
    lower = R._with_G(s, R.P.thin_rows(s.G_row, s.G_col, s.G_val, lambda r, c: not (r % n < S and c % n >= S)))   # lower-only storage
    with pytest.raises(ValueError, match="no partner"):
        kkt_solve_csr(*_args(lower), cross=True, **KW)
    one = R._with_G(s, R.P.thin_rows(s.G_row, s.G_col, s.G_val, lambda r, c: not (r == 1 and c == S)))            # one partner missing
    with pytest.raises(ValueError, match=r"1 entries.*row %d, column 1" % S):
        kkt_solve_csr(*_args(one), cross=True, **KW)
    # the partner is found the way the scatter addresses (knot of the row, col % n).  A mirror entry in a column of the last knot
    # whose raw transpose is a state row of the last knot - dropped, that knot has no M - has no partner:
    bare = R._with_G(s, R.P.thin_rows(s.G_row, s.G_col, s.G_val, lambda r, c: not ((r, c) in ((1, S), (S, 1)))))
    far = R._append(R._append(bare, S, (K - 1) * n + 1, 0.5), (K - 1) * n + 1, S, 0.5)
    with pytest.raises(ValueError, match=r"1 entries.*row %d, column %d, no entry at row 1, column %d" % (S, (K - 1) * n + 1, S)):
        kkt_solve_csr(*_args(far), cross=True, **KW)
    # and a state-row entry whose column lies in another knot and folds onto the slot is one
    folded = R._append(one, 1, n + S, 0.5)
    with pytest.raises(ValueError, match="GPU only"):
        kkt_solve_csr(*_args(folded), cross=True, **KW)
    # both triangles and upper-only storage pass the pattern check and stop at the device check: there is no CPU fallback
    for ok in (s, R.csr_upper(cell, R.csr_both)):
        with pytest.raises(ValueError, match="GPU only"):
            kkt_solve_csr(*_args(ok), cross=True, **KW)


def test_wrong_dtype_and_device_are_refused_on_the_host():
    from gato_python_amd.autograd import kkt_solve_csr
    s = R.csr_both(X.cell(2, 1, 3))
    a = list(_args(s))
    with pytest.raises(ValueError, match="GPU only"):
        kkt_solve_csr(*a, cross=True, **KW)
    bad = list(a)
    bad[1] = a[1].to(torch.float32)
    with pytest.raises(ValueError, match="G_col must be a 1-D int32 / int64 tensor"):
        kkt_solve_csr(*bad, cross=True, **KW)
    bad = list(a)
    bad[2] = a[2].numpy()
    with pytest.raises(ValueError, match="G_val must be a torch.Tensor"):
        kkt_solve_csr(*bad, cross=True, **KW)
    bad = list(a)
    bad[0] = a[0][:-1]
    with pytest.raises(ValueError, match="len\\(G_row\\)"):
        kkt_solve_csr(*bad, cross=True, **KW)
    with pytest.raises(ValueError):                                        # cross=False: the path it was
        kkt_solve_csr(*a, **KW)
