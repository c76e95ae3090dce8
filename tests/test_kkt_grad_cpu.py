"""CPU suite: the numpy reference of the KKT-solve gradients (tests/kkt_grad_ref.py) against central finite differences of
the dense solve, the CSR slot map against the scatter's rules, and the input checks of gato_python_amd.autograd."""
import os

import numpy as np
import pytest
import torch

import kkt_grad_ref as ref
from gato_python_amd import synth


def loss(s, w1, w2):
    dz, lam = synth.dense_kkt_solve(s)
    return float(w1 @ dz + w2 @ lam)


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def fd_check(s, seed, n_dirs=3):
    """Random directions, symmetric in Q / R, over every block: <grad, D> against the central difference of the dense solve."""
    rng = np.random.default_rng(seed)
    w1, w2 = rng.standard_normal(s.N), rng.standard_normal(s.S * s.K)
    gr = ref.dense_reference(s, w1, w2)
    blocks = ref.blocks_of(s)
    names = ("Q", "R", "A", "B", "q", "r", "c")
    for _ in range(n_dirs):
        D = [rng.standard_normal(b.shape) for b in blocks]
        D[0], D[1] = sym(D[0]), sym(D[1])
        D[6][0] = rng.standard_normal(s.S)
        eps = 1e-6
        at = lambda t: synth.blocks_to_csr(*[b + t * d for b, d in zip(blocks, D)], rho=s.rho, dense_q=True)
        fd = (loss(at(eps), w1, w2) - loss(at(-eps), w1, w2)) / (2 * eps)
        an = sum(float(np.sum(gr[nm] * d)) for nm, d in zip(names, D))
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (fd, an)
    return gr


def test_reference_against_finite_differences_pendulum():
    fd_check(synth.pendulum_system(), 0)


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_against_finite_differences_iiwa_14_7_8(seed):
    fd_check(synth.make_system(14, 7, 8, seed=seed), 10 + seed)


def test_reference_against_finite_differences_dense_q_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, "s32_c16_k12_seed5_denseq.npz"))
    s = synth.make_system(32, 16, 12, seed=5, dense_q=True)
    dz, lam = synth.dense_kkt_solve(s)
    assert np.abs(lam - gold["dense_lam"]).max() <= 1e-9 * np.abs(gold["dense_lam"]).max()     # the fixture's system
    fd_check(s, 7, n_dirs=2)


def test_q_and_r_gradients_are_symmetric():
    s = synth.make_system(14, 7, 6, seed=3)
    rng = np.random.default_rng(0)
    gr = ref.dense_reference(s, rng.standard_normal(s.N), rng.standard_normal(s.S * s.K))
    assert np.array_equal(gr["Q"], np.swapaxes(gr["Q"], 1, 2)) and np.array_equal(gr["R"], np.swapaxes(gr["R"], 1, 2))


# ---- the CSR slot map: the chain rule through oracle.convert's scatter --------------------------------------------------
def convert_loss(G_row, G_col, G_val, C_row, C_col, C_val, g, c, S, C, K, rho, w1, w2):
    """L of the system the scatter builds (identity blocks of C implied, as the solver assumes)."""
    M, rhs = ref.scatter_kkt(synth.KKTSystem(S, C, K, G_row, G_col, G_val, C_row, C_col, C_val, g, c, rho))
    x = np.linalg.solve(M, rhs)
    N = (S + C) * K - C
    return float(w1 @ x[:N] + w2 @ x[N:]), x[:N], x[N:], M


def odd_pendulum():
    """The pendulum with a duplicated G column (the first entry loses), an unsorted C row holding an explicit zero (B_0's
    entry) and the identity entry first, and a C row with a duplicated column."""
    p = synth.pendulum_system()
    G_rows = [list(zip(p.G_col[p.G_row[i]:p.G_row[i + 1]], p.G_val[p.G_row[i]:p.G_row[i + 1]])) for i in range(p.N)]
    C_rows = [list(zip(p.C_col[p.C_row[i]:p.C_row[i + 1]], p.C_val[p.C_row[i]:p.C_row[i + 1]])) for i in range(p.S * p.K)]
    G_rows[0] = [(0, 5.0)] + G_rows[0]                         # same column twice: the later entry (1.0) wins
    G_rows[3] = G_rows[3] + [(3, 2.0)]                         # the later entry (2.0) wins
    C_rows[2] = [(3, 1.0), (1, -0.1), (2, 0.0), (0, -1.0)]     # unsorted, explicit zero on u_0, identity first
    C_rows[3] = C_rows[3] + [(1, -1.0)]                        # column 1 again: the later entry wins
    flat = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
                         np.array([c for r in rows for c, _ in r], np.int32), np.array([v for r in rows for _, v in r]))
    G_row, G_col, G_val = flat(G_rows)
    C_row, C_col, C_val = flat(C_rows)
    return synth.KKTSystem(p.S, p.C, p.K, G_row, G_col, G_val, C_row, C_col, C_val, p.g.copy(), p.c.copy() + 0.1, p.rho)


def test_slot_map_rules():
    s = odd_pendulum()
    sg, sc = ref.csr_slot_map(s.G_row, s.G_col, s.C_row, s.C_col, s.S, s.C, s.K)
    assert sg[0] == -1 and sg[1] == 0                          # duplicate: the first entry is overwritten
    assert sc[0] == -1 and sc[1] == -1                         # block row 0 of C: the identity rows
    r2 = slice(s.C_row[2], s.C_row[3])
    assert list(sc[r2][[0]]) == [-1] and np.all(sc[r2][1:] >= 0)   # identity on x_1 dropped, the explicit zero kept
    r3 = np.arange(s.C_row[3], s.C_row[4])
    cols3 = s.C_col[r3]
    first1 = r3[list(cols3).index(1)]
    assert sc[first1] == -1 and sc[r3[-1]] >= 0
    # every identity entry of C (column of x_k+1 in block row k+1, or block row 0) maps to -1
    n = s.S + s.C
    for row in range(s.S * s.K):
        for it in range(s.C_row[row], s.C_row[row + 1]):
            if row < s.S or s.C_col[it] // n > row // s.S - 1:
                assert sc[it] == -1


def test_slot_map_gradients_against_finite_differences_of_the_scatter():
    """Each CSR value perturbed on its own through oracle.convert: the gradient of the dense slot it is written into, 0 for
    a dropped or overwritten entry (diagonal G here, so the symmetric Q gradient is the exact one)."""
    s = odd_pendulum()
    S, C, K = s.S, s.C, s.K
    rng = np.random.default_rng(4)
    w1, w2 = rng.standard_normal(s.N), rng.standard_normal(S * K)
    args = [s.G_row, s.G_col, s.G_val, s.C_row, s.C_col, s.C_val, s.g, s.c, S, C, K, s.rho, w1, w2]
    _, dz, lam, M = convert_loss(*args)
    y = np.linalg.solve(M.T, np.concatenate([w1, w2]))
    Gd, Cd = ref.grads_dense_layout(dz, lam, y[:s.N], y[s.N:], S, C, K)
    sg, sc = ref.csr_slot_map(s.G_row, s.G_col, s.C_row, s.C_col, S, C, K)
    an_G, an_C = ref.gather(Gd, sg), ref.gather(Cd, sc)
    for which, vals, an in ((2, s.G_val, an_G), (5, s.C_val, an_C)):
        for it in range(len(vals)):
            hi, lo = [a.copy() if isinstance(a, np.ndarray) else a for a in args], [a.copy() if isinstance(a, np.ndarray) else a for a in args]
            h = 1e-4 * max(abs(vals[it]), 1e-2)       # step relative to the value (R entries are 0.1, the terminal Q 100)
            hi[which][it] += h
            lo[which][it] -= h
            fd = (convert_loss(*hi)[0] - convert_loss(*lo)[0]) / (2 * h)
            assert abs(fd - an[it]) <= 5e-6 * max(abs(an[it]), 1.0), (which, it, fd, an[it])
    assert an_G[0] == 0 and an_C[s.C_row[2]] == 0 and an_C[s.C_row[2] + 2] != 0      # overwritten, identity, explicit zero


# ---- input checks: ValueError before any library call -----------------------------------------------------------------
def blocks_cpu(S=2, C=1, K=5, dt=torch.float64):
    return [torch.from_numpy(np.ascontiguousarray(b)).to(dt) for b in synth.make_blocks(S, C, K, seed=0)]


def test_kkt_solve_refuses_cpu_tensors():
    from gato_python_amd import kkt_solve
    with pytest.raises(ValueError, match="no CPU fallback"):
        kkt_solve(*blocks_cpu(), rho=1e-3, exit_tol=1e-10, max_iters=100)


@pytest.mark.parametrize("bad", ["R", "A", "B", "q", "r", "c", "Q"])
def test_kkt_solve_refuses_bad_shapes(bad):
    from gato_python_amd import kkt_solve
    args = dict(zip("Q R A B q r c".split(), blocks_cpu()))
    args[bad] = args[bad][..., :-1] if bad != "c" else args[bad][:-1]
    with pytest.raises(ValueError):
        kkt_solve(*args.values(), rho=1e-3, exit_tol=1e-10, max_iters=100)


def test_kkt_solve_refuses_non_tensors():
    from gato_python_amd import kkt_solve
    args = blocks_cpu()
    args[4] = args[4].numpy()
    with pytest.raises(ValueError, match="torch.Tensor"):
        kkt_solve(*args, rho=1e-3, exit_tol=1e-10, max_iters=100)


def csr_cpu(dt=torch.float64):
    p = synth.pendulum_system()
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    i = torch.int32
    return [t(p.G_row, i), t(p.G_col, i), t(p.G_val, dt), t(p.C_row, i), t(p.C_col, i), t(p.C_val, dt), t(p.g, dt), t(p.c, dt)]


def test_kkt_solve_csr_refuses_cpu_tensors():
    from gato_python_amd import kkt_solve_csr
    with pytest.raises(ValueError, match="no CPU fallback"):
        kkt_solve_csr(*csr_cpu(), rho=1e-3, exit_tol=1e-10, max_iters=100)


def test_kkt_solve_csr_refuses_bad_shapes():
    from gato_python_amd import kkt_solve_csr
    a = csr_cpu()
    a[6] = torch.stack([a[6], a[6]])                           # batched g beside unbatched values
    with pytest.raises(ValueError, match="1-D or all"):
        kkt_solve_csr(*a, rho=1e-3, exit_tol=1e-10, max_iters=100)
    a = csr_cpu()
    a[2], a[5], a[6], a[7] = (torch.stack([x, x, x]) for x in (a[2], a[5], a[6], a[7]))
    a[7] = a[7][:2]
    with pytest.raises(ValueError, match="batch sizes differ"):
        kkt_solve_csr(*a, rho=1e-3, exit_tol=1e-10, max_iters=100)
