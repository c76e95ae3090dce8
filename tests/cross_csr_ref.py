"""numpy reference of the CSR entry to the cross solve, for the tests.

scatter() is the scatter rule as a loop over the entries in storage order: knot = row / n, in-knot column = col % n, the last
entry wins a slot, explicit zeros are values; a G entry of a state row in a control column lands in M_k for k < K-1 and is
dropped in the last knot; the mirror entries (control row, state column) are not read; rho is not added.  It returns the blocks
in the solver's layouts and, per entry, the slot that carries its gradient (-1: none) and its kind.

The oracle's two restatements of the scatter mishandle cross entries (csr_patterns.pattern_system's note), so this module is the
reference of every cross pattern and nothing here goes through oracle.convert.

The CSR builders work on the cells of cross_ref.batch_cells and cross_hard_cells.hard_cell: both triangles (what
synth.blocks_to_csr(M=...) emits), the state-row triangle only, the csr_patterns transformations on top, a cross entry in the
last knot's state rows, and a cross entry whose column lies in another knot."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cross_ref as X                             # noqa: E402
import csr_patterns as P                          # noqa: E402
from gato_python_amd import synth                 # noqa: E402

RHO = X.RHO
# kinds of a G entry: in M and kept; control row x state column (not read); in M but a later entry of its row won the slot; a
# cross entry of the last knot; a Q or R entry that lost its slot; a Q or R entry that is kept
KEPT, MIRROR, OVERWRITTEN, DROPPED, LOST, PLAIN = "kept_cross", "mirror", "overwritten_cross", "dropped_cross", "overwritten_plain", "plain"


def scatter(s):
    """The rule on a KKTSystem -> dict: G [G_dense] (without rho), M [(K-1) S C], C [C_dense] in the dtype of the values;
    slotG / slotM per G entry (index into G / M, -1 = not there), slotC per C entry; kind per G entry."""
    S, C, K = s.S, s.C, s.K
    n, SS, CC, SC = S + C, S * S, C * C, S * C
    Gd = np.zeros((SS + CC) * K - CC, s.G_val.dtype)
    Md = np.zeros((K - 1) * SC, s.G_val.dtype)
    Cd = np.zeros((SS + SC) * (K - 1), s.C_val.dtype)
    slotG, slotM = np.full(len(s.G_col), -1, np.int64), np.full(len(s.G_col), -1, np.int64)
    slotC = np.full(len(s.C_col), -1, np.int64)
    kind = np.full(len(s.G_col), PLAIN, object)
    for row in range(s.N):
        k, isr, owner = row // n, row % n, {}
        for e in range(s.G_row[row], s.G_row[row + 1]):
            isc = int(s.G_col[e]) % n
            if isr >= S and isc < S:
                kind[e] = MIRROR
                continue
            if isr < S and isc >= S:
                if k == K - 1:
                    kind[e] = DROPPED
                    continue
                key, kind[e] = ("M", k * SC + (isc - S) * S + isr), KEPT
            elif isc < S:
                key = ("G", k * (SS + CC) + isc * S + isr)
            else:
                key = ("G", k * (SS + CC) + SS + (isc - S) * C + (isr - S))
            if key in owner:                                                # the last entry in storage order wins
                slotG[owner[key]] = slotM[owner[key]] = -1
                kind[owner[key]] = OVERWRITTEN if key[0] == "M" else LOST
            owner[key] = e
            (slotM if key[0] == "M" else slotG)[e] = key[1]
            (Md if key[0] == "M" else Gd)[key[1]] = s.G_val[e]
    for row in range(S, S * K):
        br, owner = row // S - 1, {}
        for e in range(s.C_row[row], s.C_row[row + 1]):
            col = int(s.C_col[e])
            if col // n > br:
                continue
            d = br * (SS + SC) + (col % n) * S + row % S
            if d in owner:
                slotC[owner[d]] = -1
            owner[d] = e
            slotC[e] = d
            Cd[d] = s.C_val[e]
    return dict(G=Gd, M=Md, C=Cd, slotG=slotG, slotM=slotM, slotC=slotC, kind=kind)


def counts(sc):
    return {k: int((sc["kind"] == k).sum()) for k in (KEPT, MIRROR, OVERWRITTEN, DROPPED, LOST, PLAIN)}


def blocks_of(sc, s):
    """scatter()'s flat blocks as math-shaped (Q, R, A, B, M) in float64."""
    from oracle import gato_oracle as o
    S, C, K = s.S, s.C, s.K
    Q, R = o.unpack_G(np.asarray(sc["G"], np.float64), S, C, K)
    A, B = o.unpack_C(np.asarray(sc["C"], np.float64), S, C, K) if K > 1 else (np.zeros((0, S, S)), np.zeros((0, S, C)))
    return Q, R, A, B, X.unpack_M(np.asarray(sc["M"], np.float64), S, C, K)


def cell_of(sc, s):
    """(blocks, M) of the problem scatter() built, with the system's own g and c: what cross_ref.dense_solve takes."""
    S, C, K, n = s.S, s.C, s.K, s.S + s.C
    Q, R, A, B, M = blocks_of(sc, s)
    g = np.asarray(s.g, np.float64)
    q = np.stack([g[k * n:k * n + S] for k in range(K)])
    r = np.stack([g[k * n + S:(k + 1) * n] for k in range(K - 1)]) if K > 1 else np.zeros((0, C))
    return (Q, R, A, B, q, r, np.asarray(s.c, np.float64).reshape(K, S)), M


# ---- CSR builders ------------------------------------------------------------------------------------------------------------
def csr_both(cell):
    """Both triangles, as csr_matrix(dense) would emit them (zeros dropped; every diagonal entry of these cells is non-zero)."""
    blocks, M = cell
    return synth.blocks_to_csr(*blocks, rho=RHO, M=M)


def csr_full(cell):
    """Both triangles with every entry of every knot's (S + C) x (S + C) block stored, zeros included (explicit zeros are
    values): the cells of a batch, whose Q_k differ in sparsity, share this pattern.  C as synth.blocks_to_csr emits it."""
    blocks, M = cell
    Q, R = blocks[0], blocks[1]
    K, S, C = Q.shape[0], Q.shape[1], R.shape[-1]
    n = S + C
    s = synth.blocks_to_csr(*blocks, rho=RHO)
    ptr, idx, dat = [0], [], []
    for k in range(K):
        Gk = Q[k] if k == K - 1 else np.block([[Q[k], M[k]], [M[k].T, R[k]]])
        for i in range(Gk.shape[0]):
            idx += list(range(k * n, k * n + Gk.shape[1]))
            dat += Gk[i].tolist()
            ptr.append(len(idx))
    return _with_G(s, (np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(dat, np.float64)))


def _with_G(s, G):
    return synth.KKTSystem(s.S, s.C, s.K, *G, s.C_row, s.C_col, s.C_val, s.g, s.c, s.rho)


def csr_upper(cell, base=csr_full):
    """The state-row triangle only: the mirror entries (control row, state column) are not stored."""
    s = base(cell)
    n = s.S + s.C
    return _with_G(s, P.thin_rows(s.G_row, s.G_col, s.G_val, lambda r, c: not (r % n >= s.S and c % n < s.S)))


def csr_pattern(cell, name, base=csr_full, seed=0):
    """A csr_patterns transformation (shuffled with explicit zeros, duplicates, emptied rows, all three) on both triangles.  The
    draw depends on the shape, the seed and the pattern alone, so the cells of a batch get one set of index arrays."""
    s = base(cell)
    rng = np.random.default_rng([s.S, s.C, s.K, seed, sorted(P.PATTERNS).index(name)])
    G, Cc = P.PATTERNS[name](rng, s, (s.G_row, s.G_col, s.G_val.copy()), (s.C_row, s.C_col, s.C_val.copy()))
    return synth.KKTSystem(s.S, s.C, s.K, *G, *Cc, s.g, s.c, s.rho)


def _append(s, row, col, val):
    """One more entry at the end of a G row."""
    at = int(s.G_row[row + 1])
    ptr = s.G_row.copy()
    ptr[row + 1:] += 1
    return _with_G(s, (ptr, np.insert(s.G_col, at, col).astype(np.int32), np.insert(s.G_val, at, val)))


def csr_last_knot(cell, base=csr_full):
    """Both triangles plus a cross entry in the first and the last state row of the LAST knot (its column folds onto a control
    column of knot K-2): dropped, the last knot has no M.  K >= 2."""
    s = base(cell)
    n, K = s.S + s.C, s.K
    s = _append(s, (K - 1) * n, (K - 2) * n + s.S, 0.75)
    return _append(s, (K - 1) * n + s.S - 1, (K - 1) * n - 1, -1.25)


def csr_folded(cell, base=csr_full):
    """Both triangles plus, at the end of state row 1 % S of knot 0, an entry whose column is the last control column of knot 1:
    col % n folds it onto M_0[1 % S, C-1], which it wins as the last entry of its row.  K >= 3."""
    s = base(cell)
    assert s.K >= 3
    n = s.S + s.C
    return _append(s, 1 % s.S, 2 * n - 1, 0.3125)


BUILDERS = dict(both=lambda cell, base=csr_full: base(cell), upper=csr_upper, last_knot=csr_last_knot, folded=csr_folded,
                **{name: (lambda cell, base=csr_full, name=name: csr_pattern(cell, name, base)) for name in P.PATTERNS})
# what each pattern promises of counts() at K = 5 on every shape: kinds that must occur
PROMISES = dict(both=(KEPT, MIRROR), upper=(KEPT,), last_knot=(KEPT, MIRROR, DROPPED), folded=(KEPT, MIRROR, OVERWRITTEN),
                shuffled=(KEPT, MIRROR), duplicates=(KEPT, MIRROR, OVERWRITTEN, LOST), empty=(KEPT, MIRROR),
                combined=(KEPT, MIRROR, OVERWRITTEN, LOST))


def stacked(systems, dt):
    """The systems of one pattern (shared index arrays, checked) as host arrays: idx (int32 x 4), (G_val [B, nnz], C_val, g, c)."""
    s0 = systems[0]
    for s in systems[1:]:
        assert all(np.array_equal(a, b) for a, b in zip((s.G_row, s.G_col, s.C_row, s.C_col), (s0.G_row, s0.G_col, s0.C_row, s0.C_col)))
    idx = tuple(np.asarray(a, np.int32) for a in (s0.G_row, s0.G_col, s0.C_row, s0.C_col))
    return idx, tuple(np.stack([np.asarray(getattr(s, k), dt) for s in systems]) for k in ("G_val", "C_val", "g", "c"))
