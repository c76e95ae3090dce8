"""CSR patterns a caller may legally pass that scipy's csr_matrix(dense) never produces: rows in any column order with
structurally present zeros, rows that hold a column twice (the last entry in storage order wins its slot), and structurally
empty rows (repeated row pointers).  The three transformations are the ones tests/test_gpu_parity.py applies to the forward
scatter; pattern_system() builds named systems from them for the gradient sweep (tests/test_gpu_kkt_grad_sweep.py), whose
slot map tests/test_sweep_refs_cpu.py checks against the scatter on the CPU."""
import numpy as np

from gato_python_amd import synth


def _flat(ptr, idx, dat):
    return np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(dat, np.float64)


def shuffle_rows(rng, indptr, indices, data):
    """Every row in a random column order."""
    idx, dat, ptr = [], [], [0]
    for r in range(len(indptr) - 1):
        cols = list(indices[indptr[r]:indptr[r + 1]]); vals = list(data[indptr[r]:indptr[r + 1]])
        perm = rng.permutation(len(cols))
        idx += [cols[i] for i in perm]; dat += [vals[i] for i in perm]
        ptr.append(len(idx))
    return _flat(ptr, idx, dat)


def thin_rows(indptr, indices, data, keep):
    """Only the entries with keep(row, column): rows may end up with one entry or none."""
    idx, dat, ptr = [], [], [0]
    for r in range(len(indptr) - 1):
        for e in range(indptr[r], indptr[r + 1]):
            if keep(r, int(indices[e])):
                idx.append(indices[e]); dat.append(data[e])
        ptr.append(len(idx))
    return _flat(ptr, idx, dat)


def with_duplicates(rng, indptr, indices, data, frac):
    """A share `frac` of the non-empty rows gets 1..3 extra entries: copies of columns the row already holds, with values of
    their own, anywhere in the row - before or after the original, next to it or far from it."""
    idx, dat, ptr = [], [], [0]
    for r in range(len(indptr) - 1):
        cols = list(indices[indptr[r]:indptr[r + 1]]); vals = list(data[indptr[r]:indptr[r + 1]])
        if cols and rng.random() < frac:
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(0, len(cols)))
                at = int(rng.integers(0, len(cols) + 1))
                cols.insert(at, cols[j]); vals.insert(at, float(rng.standard_normal()))
        idx += cols; dat += vals
        ptr.append(len(idx))
    return _flat(ptr, idx, dat)


# ---- named patterns on synth.make_system(S, C, K, dense_q=True) -------------------------------------------------------------
def _shuffled(rng, s, G, Cc):
    G, Cc = shuffle_rows(rng, *G), shuffle_rows(rng, *Cc)
    G[2][rng.random(len(G[2])) < 0.1] = 0.0                     # explicit zeros are just values
    Cc[2][rng.random(len(Cc[2])) < 0.1] = 0.0
    return G, Cc


def _duplicated(rng, s, G, Cc):
    """(C's block row 0 stays as it is: kkt_solve_csr reads S off its leading one-entry rows.)"""
    ptr, idx, dat = Cc
    at = ptr[s.S]
    p2, i2, d2 = with_duplicates(rng, ptr[s.S:] - at, idx[at:], dat[at:], 0.4)
    Cc = _flat(np.concatenate([ptr[:s.S], p2 + at]), np.concatenate([idx[:at], i2]), np.concatenate([dat[:at], d2]))
    return with_duplicates(rng, *G, 0.4), Cc


def _emptied(rng, s, G, Cc):
    """G: a fifth of the rows thinned down to their diagonal (symmetrically).  C: the first row of block row 1 and the last row
    of all with no entry at all, their neighbours with the identity entry only, and a sixth of the other rows one or the other."""
    S, K, n = s.S, s.K, s.S + s.C
    diag_only = set(int(r) for r in rng.choice(s.N, max(2, s.N // 5), replace=False))
    G = thin_rows(*G, lambda r, c: r == c or (r not in diag_only and c not in diag_only))
    rows = np.arange(S, S * K)
    gone, bare = {S, S * K - 1}, {S + 1, S * K - 2}
    for r in rng.choice(rows, max(2, len(rows) // 6), replace=False):
        if int(r) not in gone and int(r) not in bare:
            (gone if rng.random() < 0.5 else bare).add(int(r))

    def keep_c(r, c):
        if r in gone:
            return False
        return c == (r // S) * n + r % S if r in bare else True   # (the identity entry of row r: x_k+1 of block row k + 1)
    return G, thin_rows(*Cc, keep_c)


def _combined(rng, s, G, Cc):
    G, Cc = _emptied(rng, s, G, Cc)
    G, Cc = _duplicated(rng, s, G, Cc)
    return _shuffled(rng, s, G, Cc)


PATTERNS = dict(shuffled=_shuffled, duplicates=_duplicated, empty=_emptied, combined=_combined)


def pattern_system(name, S, C, K, seed=0):
    """The dense-Q system of `seed` through the transformation `name`.  (G entries between the Q and R parts - a state row with
    a control column - are not among the patterns: make_system has none, and the scatter's two restatements treat such an entry
    differently from the device, so no reference could carry one.)"""
    s = synth.make_system(S, C, K, seed=seed, dense_q=True)
    rng = np.random.default_rng([S, C, K, seed, sorted(PATTERNS).index(name)])
    G, Cc = PATTERNS[name](rng, s, (s.G_row, s.G_col, s.G_val.copy()), (s.C_row, s.C_col, s.C_val.copy()))
    return synth.KKTSystem(S, C, K, *G, *Cc, s.g, s.c, s.rho)


def kinds(s, slotG, slotC):
    """Counts of the entry kinds of a pattern under its slot map (kkt_grad_ref.csr_slot_map)."""
    S, n = s.S, s.S + s.C
    rowC = np.repeat(np.arange(S * s.K), np.diff(s.C_row))
    state_row = np.arange(s.N) % n < S
    ident = (rowC >= S) & (s.C_col // n > rowC // S - 1)
    return dict(block_row_0=int((rowC < S).sum()), identity=int(ident.sum()),
                overwritten_G=int((slotG < 0).sum()),              # (no G entry of these patterns lies outside every block)
                overwritten_C=int(((slotC < 0) & (rowC >= S) & ~ident).sum()),
                empty_G_rows=int((np.diff(s.G_row) == 0).sum()),
                diagonal_only_G_rows=int(((np.diff(s.G_row) == 1) & state_row).sum()),
                empty_C_rows=int((np.diff(s.C_row) == 0).sum()), identity_only_C_rows=int((np.diff(s.C_row)[S:] == 1).sum()),
                kept_G=int((slotG >= 0).sum()), kept_C=int((slotC >= 0).sum()))
