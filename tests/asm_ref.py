"""Assembly and dz against a reference from the DEFINITIONS, on dense, graded inputs (tests/test_asm_ref_cpu.py,
tests/test_gpu_asm_ref.py, tools/asm_accuracy.py).

The oracle (oracle/) restates the reference's elimination knot by knot, so agreeing with it shows sameness.  This module has no
per-knot recurrence and no Gauss-Jordan: from the CSR inputs it builds dense G + rho I and C as synth.dense_kkt does and computes,
in np.longdouble,
    Ginv = G^-1 (per diagonal block),  S = -C Ginv C^T,  gamma = c - C Ginv g,
    D = blockdiag(S),  Pinv = D^-1 - D^-1 (S - D) D^-1   (the symmetric stair: exactly block tridiagonal),
    dz = Ginv (g - C^T lambda),
with every inverse np.linalg.inv in fp64 followed by three Newton steps X <- X (2I - M X) in longdouble, and extracts the blocks
in the device layouts (column-major, [K][3][S*S] left / main / right, Ginv as Q_0^-1, R_0^-1, ...).  For an fp32 run the
reference is that of the fp32-rounded inputs and the fp32-rounded rho: what an fp32 run really solves.

Inputs: hard_blocks - dense SPD Q_k and R_k of a given condition, every block on its own power-of-two scale, A_k far from the
identity, c_0 != 0 - everything synth.make_blocks leaves out (diagonal R_k, A_k = -(I + 1 % noise), c_0 = 0, O(1) scales).

Yardstick: per block (one knot, one slot; a gamma / dz block is one knot's entries) e = max|got - truth| / max|truth|, a buffer's
e the maximum over its blocks, blocks that are structurally zero exactly zero; the bar is
    e_gpu <= FACTOR * max(e_C_oracle, e_numpy_oracle) + FLOOR_EPS eps
with the two oracles run in the same dtype on the same inputs (the project's "beside the reference's own error, held to the worse
of two CPU orders", f32_parity.check_f32, here in fp64 too).  Factor and floor: over all six shapes, K in {1, 2, 3, 5}, three
seeds, both dtypes, each CPU order judged against the other never passed 4 x + 16 eps in 2 880 comparisons (raw ratios reach 7
where both errors are a few eps: that is what the floor is for); 2 x + 42 eps was passed once."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gato_python_amd import synth                 # noqa: E402
from oracle import c_oracle as co                 # noqa: E402
from oracle import gato_oracle as o               # noqa: E402

LD = np.longdouble
FACTOR, FLOOR_EPS = 4.0, 16.0
COND, RHO = 100.0, 1e-3
GRADE = {"float64": 4, "float32": 3}
SHAPES = ((2, 1), (4, 2), (6, 3), (12, 6), (14, 7), (32, 16))
KNOTS = (1, 2, 3, 5)                              # first knot only; k == 1; first Schur-block neighbour; a last knot behind full knots
DTYPES = ("float64", "float32")
STAGE_BUFFERS = ("Ginv", "S", "Pinv_bj", "gamma", "Pinv", "dz")
WHOLE_BUFFERS = ("Ginv", "S", "Pinv", "gamma")
BLOCKS_CASES = ((6, 3, 3), (14, 7, 5), (32, 16, 3))
BATCH_CASES = ((2, 1, 5), (14, 7, 3), (32, 16, 2))
BATCH = 3
LONG = (2, 1, 16400)                              # past the 8192-workgroup cap of the Schur / stair / dz launches twice, the inversion launch's once
LONG_WINDOWS = (8190, 16382, 16390)               # ten knots from each: around both wraps of the grid, and the end
# the fp64 whole solve: exit test |r . Pinv r| < EXIT_TOL, at most MAX_ITERS iterations (tests/test_asm_ref_cpu.py asserts that the
# C oracle's solve with them is within a tenth of BASELINE's bar on every case)
EXIT_TOL, MAX_ITERS = 1e-22, 400


def eps_of(dt):
    return float(np.finfo(np.dtype(dt)).eps)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _haar(rng, shape):
    """Haar-distributed orthogonal matrices [..., n, n]: QR of a Gaussian, the signs of R's diagonal fixed."""
    Qm, Rm = np.linalg.qr(rng.standard_normal(shape))
    d = np.sign(np.diagonal(Rm, axis1=-2, axis2=-1))
    d = np.where(d == 0, 1.0, d)
    return Qm * d[..., None, :]


def _spd(rng, m, n, cond, grade):
    """m dense SPD n x n blocks U diag(ev) U^T: ev log-uniform in [1, cond] with both ends present, each block times its own 2^e,
    e uniform in [-grade, grade]."""
    U = _haar(rng, (m, n, n))
    ev = cond ** rng.uniform(0.0, 1.0, (m, n))
    ev[:, 0] = 1.0
    if n > 1:
        ev[:, -1] = cond
    e = rng.integers(-grade, grade + 1, m)
    M = (U * ev[:, None, :]) @ U.transpose(0, 2, 1)
    M = 0.5 * (M + M.transpose(0, 2, 1))
    return M * (2.0 ** e)[:, None, None]


def hard_blocks(S, C, K, seed, cond=COND, grade=0):
    """Q[K,S,S], R[K-1,C,C], A[K-1,S,S], B[K-1,S,C], q[K,S], r[K-1,C], c[K,S] (fp64; synth.make_blocks' order), drawn in this
    order from default_rng([seed, S, C, K]).  A_k = U1 diag(uniform(0.5, 1.5)) U2: condition at most 3, nowhere near the identity;
    B_k Gaussian / sqrt(C); q, r, c Gaussian, c_0 included."""
    rng = np.random.default_rng([seed, S, C, K])
    Q = _spd(rng, K, S, cond, grade)
    R = _spd(rng, K - 1, C, cond, grade)
    U1, U2 = _haar(rng, (K - 1, S, S)), _haar(rng, (K - 1, S, S))
    A = (U1 * rng.uniform(0.5, 1.5, (K - 1, S))[:, None, :]) @ U2
    B = rng.standard_normal((K - 1, S, C)) / np.sqrt(C)
    q = rng.standard_normal((K, S))
    r = rng.standard_normal((K - 1, C))
    c = rng.standard_normal((K, S))
    return Q, R, A, B, q, r, c


def to_system(blocks, rho=RHO):
    return synth.blocks_to_csr(*blocks, rho=rho, dense_q=True)


def window(blocks, w0, w1):
    """The blocks of knots [w0, w1) alone, and the knots [lo, hi) of the whole horizon whose every S, Pinv, gamma and dz block the
    window's reference reproduces: the window's first knot plays x_0 and its last has no R, A, B, so all but the two knots behind
    a cut front and the two before a cut end."""
    Q, R, A, B, q, r, c = blocks
    K = Q.shape[0]
    sub = (Q[w0:w1], R[w0:w1 - 1], A[w0:w1 - 1], B[w0:w1 - 1], q[w0:w1], r[w0:w1 - 1], c[w0:w1])
    return sub, (w0 + 2 if w0 > 0 else 0), (w1 - 2 if w1 < K else K)


def pack_C(A, B):
    """C_dense: per knot k < K-1 [A_k (S*S col-major) | B_k (S*C col-major)]."""
    Km1, S, C = B.shape
    out = np.zeros((S * S + S * C) * Km1, A.dtype)
    st = S * S + S * C
    for k in range(Km1):
        out[k * st: k * st + S * S] = A[k].T.reshape(-1)
        out[k * st + S * S: (k + 1) * st] = B[k].T.reshape(-1)
    return out


def expected_dense(blocks, rho, dt):
    """What convert must give bit for bit: the generator's blocks rounded to dt, rho added to the diagonals in dt."""
    dt = np.dtype(dt)
    Q, R, A, B = (np.asarray(m, dt) for m in blocks[:4])
    Q, R = Q.copy(), R.copy()
    S, C = Q.shape[1], R.shape[1]
    Q[:, np.arange(S), np.arange(S)] += dt.type(rho)
    R[:, np.arange(C), np.arange(C)] += dt.type(rho)
    return o.pack_G(Q, R), pack_C(A, B)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def inv_ld(M):
    """M^-1 in longdouble: np.linalg.inv in fp64, then three Newton steps X <- X (2I - M X)."""
    M = np.asarray(M, LD)
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    I2 = 2 * np.eye(M.shape[0], dtype=LD)
    for _ in range(3):
        X = X @ (I2 - M @ X)
    return X


def solve_ld(M, b):
    """M^-1 b in longdouble: an fp64 solve refined three times on the longdouble residual."""
    M, b = np.asarray(M, LD), np.asarray(b, LD)
    M64 = M.astype(np.float64)
    x = np.linalg.solve(M64, b.astype(np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(M64, (b - M @ x).astype(np.float64)).astype(LD)
    return x


class Reference:
    """The longdouble reference of one system as run in dtype dt.  Buffers (flat, device layouts): buf["Ginv"], ["S"], ["Pinv_bj"]
    (block-Jacobi: main blocks only), ["Pinv"] (stair), ["gamma"]; dz(lam); lam_kkt, dz_kkt the dense KKT solution."""

    def __init__(self, s, dt):
        dt = np.dtype(dt)
        S, C, K = s.S, s.C, s.K
        n, N, SK = S + C, s.N, S * K
        sr = s.astype(dt).astype(np.float64)                      # the inputs the run really has
        rho = LD(dt.type(s.rho))
        Kd, rhs = synth.dense_kkt(sr, with_rho=False)
        G = Kd[:N, :N].astype(LD) + rho * np.eye(N, dtype=LD)
        Cm = Kd[N:, :N].astype(LD)
        g, c = rhs[:N].astype(LD), rhs[N:].astype(LD)
        Ginv = np.zeros((N, N), LD)
        Qi, Ri = np.zeros((K, S, S), LD), np.zeros((max(K - 1, 0), C, C), LD)
        for k in range(K):
            a = k * n
            Qi[k] = Ginv[a:a + S, a:a + S] = inv_ld(G[a:a + S, a:a + S])
            if k < K - 1:
                Ri[k] = Ginv[a + S:a + n, a + S:a + n] = inv_ld(G[a + S:a + n, a + S:a + n])
        Sd = -(Cm @ Ginv @ Cm.T)
        gamma = c - Cm @ (Ginv @ g)
        Dinv = np.zeros((SK, SK), LD)
        for k in range(K):
            b = slice(k * S, (k + 1) * S)
            Dinv[b, b] = inv_ld(Sd[b, b])
        D = np.zeros((SK, SK), LD)
        for k in range(K):
            b = slice(k * S, (k + 1) * S)
            D[b, b] = Sd[b, b]
        Pd = Dinv - Dinv @ (Sd - D) @ Dinv
        self.S_, self.C_, self.K, self.dt = S, C, K, dt
        self.G, self.Cm, self.g, self.c, self.Ginv_dense, self.S_dense, self.P_dense = G, Cm, g, c, Ginv, Sd, Pd
        Sl, Sm, Sr = self._tri(Sd)
        Pl, Pm, Pr = self._tri(Pd)
        Z = np.zeros_like(Pm)
        self.buf = dict(Ginv=o.pack_G(Qi, Ri), S=o.pack_bd(Sl, Sm, Sr), Pinv_bj=o.pack_bd(Z, Pm, Z), Pinv=o.pack_bd(Pl, Pm, Pr),
                        gamma=gamma.copy())
        self.lam_kkt = solve_ld(Sd, gamma)
        self.dz_kkt = self.dz(self.lam_kkt)

    def _tri(self, M):
        S, K = self.S_, self.K
        L, Mn, R = (np.zeros((K, S, S), LD) for _ in range(3))
        for k in range(K):
            b = slice(k * S, (k + 1) * S)
            Mn[k] = M[b, b]
            if k > 0:
                L[k] = M[b, (k - 1) * S:k * S]
            if k < K - 1:
                R[k] = M[b, (k + 1) * S:(k + 2) * S]
        return L, Mn, R

    def off_band(self):
        """max |entry| of S and of Pinv outside the three block diagonals (both are exactly block tridiagonal: 0)."""
        S, K = self.S_, self.K
        kb = np.arange(S * K) // S
        out = np.abs(kb[:, None] - kb[None, :]) > 1
        return float(np.abs(self.S_dense[out]).max(initial=0)), float(np.abs(self.P_dense[out]).max(initial=0))

    def cond_main(self):
        """Largest 2-norm condition number of a main block of S."""
        S, K = self.S_, self.K
        return max(float(np.linalg.cond(self.S_dense[k * S:(k + 1) * S, k * S:(k + 1) * S].astype(np.float64))) for k in range(K))

    def dz(self, lam):
        return self.Ginv_dense @ (self.g - self.Cm.T @ np.asarray(lam, LD))

    def rounded(self, name):
        return self.buf[name].astype(self.dt)


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def block_slices(name, S, C, K):
    """[(knot, start, stop)] of the blocks of a flat buffer."""
    if name in ("Ginv", "G_dense"):
        st, out = S * S + C * C, []
        for k in range(K):
            out.append((k, k * st, k * st + S * S))
            if k < K - 1:
                out.append((k, k * st + S * S, (k + 1) * st))
        return out
    if name in ("S", "Pinv", "Pinv_bj"):
        return [(i // 3, i * S * S, (i + 1) * S * S) for i in range(3 * K)]
    if name == "gamma":
        return [(k, k * S, (k + 1) * S) for k in range(K)]
    if name == "dz":
        n = S + C
        return [(k, k * n, k * n + (n if k < K - 1 else S)) for k in range(K)]
    raise KeyError(name)


def knot_slice(name, buf, S, C, K, w0, w1):
    """The part of a whole-horizon buffer that holds knots [w0, w1), in the layout of a horizon of w1 - w0 knots."""
    sl = block_slices(name, S, C, K)
    a = min(b for k, b, _ in sl if k == w0)
    e = max(t for k, _, t in sl if k == w1 - 1)
    if name in ("Ginv", "G_dense") and w1 < K:
        e -= C * C                                               # the window's last knot has no R
    if name == "dz" and w1 < K:
        e -= C
    return buf[a:e]


def block_error(name, got, truth, S, C, K, knots=None):
    """e of one buffer: max over its blocks (of the knots given) of max|got - truth| / max|truth|; inf if a block whose truth is
    all zero - structurally zero - holds anything but zeros, or if got is not finite."""
    got, truth = np.asarray(got), np.asarray(truth, LD)
    assert got.shape == truth.shape, (name, got.shape, truth.shape)
    worst = 0.0
    for k, a, b in block_slices(name, S, C, K):
        if knots is not None and k not in knots:
            continue
        t, x = truth[a:b], got[a:b]
        if not np.all(np.isfinite(x)):
            return float("inf")
        m = np.abs(t).max()
        if m == 0:
            if np.any(x != 0):
                return float("inf")
            continue
        worst = max(worst, float(np.abs(x.astype(LD) - t).max() / m))
    return worst


def bar(e_oracles, dt, factor=FACTOR):
    """The most a device buffer may be off: factor x the worse of the CPU orders' own errors + the floor."""
    return factor * max(e_oracles) + FLOOR_EPS * eps_of(dt)


def errors(bufs, truth, S, C, K, names, knots=None):
    return {n: block_error(n, bufs[n], truth[n], S, C, K, knots) for n in names}


def judge(what, dt, e_dev, e_oracles, names=None, factor=FACTOR):
    """Print every buffer's errors in eps (device beside each CPU order) and return the list of those past the bar."""
    eps = eps_of(dt)
    bad = []
    for n in (names or e_dev):
        eo = [e[n] for e in e_oracles]
        lim = bar(eo, dt, factor)
        ratio = e_dev[n] / max(max(eo), FLOOR_EPS * eps)
        print(f"{what} {n}: device {e_dev[n] / eps:.1f} eps, CPU orders {', '.join('%.1f' % (x / eps) for x in eo)} eps, "
              f"bar {lim / eps:.1f} eps, ratio {ratio:.2f}")
        if not e_dev[n] <= lim:
            bad.append((n, e_dev[n] / eps, [x / eps for x in eo]))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# cases and their runners (a backend is the C oracle, the numpy oracle or the device: arrays in, arrays out)
# ---------------------------------------------------------------------------------------------------------------------------
def case_id(S, C, K, dt, seed=0):
    return f"{S}-{C}-{K}-{dt}" + (f"-s{seed}" if seed else "")


def stage_cases():
    return [(S, C, K, dt) for (S, C) in SHAPES for K in KNOTS for dt in DTYPES]


def all_system_keys():
    """(S, C, K, dt, seed) of every system the GPU suite builds a dense reference for."""
    keys = [(S, C, K, dt, 0) for (S, C, K, dt) in stage_cases()]
    keys += [(S, C, K, dt, b) for (S, C, K) in BATCH_CASES for dt in DTYPES for b in range(1, BATCH)]
    return keys


@functools.lru_cache(maxsize=None)
def blocks_of(S, C, K, dt, seed=0):
    return hard_blocks(S, C, K, seed, COND, GRADE[dt])


@functools.lru_cache(maxsize=None)
def system_of(S, C, K, dt, seed=0):
    return to_system(blocks_of(S, C, K, dt, seed))


@functools.lru_cache(maxsize=None)
def reference_of(S, C, K, dt, seed=0):
    return Reference(system_of(S, C, K, dt, seed), dt)


def random_lambda(S, K, dt, seed=0):
    return np.random.default_rng([77, seed, S, K]).standard_normal(S * K).astype(dt)


class OracleBackend:
    """mod: oracle.c_oracle or oracle.gato_oracle."""

    def __init__(self, mod):
        self.mod = mod

    def convert(self, s, dt):
        return self.mod.convert(*s.csr_args()[:6], s.S, s.C, s.K, s.rho, np.dtype(dt).type)

    def form_schur(self, s, Gd, Cd, g, c):
        return self.mod.form_schur(Gd, Cd, g, c, s.S, s.C, s.K)

    def form_ss(self, s, Sb, Pb):
        return self.mod.form_ss(Sb, Pb, s.S, s.K)

    def compute_dz(self, s, Gi, Cd, g, lam):
        return self.mod.compute_dz(Gi, Cd, g, lam, s.S, s.C, s.K)


class DeviceBackend:
    """The stage entries of a Solver (gato_convert, gato_form_schur with its own inversions, gato_form_ss, gato_compute_dz)."""

    def __init__(self, sol):
        self.sol = sol

    @staticmethod
    def _h(t):
        return t.detach().cpu().numpy()

    def convert(self, s, dt):
        dev = self.sol.upload_system(s)
        Gd, Cd = self.sol.convert(*dev[:6], s.rho)
        return self._h(Gd), self._h(Cd)

    def form_schur(self, s, Gd, Cd, g, c):
        t = self.sol.to_device
        return tuple(self._h(x) for x in self.sol.form_schur(t(Gd), t(Cd) if s.K > 1 else self.sol.new(1), t(g), t(c)))

    def form_ss(self, s, Sb, Pb):
        return self._h(self.sol.form_ss(self.sol.to_device(Sb), self.sol.to_device(Pb)))

    def compute_dz(self, s, Gi, Cd, g, lam):
        t = self.sol.to_device
        return self._h(self.sol.compute_dz(t(Gi), t(Cd) if s.K > 1 else self.sol.new(1), t(g), t(lam)))


def isolated_stages(be, s, dt, feed, lam):
    """Every stage on its own: convert; form_schur on convert's blocks; form_ss and compute_dz on feed - the rounded reference
    outputs of the stage before them (feed["S"], ["Pinv_bj"], ["Ginv"]) - and the given lambda.  -> dict of flat buffers."""
    dt = np.dtype(dt)
    g, c = s.g.astype(dt), s.c.astype(dt)
    Gd, Cd = be.convert(s, dt)
    Sb, Pb, gam, Gi = be.form_schur(s, Gd, Cd, g, c)
    P2 = be.form_ss(s, feed["S"], feed["Pinv_bj"])
    dz = be.compute_dz(s, feed["Ginv"], Cd, g, lam)
    return dict(G_dense=Gd, C_dense=Cd, Ginv=Gi, S=Sb, Pinv_bj=Pb, gamma=gam, Pinv=P2, dz=dz)


def chained_stages(be, s, dt):
    """The assembly as a whole call runs it: every stage on the outputs of the one before."""
    dt = np.dtype(dt)
    Gd, Cd = be.convert(s, dt)
    Sb, Pb, gam, Gi = be.form_schur(s, Gd, Cd, s.g.astype(dt), s.c.astype(dt))
    return dict(G_dense=Gd, C_dense=Cd, Ginv=Gi, S=Sb, Pinv_bj=Pb, gamma=gam, Pinv=be.form_ss(s, Sb, Pb))


def feed_of(ref):
    return {n: ref.rounded(n) for n in ("Ginv", "S", "Pinv_bj")}


@functools.lru_cache(maxsize=None)
def oracle_stage_errors(S, C, K, dt, seed=0):
    """(e of the C oracle, e of the numpy oracle) per buffer, stages isolated."""
    s, ref = system_of(S, C, K, dt, seed), reference_of(S, C, K, dt, seed)
    lam = random_lambda(S, K, dt, seed)
    truth = dict(ref.buf, dz=ref.dz(lam))
    return tuple(errors(isolated_stages(OracleBackend(m), s, dt, feed_of(ref), lam), truth, S, C, K, STAGE_BUFFERS) for m in (co, o))


@functools.lru_cache(maxsize=None)
def oracle_chain_errors(S, C, K, dt, seed=0):
    s, ref = system_of(S, C, K, dt, seed), reference_of(S, C, K, dt, seed)
    return tuple(errors(chained_stages(OracleBackend(m), s, dt), ref.buf, S, C, K, WHOLE_BUFFERS + ("Pinv_bj",)) for m in (co, o))


def pinv0_is_minus_q0(Pb, Gd, S):
    """Pinv[0].main == -(Q_0 + rho I) bit for bit (the first knot's block is copied, not inverted twice)."""
    return np.array_equal(Pb[S * S:2 * S * S], -Gd[:S * S])


def _on_device(S, C, K, dt, run, stand_in=None):
    """run(backend) on the stage entries of a new Solver (stand_in: on that backend instead - the CPU suite's dry run)."""
    if stand_in is not None:
        return run(stand_in)
    from gato_python_amd.solver import Solver
    sol = Solver(S, C, K, np.dtype(dt))
    try:
        return run(DeviceBackend(sol))
    finally:
        sol.close()


def device_stage_case(S, C, K, dt, seed=0, stand_in=None):
    """The four stage entries on one hard system -> (device buffers, e of the device, (e of the C order, e of the numpy order))."""
    s, ref = system_of(S, C, K, dt, seed), reference_of(S, C, K, dt, seed)
    lam = random_lambda(S, K, dt, seed)
    got = _on_device(S, C, K, dt, lambda be: isolated_stages(be, s, dt, feed_of(ref), lam), stand_in)
    truth = dict(ref.buf, dz=ref.dz(lam))
    return got, errors(got, truth, S, C, K, STAGE_BUFFERS), oracle_stage_errors(S, C, K, dt, seed)


def long_horizon_case(dt, stand_in=None):
    """The stage entries at LONG, windows of ten knots at LONG_WINDOWS against the dense reference of each window; form_ss and
    compute_dz are fed the C oracle's S, Pinv and Ginv (no dense reference of 16 400 knots), and the C order alone sets the bar.
    -> (device buffers, C oracle's buffers, e of the device, (e of the C order,))."""
    S, C, K = LONG
    blocks = hard_blocks(S, C, K, 0, COND, GRADE[dt])
    s = to_system(blocks)
    lam = random_lambda(S, K, dt)
    feed = chained_stages(OracleBackend(co), s, dt)
    want = isolated_stages(OracleBackend(co), s, dt, feed, lam)
    got = _on_device(S, C, K, dt, lambda be: isolated_stages(be, s, dt, feed, lam), stand_in)
    e_dev, e_c = dict.fromkeys(STAGE_BUFFERS, 0.0), dict.fromkeys(STAGE_BUFFERS, 0.0)
    for w in LONG_WINDOWS:
        w0, w1 = w - 2, min(w + 12, K)
        sub, lo, hi = window(blocks, w0, w1)
        assert lo == w and hi >= min(w + 10, K)
        ref = Reference(to_system(sub), dt)
        truth = dict(ref.buf, dz=ref.dz(lam[w0 * S:w1 * S]))
        knots = range(lo - w0, hi - w0)
        for n in STAGE_BUFFERS:
            for bufs, e in ((got, e_dev), (want, e_c)):
                part = knot_slice(n, bufs[n], S, C, K, w0, w1)
                e[n] = max(e[n], block_error(n, part, truth[n], S, C, w1 - w0, knots))
    return got, want, e_dev, (e_c,), expected_dense(blocks, s.rho, dt)


def device_batch_case(S, C, K, dt, mode):
    """BATCH different hard systems (seeds 0 ..) in one linsys_batched call with asm_mode = mode, one PCG iteration ->
    (last_asm_fused, [(e of system b's share of the work buffers against its own reference, its CPU orders' e)])."""
    import torch
    from gato_python_amd.solver import Solver
    systems = [system_of(S, C, K, dt, b) for b in range(BATCH)]
    sol = Solver(S, C, K, np.dtype(dt), batch=BATCH)
    sol.set_option("asm_mode", mode)
    lam, dz = sol.new(BATCH * S * K), sol.new(BATCH * sol.N)
    sol.linsys_batched(*sol.upload_batch(systems), 0.0, 1, RHO, lam, dz)
    torch.cuda.synchronize()
    sol.check_status()
    fused = sol.get_option("last_asm_fused")
    bufs = {n: sol.read_buffer(n).reshape(BATCH, -1) for n in WHOLE_BUFFERS}
    sol.close()
    return fused, [(errors({n: bufs[n][b] for n in bufs}, reference_of(S, C, K, dt, b).buf, S, C, K, WHOLE_BUFFERS),
                    oracle_chain_errors(S, C, K, dt, b)) for b in range(BATCH)]


def whole_call(sol, s, mode, tol=0.0, iters=1, blocks=None):
    """One linsys (or, with blocks = (G_blocks, C_blocks) without rho, linsys_blocks) call with option asm_mode = mode; -> the
    work buffers, lambda and dz as host arrays, and last_asm_fused."""
    import torch
    sol.set_option("asm_mode", mode)
    lam, dz = sol.new(s.S * s.K), sol.new(sol.N)
    if blocks is None:
        sol.linsys(*sol.upload_system(s), tol, iters, s.rho, lam, dz)
    else:
        t = sol.to_device
        sol.linsys_blocks(t(blocks[0]), t(blocks[1]) if s.K > 1 else sol.new(1), t(s.g), t(s.c), tol, iters, s.rho, lam, dz)
    torch.cuda.synchronize()
    sol.check_status()
    out = {n: sol.read_buffer(n) for n in WHOLE_BUFFERS}
    out.update(lam=lam.cpu().numpy(), dz=dz.cpu().numpy(), fused=sol.get_option("last_asm_fused"))
    return out
