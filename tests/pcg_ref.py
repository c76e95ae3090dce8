"""Every PCG route, every dz epilogue and the re-solve against references from the DEFINITIONS, on the dense, graded inputs of
tests/asm_ref.py (tests/test_pcg_ref_cpu.py, tests/test_gpu_pcg_ref.py, tools/pcg_accuracy.py).

Inputs: asm_ref.hard_blocks at asm_ref.COND and asm_ref.GRADE[dtype] - dense SPD Q_k and R_k, every block on its own power-of-two
scale, A_k far from the identity, c_0 != 0 - with asm_ref.RHO; new right-hand sides of a re-solve are Gaussian g and c (c_0 != 0)
from default_rng([seed, b, r, S, C, K]).

References (np.longdouble, none of them restates a kernel's order):
    pcg_ld           textbook PCG with dense matrix-vector products on dense_bd() of the very S / Pinv buffers the device is given
                     (the C oracle's chained assembly of the hard system in the run's dtype), every iterate;
    BlockReference   per knot, from the blocks of the dtype-rounded inputs: Q_k^-1, R_k^-1 (asm_ref.inv_ld),
                     gamma = c - C G^-1 g,  dz = G^-1 (g - C^T lambda), and lam_kkt / dz_kkt, the solution of S lambda = gamma with
                     S = -C G^-1 C^T put together from its blocks (asm_ref.solve_ld) - no dense N x N product.

Yardstick: asm_ref's.  Per knot e = max|got - truth| / max|truth|, a vector's e the maximum over its knots, and the bar
    e_gpu <= FACTOR * max(e of the CPU orders) + FLOOR_EPS eps.
CPU orders: for PCG co.pcg and o.pcg on the same matrices (pcg_variant = 1 cases: o.pcg_single_reduction and co.pcg); for gamma
and dz each oracle's form_schur / compute_dz on its own chained Ginv.

Where the PCG factors come from (tests/test_pcg_ref_cpu.py::test_each_cpu_order_is_within_the_bar_of_the_other is the
measurement; tools/pcg_accuracy.py --cpu prints these counts): the 20 cases of CASES x seeds 0, 1, 2, each CPU order judged against
the other with the floor of 16 eps - 120 comparisons per n.  Errors of the CPU orders, comparisons past 1 x, 2 x, 4 x, 8 x, and the
largest e_a / max(e_b, floor):
    n = 1      1 - 16 eps          0 /  0 / 0 / 0     0.98
    n = 3      7 - 336 eps        21 /  1 / 0 / 0     4.38
    n = 12     6 - 70 606 eps     37 /  8 / 2 / 0     4.41     (70 606 eps: 4/2/9 fp32, 36 unknowns, past its convergence)
The smallest power of two that no comparison passes is 1 at n = 1, 4 at n = 3 and 8 at n = 12: no n needs more than 8, so all
three are kept, each with its own factor (PCG_FACTOR).  At n = 12 the 4/2/9 fp32 case (pair-f32-4-2-9) is past its convergence:
both CPU orders are 23 000 - 70 600 eps off there, its bar is 7 % per knot and sees next to nothing; n = 1 and n = 3 carry that
case.  gamma of a new right-hand side and dz of a random lambda, every system of DZ_CASES
and RESOLVE_CASES (148 comparisons): none passes 2 x + 16 eps, the largest ratio is 1.58 (gamma) and 1.46 (dz);
asm_ref.FACTOR = 4 and FLOOR_EPS = 16 stand for them."""
import functools

import numpy as np

import asm_ref as ar
import resolve_sweep_ref as RS
from asm_ref import LD, co, o

F64, F32 = "float64", "float32"
PCG_FACTOR, FLOOR_EPS = {1: 1.0, 3: 4.0, 12: 8.0}, ar.FLOOR_EPS    # per fixed iteration count n
FACTOR = ar.FACTOR                                # gamma and dz
NS = (1, 3, 12)                                   # fixed iteration counts a route is judged at
SEEDS = (0, 1, 2)
# the fp64 converged solve: asm_ref's exit tolerance; the cap is one and a half times the most either CPU order took over every
# fp64 case and seeds 0, 1, 2 (267 iterations, 14/7/45 seed 1; seed 0, what the GPU suite runs: 224)
EXIT_TOL, MAX_ITERS = ar.EXIT_TOL, 400
BASELINE = 1e-6                                   # |dz - dz_ref|_inf, lambda relative
IT_SLACK = 2                                      # the two CPU orders' own exit iterations differ by up to two (6/3/9 seed 1: 26, 28)
F32_ITERS = 6                                     # whole solves in fp32 are judged at a fixed count only
REPORT = ("last_mode", "last_groups", "last_threads", "last_pair", "last_dpp", "last_variant", "last_dz_fused")
DISTINCT = 1e-3


class Case:
    """One PCG route: shape, dtype, the options that select it and the last_* options that prove it ran."""

    def __init__(self, name, S, C, K, dt, opts=None, route=None):
        self.name, self.S, self.C, self.K, self.dt = name, S, C, K, dt
        self.opts, self.route = dict(opts or {}), dict(route or {})

    @property
    def cg1(self):
        return self.opts.get("pcg_variant") == 1

    @property
    def key(self):
        return (self.S, self.C, self.K, self.dt)


def _sweep(name, **more):
    """A route of resolve_sweep_ref.ROUTES / LAUNCHES under its name there."""
    c = RS.BY_NAME[name]
    return Case(name, c.S, c.C, c.K, np.dtype(c.dt).name, c.opts, dict(c.route, **more))


MULTI = dict(last_mode=1, last_pair=0, last_variant=0)
CASES = [
    # fp32, two rows per lane (14/7/19: a wave boundary inside a knot)
    _sweep("pair-f32-14-7-9"),
    Case("pair-f32-14-7-19", 14, 7, 19, F32, route=dict(RS.ONE_WG, last_pair=1)),
    _sweep("pair-f32-4-2-9"),                     # (36 unknowns: converged before n = 12, where its bar is 7 % per knot - judged by n = 1, 3)
    # fp64 mixed rows: 14/7/37 leaves lanes idle, 14/7/50 is the largest
    Case("mixed-f64-14-7-37", 14, 7, 37, F64, route=dict(RS.ONE_WG, last_pair=2, last_threads=512)),
    Case("mixed-f64-14-7-50", 14, 7, 50, F64, route=dict(RS.ONE_WG, last_pair=2, last_threads=512)),
    _sweep("dpp-f64-14-7-20"), _sweep("dpp-f64-12-6-9"), _sweep("dpp-f64-32-16-5"),
    _sweep("plain-f64-2-1-9"), _sweep("plain-f64-6-3-9"),
    _sweep("plain-f32-14-7-9-no_pair"), _sweep("plain-f32-32-16-7"),
    _sweep("single-cu-f64-14-7-45", last_threads=640),
    _sweep("cg1-f64-14-7-16"), _sweep("cg1-f32-14-7-9"),
    # several workgroups at a size whose dense reference is cheap.  (no_single_lds = 1 and dpp_rows = 1 reach the SAME launch here, by
    # two ways through the planner - the DPP-row kernel in two workgroups of 512 - and no last_* option tells the ways apart: the
    # device's lambda is the same bits in both, and the two cases pin that either option still lands there.)
    Case("wg13-f64-14-7-50-threads64", 14, 7, 50, F64, dict(pcg_threads=64), dict(MULTI, last_groups=13, last_threads=64, last_dpp=1)),
    Case("wg2-f64-14-7-50-no_single_lds", 14, 7, 50, F64, dict(no_single_lds=1), dict(MULTI, last_groups=2, last_dpp=1)),
    Case("wg2-f64-14-7-50-dpp_rows", 14, 7, 50, F64, dict(dpp_rows=1), dict(MULTI, last_groups=2, last_dpp=1)),
    Case("wg7-f32-14-7-50-groups7", 14, 7, 50, F32, dict(pcg_groups=7), dict(MULTI, last_groups=7, last_dpp=0)),
    _sweep("streaming-f64-14-7-50"),
]
BY_NAME = {c.name: c for c in CASES}


class SolveCase:
    """A whole linsys (B = 1) or linsys_batched (B different systems, seeds 0 ..) call and what the solver must report of it."""

    def __init__(self, name, S, C, K, dt, B=1, opts=None, expect=None):
        self.name, self.S, self.C, self.K, self.dt, self.B = name, S, C, K, dt, B
        self.opts, self.expect = dict(opts or {}), dict(expect or {})

    @property
    def tol_iters(self):
        return (EXIT_TOL, MAX_ITERS) if self.dt == F64 else (0.0, F32_ITERS)


_EPI = dict(no_fuse_dz=-1, no_pair=1)


def _exp(fused, pair):
    return dict(last_dz_fused=fused, last_pair=pair, last_groups=1)


BATCH = 3
# the four dz sites: helper blocks (last_dz_fused = 2; pair = 2: pcg_single_f64m_kernel's launch, pair = 1: pcg_single_f32x2_kernel's),
# the epilogue of pcg_single_f32x2_kernel (batch, pair = 1), of pcg_single_f64m_kernel (pair = 2 with last_dz_fused = 1) and of
# pcg_resident_kernel (pair = 0)
DZ_CASES = [
    SolveCase("helpers-f64-14-7-37", 14, 7, 37, F64, expect=_exp(2, 2)),
    SolveCase("helpers-f64-14-7-50", 14, 7, 50, F64, expect=_exp(2, 2)),
    SolveCase("helpers-f32-14-7-9", 14, 7, 9, F32, expect=_exp(2, 1)),
    SolveCase("helpers-f32-14-7-19", 14, 7, 19, F32, expect=_exp(2, 1)),
    SolveCase("resident-f64-14-7-20", 14, 7, 20, F64, opts=_EPI, expect=_exp(1, 0)),
    SolveCase("resident-f64-2-1-9", 2, 1, 9, F64, opts=_EPI, expect=_exp(1, 0)),
    SolveCase("resident-f32-32-16-5", 32, 16, 5, F32, opts=_EPI, expect=_exp(1, 0)),
    SolveCase("mixed-epilogue-f64-14-7-50", 14, 7, 50, F64, opts=dict(no_fuse_dz=-1), expect=_exp(1, 2)),
    SolveCase("batch-mixed-f64-14-7-37", 14, 7, 37, F64, BATCH, expect=_exp(1, 2)),
    SolveCase("batch-f64-14-7-9", 14, 7, 9, F64, BATCH, expect=_exp(1, 0)),
    SolveCase("batch-f32-14-7-9", 14, 7, 9, F32, BATCH, expect=_exp(1, 1)),
    SolveCase("batch-f64-32-16-5", 32, 16, 5, F64, BATCH, expect=_exp(1, 0)),
    SolveCase("batch-f32-32-16-5", 32, 16, 5, F32, BATCH, expect=_exp(1, 0)),
]
# the re-solve: B = 2 different systems x R = 2 new right-hand sides, one case per one-workgroup route family; every one with
# dz in the PCG launch's epilogue and as a launch of its own, but the single-reduction kernel, which has no epilogue
RESOLVE_B, RESOLVE_R = 2, 2
RESOLVE_CASES = [SolveCase(n, BY_NAME[n].S, BY_NAME[n].C, BY_NAME[n].K, BY_NAME[n].dt, RESOLVE_B, BY_NAME[n].opts,
                           {k: v for k, v in BY_NAME[n].route.items() if k != "last_threads"})
                 for n in ("pair-f32-14-7-9", "mixed-f64-14-7-37", "dpp-f64-14-7-20", "plain-f64-6-3-9", "plain-f32-32-16-7",
                           "single-cu-f64-14-7-45", "cg1-f64-14-7-16")]
RESOLVE_RUNS = [(c, nofuse) for c in RESOLVE_CASES for nofuse in (0, 1) if nofuse or not c.opts.get("pcg_variant")]


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def dense_bd(buf, S, K):
    """The dense S K x S K longdouble matrix of a [K][3][S*S] column-major left / main / right buffer; left of knot 0 and right
    of knot K - 1 are not read."""
    b = np.asarray(buf).reshape(K, 3, S, S)
    M = np.zeros((S * K, S * K), LD)
    for k in range(K):
        r = slice(k * S, (k + 1) * S)
        M[r, r] = b[k, 1].T
        if k > 0:
            M[r, (k - 1) * S:k * S] = b[k, 0].T
        if k < K - 1:
            M[r, (k + 1) * S:(k + 2) * S] = b[k, 2].T
    return M


def pcg_ld(Sd, Pd, gamma, n):
    """Preconditioned conjugate gradients on S lambda = gamma from lambda = 0 with the preconditioner Pd ~ S^-1, in longdouble
    with dense products: [lambda_1, ..., lambda_n]."""
    Sd, Pd = np.asarray(Sd, LD), np.asarray(Pd, LD)
    r = np.asarray(gamma, LD).copy()
    lam = np.zeros_like(r)
    z = Pd @ r
    p = z.copy()
    eta = r @ z
    out = []
    for _ in range(n):
        Sp = Sd @ p
        alpha = eta / (p @ Sp)
        lam = lam + alpha * p
        r = r - alpha * Sp
        z = Pd @ r
        eta_new = r @ z
        p = z + (eta_new / eta) * p
        eta = eta_new
        out.append(lam.copy())
    return out


class BlockReference:
    """The longdouble reference of one system as run in dtype dt, knot by knot.  Q, R (rho added), A, B, Qi, Ri: the blocks;
    g, c: the system's own right-hand side; gamma(g, c), dz(lam, g), lam_kkt(g, c), dz_kkt(g, c) (g, c None: the system's own)."""

    def __init__(self, s, dt):
        from scipy import sparse
        dt = np.dtype(dt)
        S, C, K = s.S, s.C, s.K
        n, N = S + C, s.N
        sr = s.astype(dt)
        rho = LD(dt.type(s.rho))
        G = sparse.csr_matrix((sr.G_val.astype(np.float64), sr.G_col, sr.G_row), shape=(N, N)).tocsc()
        Cm = sparse.csr_matrix((sr.C_val.astype(np.float64), sr.C_col, sr.C_row), shape=(S * K, N)).tocsc()
        blk = lambda M, r0, r1, c0, c1: M[r0:r1, c0:c1].toarray().astype(LD)
        self.Q = np.stack([blk(G, k * n, k * n + S, k * n, k * n + S) + rho * np.eye(S, dtype=LD) for k in range(K)])
        self.R = np.stack([blk(G, k * n + S, (k + 1) * n, k * n + S, (k + 1) * n) + rho * np.eye(C, dtype=LD) for k in range(K - 1)]) \
            if K > 1 else np.zeros((0, C, C), LD)
        self.A = np.stack([blk(Cm, (k + 1) * S, (k + 2) * S, k * n, k * n + S) for k in range(K - 1)]) if K > 1 else np.zeros((0, S, S), LD)
        self.B = np.stack([blk(Cm, (k + 1) * S, (k + 2) * S, k * n + S, (k + 1) * n) for k in range(K - 1)]) if K > 1 else np.zeros((0, S, C), LD)
        self.Qi = np.stack([ar.inv_ld(M) for M in self.Q])
        self.Ri = np.stack([ar.inv_ld(M) for M in self.R]) if K > 1 else self.R
        self.S_, self.C_, self.K, self.dt = S, C, K, dt
        self.g, self.c = sr.g.astype(LD), sr.c.astype(LD)
        self._S = None

    def _split(self, g):
        """g [N] -> q [K, S], r [K - 1, C]."""
        S, C, K = self.S_, self.C_, self.K
        n = S + C
        g = np.asarray(g, LD)
        q = np.stack([g[k * n:k * n + S] for k in range(K)])
        r = np.stack([g[k * n + S:(k + 1) * n] for k in range(K - 1)]) if K > 1 else np.zeros((0, C), LD)
        return q, r

    def gamma(self, g=None, c=None):
        """c - C G^-1 g: row block 0 of C is the identity on x_0, row block k >= 1 is [A_{k-1} B_{k-1}] on (x, u)_{k-1}, I on x_k."""
        S, K = self.S_, self.K
        q, r = self._split(self.g if g is None else g)
        c = np.asarray(self.c if c is None else c, LD).reshape(K, S)
        out = np.zeros((K, S), LD)
        for k in range(K):
            out[k] = c[k] - self.Qi[k] @ q[k]
            if k > 0:
                out[k] -= self.A[k - 1] @ (self.Qi[k - 1] @ q[k - 1]) + self.B[k - 1] @ (self.Ri[k - 1] @ r[k - 1])
        return out.reshape(-1)

    def dz(self, lam, g=None):
        """G^-1 (g - C^T lambda)."""
        S, C, K = self.S_, self.C_, self.K
        n = S + C
        q, r = self._split(self.g if g is None else g)
        lam = np.asarray(lam, LD).reshape(K, S)
        out = np.zeros(n * K - C, LD)
        for k in range(K):
            t = q[k] - lam[k]
            if k < K - 1:
                t = t - self.A[k].T @ lam[k + 1]
                out[k * n + S:(k + 1) * n] = self.Ri[k] @ (r[k] - self.B[k].T @ lam[k + 1])
            out[k * n:k * n + S] = self.Qi[k] @ t
        return out

    def schur(self):
        """S = -C G^-1 C^T, dense S K x S K, put together from its blocks."""
        if self._S is None:
            S, K = self.S_, self.K
            M = np.zeros((S * K, S * K), LD)
            for k in range(K):
                d = slice(k * S, (k + 1) * S)
                M[d, d] = -self.Qi[k]
                if k > 0:
                    A, B = self.A[k - 1], self.B[k - 1]
                    phi = A @ self.Qi[k - 1]
                    M[d, d] -= phi @ A.T + (B @ self.Ri[k - 1]) @ B.T
                    M[d, (k - 1) * S:k * S] = -phi
                    M[(k - 1) * S:k * S, d] = -phi.T
            self._S = M
        return self._S

    def lam_kkt(self, g=None, c=None):
        return ar.solve_ld(self.schur(), self.gamma(g, c))

    def dz_kkt(self, g=None, c=None):
        return self.dz(self.lam_kkt(g, c), g)


@functools.lru_cache(maxsize=None)
def block_reference_of(S, C, K, dt, seed=0):
    return BlockReference(ar.system_of(S, C, K, dt, seed), dt)


@functools.lru_cache(maxsize=None)
def chain_of(S, C, K, dt, seed=0, numpy_order=False):
    """The chained assembly of a hard system by the C oracle (numpy_order: the numpy oracle)."""
    return ar.chained_stages(ar.OracleBackend(o if numpy_order else co), ar.system_of(S, C, K, dt, seed), dt)


def chains_of(S, C, K, dt, seed=0):
    return chain_of(S, C, K, dt, seed), chain_of(S, C, K, dt, seed, True)


@functools.lru_cache(maxsize=None)
def pcg_truth(S, C, K, dt, seed=0):
    """([lambda_1 .. lambda_max(NS)] of pcg_ld, S^-1 gamma by asm_ref.solve_ld) on the C oracle's chained matrices."""
    m = chain_of(S, C, K, dt, seed)
    Sd, Pd = dense_bd(m["S"], S, K), dense_bd(m["Pinv"], S, K)
    return pcg_ld(Sd, Pd, m["gamma"], max(NS)), ar.solve_ld(Sd, m["gamma"])


def new_rhs(S, C, K, dt, seed, b, r):
    """(g [N], c [S K]) of right-hand side r of system b, in dt."""
    rng = np.random.default_rng([seed, b, r, S, C, K])
    return rng.standard_normal((S + C) * K - C).astype(dt), rng.standard_normal(S * K).astype(dt)


def lam_error(lam, truth, S, C, K):
    return ar.block_error("gamma", lam, truth, S, C, K)


def dz_error(dz, truth, S, C, K):
    return ar.block_error("dz", dz, truth, S, C, K)


def rel(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the CPU orders
# ---------------------------------------------------------------------------------------------------------------------------
def cpu_orders_pcg(case, m, tol, iters):
    """[(lambda, iterations)] of the two CPU orders of a case on the matrices m."""
    S, K = case.S, case.K
    first = o.pcg_single_reduction if case.cg1 else o.pcg
    return [first(m["S"], m["Pinv"], m["gamma"], S, K, tol, iters), co.pcg(m["S"], m["Pinv"], m["gamma"], S, K, tol, iters)]


@functools.lru_cache(maxsize=None)
def cpu_pcg_errors(name, seed=0):
    """Per CPU order {"lambda after n": e} of a case."""
    case = BY_NAME[name]
    S, C, K, dt = case.key
    m, (truth, _) = chain_of(S, C, K, dt, seed), pcg_truth(S, C, K, dt, seed)
    out = ({}, {})
    for n in NS:
        for e, (lam, _) in zip(out, cpu_orders_pcg(case, m, 0.0, n)):
            e[f"lambda after {n}"] = lam_error(lam, truth[n - 1], S, C, K)
    return out


def cpu_orders_dz(chains, S, C, K, dt, g, lam):
    """dz of both oracles' compute_dz, each on its own chained Ginv (chains: the C oracle's and the numpy oracle's assembly)."""
    return [mod.compute_dz(m["Ginv"], m["C_dense"], np.asarray(g, dt), np.asarray(lam, dt), S, C, K) for mod, m in zip((co, o), chains)]


def cpu_orders_gamma(chains, S, C, K, dt, g, c):
    """gamma of both oracles' form_schur on (g, c)."""
    return [mod.form_schur(m["G_dense"], m["C_dense"], np.asarray(g, dt), np.asarray(c, dt), S, C, K)[2] for mod, m in zip((co, o), chains)]


# ---------------------------------------------------------------------------------------------------------------------------
# backends: the device, and the C oracle standing in for it (the CPU suite's dry run of every runner below)
# ---------------------------------------------------------------------------------------------------------------------------
class Device:
    @staticmethod
    def _solver(S, C, K, dt, B, opts):
        from gato_python_amd.solver import Solver
        sol = Solver(S, C, K, np.dtype(dt), batch=B)
        for k, v in opts.items():
            sol.set_option(k, v)
        return sol

    @staticmethod
    def _report(sol):
        return {k: sol.get_option(k) for k in REPORT}

    def pcg(self, case, m, runs):
        """Solver.pcg on the host matrices m, once per (exit_tol, max_iters) of runs -> ([(lambda, iterations)], last_* report)."""
        sol = self._solver(case.S, case.C, case.K, case.dt, 1, case.opts)
        try:
            dS, dP, dg = sol.to_device(m["S"]), sol.to_device(m["Pinv"]), sol.to_device(m["gamma"])
            out = []
            for tol, iters in runs:
                lam, it = sol.pcg(dS, dP, dg, tol, iters)
                out.append((lam.cpu().numpy().copy(), int(it.cpu().numpy()[0])))
            return out, self._report(sol)
        finally:
            sol.close()

    def solve(self, case, systems, opts, tol, iters, rhs=None):
        """linsys (one system) or linsys_batched with dz prefilled with NaN -> dict lam [B, S K], dz [B, N], report; rhs = (g, c)
        [B][R] flat: then solve_rhs as well -> gamma2, lam2, dz2 [B, R, .], it2 [B, R], report2."""
        import torch
        S, K, B = case.S, case.K, len(systems)
        sol = self._solver(S, case.C, K, case.dt, B, opts)
        try:
            lam, dz = sol.new(B * S * K).zero_(), sol.new(B * sol.N).fill_(float("nan"))
            if B > 1:
                sol.linsys_batched(*sol.upload_batch(systems), tol, iters, systems[0].rho, lam, dz)
            else:
                sol.linsys(*sol.upload_system(systems[0]), tol, iters, systems[0].rho, lam, dz)
            torch.cuda.synchronize()
            sol.check_status()
            out = dict(lam=lam.cpu().numpy().reshape(B, -1), dz=dz.cpu().numpy().reshape(B, -1), report=self._report(sol))
            if rhs is not None:
                g2, c2 = sol.to_device(rhs[0]), sol.to_device(rhs[1])
                R = g2.numel() // (B * sol.N)
                dz2 = sol.new(B * R * sol.N).fill_(float("nan"))
                lam2, dz2, it2 = sol.solve_rhs(g2, c2, tol, iters, dz=dz2)
                torch.cuda.synchronize()
                sol.check_status()
                out.update(gamma2=sol.read_rhs_gamma(R).reshape(B, R, -1), lam2=lam2.cpu().numpy().reshape(B, R, -1),
                           dz2=dz2.cpu().numpy().reshape(B, R, -1), it2=it2.cpu().numpy().reshape(B, R), report2=self._report(sol))
            return out
        finally:
            sol.close()


class StandIn:
    """The C oracle behind Device's two methods; it reports the route it is asked for."""

    def pcg(self, case, m, runs):
        rep = dict.fromkeys(REPORT, 0)
        rep.update(case.route)
        return [co.pcg(m["S"], m["Pinv"], m["gamma"], case.S, case.K, tol, iters) for tol, iters in runs], rep

    def solve(self, case, systems, opts, tol, iters, rhs=None):
        S, C, K, dt, B = case.S, case.C, case.K, np.dtype(case.dt), len(systems)
        rep = dict.fromkeys(REPORT, 0)
        rep.update(case.expect)
        rep["last_dz_fused"] = 0 if opts.get("no_fuse_dz") == 1 or opts.get("pcg_variant") else case.expect.get("last_dz_fused", 1)
        sols = [co.linsys_solve(*s.csr_args(), S, C, K, tol, iters, s.rho, dtype=dt) for s in systems]
        out = dict(lam=np.stack([x[0] for x in sols]), dz=np.stack([x[1] for x in sols]), report=rep)
        if rhs is not None:
            N = (S + C) * K - C
            g2, c2 = np.asarray(rhs[0], dt).reshape(B, -1, N), np.asarray(rhs[1], dt).reshape(B, -1, S * K)
            R = g2.shape[1]
            gam, lam2, dz2 = (np.zeros((B, R, n), dt) for n in (S * K, S * K, N))
            it2 = np.zeros((B, R), np.int32)
            for b, s in enumerate(systems):
                Gd, Cd = co.convert(*s.csr_args()[:6], S, C, K, s.rho, dt)
                for r in range(R):
                    Sb, Pb, gam[b, r], Gi = co.form_schur(Gd, Cd, g2[b, r], c2[b, r], S, C, K)
                    lam2[b, r], it2[b, r] = co.pcg(Sb, co.form_ss(Sb, Pb, S, K), gam[b, r], S, K, tol, iters)
                    dz2[b, r] = co.compute_dz(Gi, Cd, g2[b, r], lam2[b, r], S, C, K)
            out.update(gamma2=gam, lam2=lam2, dz2=dz2, it2=it2, report2=rep)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# runners: -> (what must hold exactly: a list of (description, bool); the buffers past the bar, as asm_ref.judge lists them)
# ---------------------------------------------------------------------------------------------------------------------------
def check_report(name, report, want):
    print(name, report)
    return [(f"{name}: {k} = {report[k]}, expected {v}", report[k] == v) for k, v in want.items()]


def run_pcg_route(case, backend, seed=0, record=None):
    """A route at every n of NS and, in fp64, to convergence: lambda per knot against pcg_ld beside both CPU orders; the route;
    a bit-identical second run; the converged lambda against the dense solution of the same matrices at BASELINE's bar, the exit
    iteration within IT_SLACK of the C oracle's."""
    S, C, K, dt = case.key
    m, (truth, lam_dense) = chain_of(S, C, K, dt, seed), pcg_truth(S, C, K, dt, seed)
    f64 = dt == F64
    runs = [(0.0, n) for n in NS] + ([(EXIT_TOL, MAX_ITERS)] if f64 else [])
    got, report = backend.pcg(case, m, runs + runs[-1:])
    facts = check_report(case.name, report, case.route)
    facts.append((f"{case.name}: the second run gave other bits", np.array_equal(got[-1][0], got[-2][0]) and got[-1][1] == got[-2][1]))
    e_or, bad = cpu_pcg_errors(case.name, seed), []
    for n, (lam, it) in zip(NS, got):
        facts.append((f"{case.name}: {it} iterations reported of {n} fixed", it == n))
        e_dev = {f"lambda after {n}": lam_error(lam, truth[n - 1], S, C, K)}
        bad += ar.judge(case.name, dt, e_dev, e_or, e_dev, PCG_FACTOR[n])
        if record is not None:
            record(case.name, dt, e_dev, e_or, PCG_FACTOR[n])
    if f64:
        lam, it = got[len(NS)]
        it_c = co.pcg(m["S"], m["Pinv"], m["gamma"], S, K, EXIT_TOL, MAX_ITERS)[1]
        el = rel(lam, lam_dense)
        print(f"{case.name} converged: {it} iterations (C oracle {it_c}), lambda {el:.1e} relative to the dense solution")
        facts.append((f"{case.name}: converged lambda {el:.1e} from the dense solution", el < BASELINE))
        facts.append((f"{case.name}: {it} iterations, C oracle {it_c}", abs(it - it_c) <= IT_SLACK and it < MAX_ITERS))
    return facts, bad


def judge_dz(what, case, seed, lam, dz, g=None, record=None):
    """dz against BlockReference.dz of the SAME lambda, beside both oracles' compute_dz of that lambda."""
    S, C, K, dt = case.S, case.C, case.K, case.dt
    ref = block_reference_of(S, C, K, dt, seed)
    truth = ref.dz(lam, g)
    gg = ar.system_of(S, C, K, dt, seed).g if g is None else g
    e_or = tuple(dict(dz=dz_error(x, truth, S, C, K)) for x in cpu_orders_dz(chains_of(S, C, K, dt, seed), S, C, K, dt, gg, lam))
    e_dev = dict(dz=dz_error(dz, truth, S, C, K))
    if record is not None:
        record(what, dt, e_dev, e_or, FACTOR)
    return ar.judge(what, dt, e_dev, e_or, factor=FACTOR)


def run_dz_case(case, backend, record=None):
    """One whole call with dz in the PCG launch and one with no_fuse_dz = 1: the report, the same bits, dz per knot."""
    systems = [ar.system_of(case.S, case.C, case.K, case.dt, b) for b in range(case.B)]
    tol, iters = case.tol_iters
    fused = backend.solve(case, systems, case.opts, tol, iters)
    plain = backend.solve(case, systems, dict(case.opts, no_fuse_dz=1), tol, iters)
    facts = check_report(case.name, fused["report"], case.expect)
    facts += check_report(case.name + " no_fuse_dz = 1", plain["report"], dict(case.expect, last_dz_fused=0))
    facts.append((f"{case.name}: lambda differs from the run with the dz launch", np.array_equal(fused["lam"], plain["lam"])))
    facts.append((f"{case.name}: dz differs from the dz launch's", np.array_equal(fused["dz"], plain["dz"])))
    bad = []
    for b in range(case.B):
        bad += judge_dz(f"{case.name} system {b}", case, b, fused["lam"][b], fused["dz"][b], record=record)
    return facts, bad


def resolve_inputs(case):
    """(systems [B], g [B][R][N], c [B][R][S K]) of a re-solve case."""
    S, C, K, dt = case.S, case.C, case.K, case.dt
    systems = [ar.system_of(S, C, K, dt, b) for b in range(case.B)]
    rhs = [[new_rhs(S, C, K, dt, 0, b, r) for r in range(RESOLVE_R)] for b in range(case.B)]
    return systems, np.stack([[x[0] for x in per] for per in rhs]), np.stack([[x[1] for x in per] for per in rhs])


def run_resolve_case(case, nofuse, backend, record=None):
    """A whole solve of B different systems, then solve_rhs of R new right-hand sides each: gamma and dz of every (b, r) per
    knot; fp64: the converged lambda and dz against lam_kkt / dz_kkt at BASELINE's bar."""
    S, C, K, dt = case.S, case.C, case.K, case.dt
    systems, g2, c2 = resolve_inputs(case)
    tol, iters = case.tol_iters
    opts = dict(case.opts, no_fuse_dz=1) if nofuse else case.opts
    got = backend.solve(case, systems, opts, tol, iters, rhs=(g2.reshape(-1), c2.reshape(-1)))
    name = case.name + (" dz launch" if nofuse else " dz epilogue")
    want = dict(case.expect, last_dz_fused=0 if nofuse or case.opts.get("pcg_variant") else 1)
    facts = check_report(name, got["report2"], want)
    if not nofuse:                                                # the epilogue's bits are those of the dz launch, every (b, r)
        plain = backend.solve(case, systems, dict(case.opts, no_fuse_dz=1), tol, iters, rhs=(g2.reshape(-1), c2.reshape(-1)))
        facts += check_report(name + ", again with no_fuse_dz = 1", plain["report2"], dict(want, last_dz_fused=0))
        for n in ("gamma2", "lam2", "dz2", "it2"):
            facts.append((f"{name}: {n} differs from the run with the dz launch", np.array_equal(got[n], plain[n])))
    bad = []
    for b in range(case.B):
        ref = block_reference_of(S, C, K, dt, b)
        for r in range(RESOLVE_R):
            what = f"{name} system {b} rhs {r}"
            truth = ref.gamma(g2[b, r], c2[b, r])
            e_or = tuple(dict(gamma=lam_error(x, truth, S, C, K)) for x in cpu_orders_gamma(chains_of(S, C, K, dt, b), S, C, K, dt, g2[b, r], c2[b, r]))
            e_dev = dict(gamma=lam_error(got["gamma2"][b, r], truth, S, C, K))
            if record is not None:
                record(what, dt, e_dev, e_or, FACTOR)
            bad += ar.judge(what, dt, e_dev, e_or, factor=FACTOR)
            bad += judge_dz(what, case, b, got["lam2"][b, r], got["dz2"][b, r], g2[b, r], record)
            if dt == F64:
                lam_t = ref.lam_kkt(g2[b, r], c2[b, r])
                el, ez = rel(got["lam2"][b, r], lam_t), float(np.abs(got["dz2"][b, r] - ref.dz(lam_t, g2[b, r])).max())
                print(f"{what} converged: {got['it2'][b, r]} iterations, lambda {el:.1e} relative, |dz - dz_ref|_inf {ez:.1e}")
                facts.append((f"{what}: lambda {el:.1e}, dz {ez:.1e} from the KKT solution", el < BASELINE and ez < BASELINE))
    return facts, bad


def distinct(case):
    """min over (b, r) of the relative distance between the reference solution (lambda, dz, and gamma) of right-hand side (b, r)
    with the matrices of system b and with those of system (b + 1) % B: what reading the wrong system's matrices costs."""
    S, C, K, dt = case.S, case.C, case.K, case.dt
    _, g2, c2 = resolve_inputs(case)
    worst = np.inf
    for b in range(case.B):
        own, other = block_reference_of(S, C, K, dt, b), block_reference_of(S, C, K, dt, (b + 1) % case.B)
        for r in range(RESOLVE_R):
            g, c = g2[b, r], c2[b, r]
            worst = min(worst, rel(other.lam_kkt(g, c), own.lam_kkt(g, c)), rel(other.dz_kkt(g, c), own.dz_kkt(g, c)),
                        rel(other.gamma(g, c), own.gamma(g, c)))
    return worst
