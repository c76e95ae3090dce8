"""Every PCG route, the four dz back-substitutions that ride in a PCG launch, and the re-solve's rhs_gamma_kernel, on inputs with
dense graded Q_k and R_k, A_k far from the identity and c_0 != 0, against the longdouble references of tests/pcg_ref.py: per
knot, beside the two CPU orders' own errors (the bars and where their factors come from: tests/pcg_ref.py; that they hold
between the CPU orders, that a subtly wrong kernel breaks them on these inputs and not on synth.make_system's, and each runner
below with the C oracle standing in: tests/test_pcg_ref_cpu.py).  Every test prints the per-buffer errors and ratios (pytest -s;
tools/pcg_accuracy.py records them in profiles/pcg_accuracy.json)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pcg_ref as pr                               # noqa: E402  (tests/pcg_ref.py)
from gato_python_amd import _lib                   # noqa: E402

names = lambda cases: [c.name for c in cases]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib.lib()                                    # the HIP library must be the thing that runs


def holds(facts, bad):
    assert [what for what, ok in facts if not ok] == []
    assert bad == []


@pytest.mark.parametrize("case", pr.CASES, ids=names(pr.CASES))
def test_pcg_routes(case):
    """Solver.pcg on the C oracle's matrices of the hard system: lambda after 1, 3 and 12 fixed iterations per knot against the
    longdouble PCG; the route the solver reports; the same bits on a second run; fp64: the converged lambda against the dense
    solution of those matrices at BASELINE's bar, the exit iteration within two of the C oracle's."""
    holds(*pr.run_pcg_route(case, pr.Device()))


@pytest.mark.parametrize("case", pr.DZ_CASES, ids=names(pr.DZ_CASES))
def test_dz_epilogues(case):
    """Whole linsys / linsys_batched calls (batches: three different systems) whose dz comes from the helper blocks or from the
    epilogue of each one-workgroup kernel: dz prefilled with NaN; dz and lambda the bits of the same call with the dz launch; dz
    per knot against the longdouble back-substitution of the device's own lambda."""
    holds(*pr.run_dz_case(case, pr.Device()))


@pytest.mark.parametrize("case,nofuse", pr.RESOLVE_RUNS, ids=[f"{c.name}-{'launch' if n else 'epilogue'}" for c, n in pr.RESOLVE_RUNS])
def test_resolve(case, nofuse):
    """solve_rhs of two new right-hand sides for each of two different systems: rhs_gamma_kernel's gamma and dz of every (b, r)
    per knot; fp64: the converged lambda and dz against the KKT solution at BASELINE's bar."""
    holds(*pr.run_resolve_case(case, nofuse, pr.Device()))
