"""Re-solve entries without a GPU: declarations, exports and the refusals that come before any device work."""
import ctypes as ct
import os

import numpy as np
import pytest

from gato_python_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gato_solver_reserve_rhs", "gato_solve_rhs", "gato_linsys_resolve_f32", "gato_linsys_resolve_f64")


def test_header_declares_and_library_exports_the_resolve_entries():
    header = open(os.path.join(ROOT, "include", "gato_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert f" {name}(" in header, name
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS, name


def test_solve_rhs_of_no_solver_is_refused():
    L = _lib.lib()
    rc = L.gato_solve_rhs(None, 1, None, None, 1e-6, 10, None, None, None, None)
    assert rc == -1
    assert "solve_rhs" in L.gato_last_error().decode()
    assert L.gato_solver_reserve_rhs(None, 1) == -1


@pytest.mark.parametrize("name,dt", [("gato_linsys_resolve_f64", np.float64), ("gato_linsys_resolve_f32", np.float32)])
def test_host_resolve_before_any_solve_is_refused(name, dt):
    L = _lib.lib()
    L.gato_release_cache()
    g, c = np.zeros(8, dt), np.zeros(4, dt)
    lam, dz = np.zeros(4, dt), np.zeros(8, dt)
    it = ct.c_int(-7)
    p = lambda a: a.ctypes.data
    rc = getattr(L, name)(p(g), len(g), p(c), len(c), 1e-6, 10, p(lam), p(dz), ct.byref(it))
    assert rc == -1
    assert "no system to re-solve" in L.gato_last_error().decode()
    assert it.value == -7 and not lam.any() and not dz.any()


def test_linsys_resolve_argument_checks():
    import gato_python_amd as gp
    gp.set_precision("f64")
    try:
        _lib.lib().gato_release_cache()
        with pytest.raises(ValueError):                    # nothing to re-solve: refused as linsys_solve refuses bad input
            gp.linsys_resolve([0.0] * 8, [0.0] * 4, 1e-6, 10)
        with pytest.raises(TypeError):                     # not numbers: the same list conversion as linsys_solve
            gp.linsys_resolve(["a"] * 8, [0.0] * 4, 1e-6, 10)
        with pytest.raises((TypeError, ValueError)):
            gp.linsys_solve([0], [], [], [0], [], [], ["a"], [0.0], [0.0], 1, 1e-6, 10, 0, 1e-3)
    finally:
        gp.set_precision("f32")
