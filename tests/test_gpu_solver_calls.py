"""What gato_python_amd.solver hands the C library, call for call: tools/solver_call_trace.py drives a fixed script of the public
Solver methods through a recorder in place of the library object and notes per C call the function, every scalar argument, null
or non-null per pointer and which pointers share an address.  tests/golden/solver_calls.json is that trace recorded on the commit
before solver.py got its operand table, one checker and shared re-solve and tangent bodies: an argument in another slot, a
missing or an extra call, or an output that is no longer the tensor the caller gave shows as a difference.  Shapes 2/1/3 and
2/1/1 (K = 1 has no M and no C), B = 2, R = 2, both precisions, at most 20 PCG and 50 ADMM iterations per call."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_c_calls_are_those_of_the_golden_trace(golden_dir):
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    spec = importlib.util.spec_from_file_location("solver_call_trace", os.path.join(ROOT, "tools", "solver_call_trace.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got = json.loads(json.dumps(tool.record()))
    with open(os.path.join(golden_dir, "solver_calls.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for part in want:
        names = [c["fn"] for c in got[part]]
        assert names == [c["fn"] for c in want[part]], part
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, (part, i, g["fn"])
        print(part, len(names), "calls")
