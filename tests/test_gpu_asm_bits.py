"""The assembly's work buffers, bit for bit against the commit before the Gauss-Jordan issue order changed.

gj_inverse_reg (csrc/gato_gj.h) issues its row updates pivot-row-first, reads the multipliers of a step ahead of its FMAs and
starts the next pivot's reciprocal under them; the fused launch loads g and c ahead of the CSR round trip.  None of that may
change a floating-point operation or an operand.  Stage launches and fused launch share the elimination, so they cannot
check each other here: tests/golden/asm_bits_parent.json holds SHA-256 digests of Ginv, S, Pinv, gamma, lambda (3 PCG
iterations) and dz recorded from the parent commit's library (tools/record_asm_bits.py); cases in tests/asm_bits_cases.py."""
import json

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import asm_bits_cases as ab                        # noqa: E402  (tests/asm_bits_cases.py)

CASES = ab.all_cases()


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    with open(ab.GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_work_buffers_have_the_parents_bits(golden, cid):
    case = dict(CASES)[cid]
    got = ab.run_case(case)
    want = golden[cid]
    differ = [(p, b) for p, _ in ab.PATHS for b in ab.BUFFERS if got[p][b] != want[p][b]]
    print(cid, "buffers that differ from the parent's:", differ or "none")
    assert not differ, (cid, differ)
