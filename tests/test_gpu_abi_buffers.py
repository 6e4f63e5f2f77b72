"""GPU: the buffer promises of include/jdet_hip.h -- inputs are never written, outputs are fully overwritten, no
entry point depends on the content of a workspace or writes outside a buffer -- for every row of tests/abi_cases.py,
by the guard-band / poison protocol of tests/guarded.py: a clean run A, a hostile run B (canaries in the outputs and
around every buffer, 0xFF workspaces, NaN next to every float input and in the unused columns of strided ones, poison
outside the window of blocked inputs), B == A bit for bit where the kernel is deterministic, both within the bound of
the kernel's existing test of its float64 / oracle reference, and a workspace claim one byte short refused with
JDET_E_WORKSPACE.  Each row prints one line: entry point, shape, whether B equalled A, max error, bound."""
import pytest

from tests import abi_cases, guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", abi_cases.CASES, ids=[c.id for c in abi_cases.CASES])
def test_buffer_contract(dev, case):
    guarded.run_case(case.entry_points[0], case.label, case.fn, dev)
