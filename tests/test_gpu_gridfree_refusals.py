"""test_cpu_gridfree_refusals.py's replay for the cases that need a handle: missing pointers, noutput_items > max_batch,
ESPRIT and per-item counts at 32 bits, work_dev_auto's own rules, and the calls that break two rules at once (which pin the
order in which an entry refuses).  Every case is refused before the device is touched; the handle is what needs one."""
import pytest

import gridfree_cases as cases
from test_cpu_gridfree_refusals import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.REFUSALS_GPU)
def test_refusal_with_a_handle(name):
    assert cases.run_refusal(name) == GOLDEN[name]
