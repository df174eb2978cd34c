"""The refusals of the grid-free estimators' entries and of the seven entries the two pipeline handles share, replayed
against tests/golden/gridfree_refusals.json (recorded by tests/golden/make_gridfree_golden.py at the commit before the
entries moved onto gridfree_chain.hpp and PipeFront): return code and doa_last_error() text, byte for byte.  These are the
cases that need no handle, and so no device; test_gpu_gridfree_refusals.py replays the rest."""
import json
import os

import pytest

import gridfree_cases as cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gridfree_refusals.json")))


def test_the_recording_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(cases.REFUSALS_CPU + cases.REFUSALS_GPU)
    assert len(cases.REFUSALS_CPU) >= 40 and len(cases.REFUSALS_GPU) >= 90


@pytest.mark.parametrize("name", cases.REFUSALS_CPU)
def test_refusal_without_a_handle(name):
    assert cases.run_refusal(name) == GOLDEN[name]
