"""Every form of rootMUSIC_linear_array, esprit_linear_array and root_pipeline on the seeded inputs of
tests/golden/gridfree_chain_bits.npz, compared word for word (==, no tolerance) with the outputs recorded there by
tests/golden/make_gridfree_golden.py at the commit before the three moved onto gridfree_chain.hpp: angles, status words,
counts, eigenvalues, the roots of the debug entry, and the host entries' return code and error text.  Shapes
(tests/gridfree_cases.py): N in {2, 3, 4, 5, 8, 9, 16} -- the one-lane, 8-lane and block eigen kernels and every root group
size --, M in {1, min(N - 1, 3)}, 19 items (one full wave of the 16-items-per-wave forms and a ragged tail) with an all-zero
and an all-NaN item, and one smoothed pipeline shape.  Running a shape also asserts that the pipeline's angles equal the
chained blocks' bit for bit in both estimator modes (gridfree_cases.run_bits)."""
import os

import numpy as np
import pytest

import gridfree_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gridfree_chain_bits.npz"))
INPUTS = {k[3:]: GOLDEN[k] for k in GOLDEN.files if k.startswith("in/")}


def test_the_inputs_are_the_seeded_ones():
    fresh = cases.make_inputs()
    assert sorted(fresh) == sorted(INPUTS)
    for k, v in fresh.items():
        assert v.dtype == INPUTS[k].dtype and np.array_equal(v.view(np.uint8), INPUTS[k].view(np.uint8)), k


def test_the_recording_holds_every_shape():
    recorded = {k.split("/")[0] for k in GOLDEN.files} - {"in"}
    assert recorded == {cases.shape_key(*s) for s in cases.ALL_SHAPES}


@pytest.mark.parametrize("N,M,smoothing", cases.ALL_SHAPES, ids=[cases.shape_key(*s) for s in cases.ALL_SHAPES])
def test_bits_equal_the_recording(N, M, smoothing):
    key = cases.shape_key(N, M, smoothing)
    got = cases.run_bits(INPUTS, N, M, smoothing)
    want = {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(key + "/")}
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        if want[name].dtype == np.uint8:
            assert bytes(got[name]).decode() == bytes(want[name]).decode(), (key, name)
        else:
            assert got[name].dtype == np.uint32 and np.array_equal(got[name], want[name]), (key, name)
