"""CPU tests of the source-count feature: the fp64 reference of the criterion itself (tests/source_count_ref.py) pinned on
hand-computed cases, the constructor's argument validation (before the device is touched) and the GRC descriptor."""
import math
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import source_count_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_on_one_source_over_a_flat_floor():
    # l = (1, 1, 1, 10), N = 4, K = 100: equal noise eigenvalues make L_k = 0 for every k >= 1, so MDL_k is the penalty
    # 0.5 k (8 - k) log 100 there; k = 0: L_0 = log 10 - 4 log(13/4)
    vals, count = ref.criterion([1.0, 1.0, 1.0, 10.0], 100, ref.MDL)
    for k in (1, 2, 3):
        assert ref.log_likelihood([1.0, 1.0, 1.0, 10.0], k) == 0.0
    L0 = math.log(10.0) - 4.0 * math.log(13.0 / 4.0)
    want = [-100.0 * L0, 3.5 * math.log(100.0), 6.0 * math.log(100.0), 7.5 * math.log(100.0)]
    assert np.allclose(vals, want, rtol=1e-14, atol=0.0)
    assert np.allclose(vals, [241.20348924, 16.11809565, 27.63102112, 34.53877639], rtol=0, atol=5e-9)
    assert count == 1
    vals, count = ref.criterion([1.0, 1.0, 1.0, 10.0], 100, ref.AIC)
    assert np.allclose(vals, [-200.0 * L0, 14.0, 24.0, 30.0], rtol=1e-14, atol=0.0) and count == 1


def test_reference_aic_and_mdl_part_on_a_weak_second_source():
    # one dominant eigenvalue and one a factor 1.5 over the floor, K = 100: AIC's lighter penalty (24 against 25.397)
    # accepts the second source, MDL's (27.631 against 21.817) does not
    l = [1.0, 1.0, 1.5, 10.0]
    mdl, k_mdl = ref.criterion(l, 100, ref.MDL)
    aic, k_aic = ref.criterion(l, 100, ref.AIC)
    assert (k_mdl, k_aic) == (1, 2)
    assert np.allclose(mdl, [215.75310962, 21.81678879, 27.63102112, 34.53877639], rtol=0, atol=5e-9)
    assert np.allclose(aic, [431.50621924, 25.39738627, 24.0, 30.0], rtol=0, atol=5e-9)
    # a cap below the answer: the best of what is allowed
    assert ref.criterion(l, 100, ref.AIC, kmax=1)[1] == 1
    # ties go to the smallest k
    assert ref.criterion([2.0, 2.0], 2, ref.AIC)[1] == 0


def test_reference_floor_and_status():
    # rounding-level (negative, tiny) noise eigenvalues of a rank-deficient item are lifted to l_max 2^-40 before the logs
    vals, count = ref.criterion([-1e-9, 1e-20, 1.0, 4.0], 50, ref.MDL)
    floored, count2 = ref.criterion([4.0 * 2.0 ** -40, 4.0 * 2.0 ** -40, 1.0, 4.0], 50, ref.MDL)
    assert np.array_equal(vals, floored) and count == count2 == 2
    assert np.all(np.isfinite(vals))
    # status -1: no positive eigenvalue, or anything non-finite
    assert ref.criterion([0.0, 0.0, 0.0], 50, ref.MDL) == (None, -1)
    assert ref.criterion([-3.0, -2.0], 50, ref.AIC) == (None, -1)
    assert ref.criterion([1.0, float("nan"), 2.0], 50, ref.MDL) == (None, -1)
    assert ref.criterion([1.0, 2.0, float("inf")], 50, ref.MDL) == (None, -1)


def test_reference_reads_the_upper_triangle_only():
    rng = np.random.default_rng(3)
    N = 5
    X = rng.standard_normal((N, 40)) + 1j * rng.standard_normal((N, 40))
    A = (X @ X.conj().T / 40).astype(np.complex64)
    item = A.reshape(-1, order="F").copy()
    dirty = A.copy()
    dirty[np.tril_indices(N, -1)] = 1e3 + 7j
    dirty[np.diag_indices(N)] += 5j              # imaginary parts of the diagonal are not part of the matrix either
    c0, e0, _ = ref.source_count(item[None, :], N, 40, ref.MDL)
    c1, e1, _ = ref.source_count(dirty.reshape(-1, order="F")[None, :], N, 40, ref.MDL)
    assert np.array_equal(e0, e1) and np.array_equal(c0, c1)
    assert np.allclose(e0[0], np.linalg.eigvalsh(A.astype(np.complex128)), rtol=1e-6)
    bad = item.copy()
    bad[1 + 3 * N] = np.nan                      # (row 1, col 3): upper triangle
    c2, e2, d2 = ref.source_count(bad[None, :], N, 40, ref.MDL)
    assert c2[0] == -1 and np.all(np.isnan(e2)) and d2[0]


def test_source_count_validation_happens_in_create():
    import doa
    bad = [(1, 64, "mdl", None), (17, 64, "mdl", 3), (4, 1, "mdl", 3), (4, 64, 2, 3), (4, 64, "aic", 0), (4, 64, "mdl", 4)]
    for args in bad:
        with pytest.raises(doa.DoaError) as ei:
            doa.source_count(*args)
        assert "no HIP device" not in str(ei.value), args      # rejected on the arguments, before the device
    with pytest.raises(ValueError):
        doa.source_count(4, 64, "bic", 3)


def test_entries_are_exported():
    import doa
    from doa import _lib
    assert doa.source_count.__name__ == "source_count"
    for cls, names in ((doa.MUSIC_lin_array, ("work_counts", "work_dev_counts")), (doa.find_local_max, ("work_counts", "work_dev_counts")),
                       (doa.music_pipeline, ("work_dev_auto",)), (doa.source_count, ("work", "work_dev"))):
        for name in names:
            assert callable(getattr(cls, name))
    assert _lib.lib.doa_hip_abi_version() == 1


def test_grc_descriptor():
    root = ET.parse(os.path.join(ROOT, "gr-doa_amd", "grc", "doa_source_count.xml")).getroot()
    assert root.findtext("key") == "doa_source_count"
    assert root.findtext("import") == "import doa"
    assert root.findtext("make").strip() == "doa.source_count($inputs, $snapshot_size, $method, $max_sources)"
    params = [p.findtext("key") for p in root.findall("param")]
    assert params == ["inputs", "snapshot_size", "method", "max_sources"]
    assert [c.text for c in root.findall("check")] == ["$inputs > 1", "$snapshot_size > 1", "$inputs > $max_sources"]
    ports = lambda tag: [(p.findtext("type"), p.findtext("vlen")) for p in root.findall(tag)]
    assert ports("sink") == [("complex", "$inputs*$inputs")]
    assert ports("source") == [("int", None), ("float", "$inputs")]
    assert root.findtext("category") == "DoA" and root.findtext("doc").strip()
