"""CPU tests of the ESPRIT estimator: the numpy statement (tests/esprit_ref.py) agrees with the fp64 Root-MUSIC oracle where
the two methods solve the same problem (one noise vector), finds the true directions, and reports the three unsolvable
items; and the parts of the product that need no device (argument validation in create, the new symbols in header, library
and binding, the GRC descriptor).  The figures are printed before they are asserted (run with -s)."""
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import doa_oracle as oracle
import esprit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,M", [(2, 1), (3, 2), (4, 3), (5, 4), (8, 7)])
def test_reference_agrees_with_root_music_for_one_noise_vector(N, M):
    """M = N - 1: the noise subspace is one vector, Root-MUSIC's polynomial has exactly the signal roots, and both methods
    return the generalised eigenvalues of the same pencil."""
    R = ref.covariance(N, ref.ANGLES[(N, M)], 20.0, k=1024, n_items=16)
    a, st, gamma, gap = ref.esprit(R, ref.D, M, N)
    want = oracle.root_music(R, ref.D, M, N, "f64")
    err = float(np.abs(a.astype(np.float64) - want).max())
    print("N=%d M=%d: ESPRIT vs fp64 Root-MUSIC %.3g deg (bound 1e-3), gamma >= %.3g" % (N, M, err, gamma.min()))
    assert np.all(st == 0)
    assert err <= 1e-3


def test_reference_finds_the_true_directions():
    thetas = (30.0, 123.0)
    R = ref.covariance(4, thetas, 20.0, k=1024, n_items=16)
    a, st, _, _ = ref.esprit(R, ref.D, 2, 4)
    err = float(np.abs(a - np.array(thetas)[None, :]).max())
    print("N=4 M=2 at 20 dB: max angle error %.3f deg (bound 0.5)" % err)
    assert np.all(st == 0) and err <= 0.5


def test_reference_status_of_the_unsolvable_items():
    sing = np.diag([1.0, 1.0, 1.0, 5.0]).astype(np.complex64).reshape(-1)
    a, st, gamma, _ = ref.esprit_item(sing, ref.D, 1, 4)
    assert st == 1 and gamma == 0.0 and np.all(np.isnan(a))
    good = np.array(ref.covariance(4, (30.0, 123.0), 20.0, k=1024, n_items=16)[0])
    assert ref.esprit_item(good, ref.D, 2, 4)[1] == 0
    for item in ref.failure_items(4, good):
        a, st, _, _ = ref.esprit_item(item, ref.D, 1, 4)
        assert st == 1 and np.all(np.isnan(a))
    ang, st = ref.esprit_counts(np.stack([good] * 4), [-1, 0, 2, 4], ref.D, 3, 4)
    assert list(st) == [2, 0, 0, 2]
    assert np.isnan(ang[[0, 1, 3]]).all() and not np.isnan(ang[2, :2]).any() and np.isnan(ang[2, 2])


def test_create_validates_before_the_device():
    """Through the C ABI: NULL and a message for each bad argument, the device untouched."""
    from doa import _lib
    create = _lib.lib.doa_esprit_linear_array_create
    for args, word in [((0.4, 1, 1), "num_ant_ele"), ((0.4, 1, 17), "num_ant_ele"), ((0.4, 0, 4), "num_targets"),
                       ((0.4, 4, 4), "num_targets"), ((0.0, 1, 4), "norm_spacing"), ((0.6, 1, 4), "norm_spacing"),
                       ((float("nan"), 1, 4), "norm_spacing")]:
        assert not create(*args), args
        msg = _lib.last_error()
        assert word in msg and "no HIP device" not in msg, (args, msg)
    import doa
    with pytest.raises(doa.DoaError) as ei:
        doa.esprit_linear_array(0.4, 4, 4)
    assert ei.value.status == -1


def test_set_estimator_is_declared_exported_and_bound():
    from doa import _lib
    header = open(os.path.join(ROOT, "include", "doa_hip.h")).read()
    assert re.search(r"DOA_HIP_API\s+int\s+doa_root_pipeline_set_estimator\s*\(", header)
    assert re.search(r"#define\s+DOA_GRIDFREE_ROOT_MUSIC\s+0\b", header) and re.search(r"#define\s+DOA_GRIDFREE_ESPRIT\s+1\b", header)
    assert re.search(r"#define\s+DOA_ESPRIT_GAMMA_MIN\s+\(1\.0 / 1073741824\.0\)", header) and 2.0 ** 30 == 1073741824.0
    assert hasattr(_lib.lib, "doa_root_pipeline_set_estimator") and "doa_root_pipeline_set_estimator" in _lib.SIGNATURES
    for suffix in ("create", "destroy", "work", "work_dev", "work_counts", "work_dev_counts"):
        name = "doa_esprit_linear_array_" + suffix
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    # a NULL handle is refused on its arguments
    assert _lib.lib.doa_root_pipeline_set_estimator(None, 1) == -1


def test_grc_descriptor():
    root = ET.parse(os.path.join(ROOT, "gr-doa_amd", "grc", "doa_esprit_linear_array.xml")).getroot()
    assert root.findtext("key") == "doa_esprit_linear_array"
    keys = [p.findtext("key") for p in root.findall("param")]
    assert keys == ["norm_spacing", "num_targets", "inputs"]
    assert root.findtext("make") == "doa.esprit_linear_array($norm_spacing, $num_targets, $inputs)"
    checks = [c.text for c in root.findall("check")]
    assert checks == ["$num_targets > 0", "$num_targets < $inputs", "$norm_spacing <= 0.5"]
    sink, source = root.find("sink"), root.find("source")
    assert sink.findtext("type") == "complex" and sink.findtext("vlen") == "$inputs*$inputs"
    assert source.findtext("type") == "float" and source.findtext("vlen") == "$num_targets"
