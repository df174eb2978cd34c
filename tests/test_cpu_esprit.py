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


# ---- the inputs of tests/test_gpu_esprit_solver.py: what its comparisons rest on, checked where there is no GPU ------------------
@pytest.mark.parametrize("N,m", ref.RECORD_SHAPES)
def test_random_records_are_comparable(N, m):
    """The fixed-seed records: orthonormal, the unused columns NaN, every item solvable by the definition, at most 5 % of
    the items outside the gate (amp <= 1e8, | |c| - 1 | >= 1e-6), and rows that mix angles and NaN among them."""
    Es, rec = ref.random_records(N, m)
    a_ref, st_ref, gamma, c, amp, ok = ref.record_reference(N, m)
    eye = np.einsum("nrk,nrl->nkl", Es.conj(), Es)
    assert np.abs(eye - np.eye(m)[None]).max() <= 1e-13
    r = rec.reshape(-1, N, N, 2)
    assert np.isnan(r[:, m:]).all() and np.array_equal(r[:, :m, :, 0] + 1j * r[:, :m, :, 1], Es.transpose(0, 2, 1))
    share = 1.0 - float(ok.mean())
    mixed = np.isnan(a_ref).any(axis=1) & ~np.isnan(a_ref).all(axis=1)
    print("records N=%d m=%d: gamma >= %.3g, non-comparable share %.4f (cap %.2f), NaN share %.3f, %d of %d rows mix angles "
          "and NaN" % (N, m, gamma.min(), share, ref.NONCOMPARABLE_CAP, np.isnan(a_ref).mean(), mixed.sum(), len(ok)))
    assert len(ok) == 403 and np.all(st_ref == 0)
    assert share <= ref.NONCOMPARABLE_CAP
    assert mixed.sum() >= len(ok) // 4
    for row in a_ref:                                                   # sorted, NaN last
        k = int(np.isnan(row).sum())
        assert not np.isnan(row[:m - k]).any() and np.all(np.diff(row[:m - k]) >= 0)


def test_esprit_from_record_is_the_definition_and_predicts_its_sensitivity():
    """On an item's own signal subspace it returns esprit_item's angles; and amp bounds what a relative perturbation eps of Es
    does to the angles: the change is at most amp * eps (to first order; a factor of 4 is left for the orthonormalisation
    of the perturbed basis and the norm of the random direction)."""
    N, M = 8, 3
    R = ref.covariance(N, ref.ANGLES[(N, M)], 20.0, k=1024, n_items=16)
    rng = np.random.default_rng(5)
    for item in R[:4]:
        want, st, gamma, _ = ref.esprit_item(item, ref.D, M, N)
        Es = ref.signal_subspace(ref.hermitian_from_upper(item, N), M)[0]
        ang, st2, gamma2, c, amp = ref.esprit_from_record(Es, ref.D, M)
        assert st == st2 == 0 and gamma == gamma2 and np.array_equal(ang, want) and ref.comparable(c, amp)
        order = np.argsort(c)[::-1]                                    # ascending angle = descending c
        eps = 1e-9
        P = rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M))
        Ep = np.linalg.qr(Es + eps * P / np.linalg.norm(P, 2))[0]
        c2 = ref.esprit_from_record(Ep, ref.D, M)[3]
        moved = np.abs(np.degrees(np.arccos(np.sort(c2)[::-1])) - np.degrees(np.arccos(c[order])))
        assert np.all(moved <= 4.0 * amp[order] * eps), (moved, amp[order] * eps)


def test_analytic_items_are_well_posed_at_every_shape():
    """N = 2 .. 16, M = 1 .. N-1: the gate of the GPU test (gamma >= 1e-4, gap >= 1e-4, amp <= 1e8) holds for all 19 items of
    every shape, and the definition finds the directions the items were built from."""
    worst = [1.0, None, 1.0, None, 0.0]
    for N in range(2, 17):
        for M in range(1, N):
            a, st, gamma, gap, amp, edge = ref.esprit_gated(ref.spread_items(N, M), ref.D, M, N)
            assert np.all(st == 0) and amp.max() <= ref.AMP_MAX and edge.min() >= ref.EDGE_MIN, (N, M)
            assert np.abs(a - np.array(ref.spread_angles(M))[None, :]).max() <= 0.5, (N, M)
            if gamma.min() < worst[0]:
                worst[0:2] = [float(gamma.min()), (N, M)]
            if gap.min() < worst[2]:
                worst[2:4] = [float(gap.min()), (N, M)]
            worst[4] = max(worst[4], float(amp.max()))
    print("analytic items: smallest gamma %.3g at %s, smallest gap %.3g at %s, largest amp %.3g" % tuple(worst))
    assert worst[0] >= 1e-4 and worst[2] >= 1e-4
    for N, phases in ref.OUT_OF_VISIBLE.items():
        a, st, gamma, gap, amp, edge = ref.esprit_gated(ref.out_of_visible_items(N), ref.D, len(phases), N)
        want_nan = sum(abs(p) > 2.0 * np.pi * float(np.float32(ref.D)) for p in phases)
        assert gamma.min() >= 0.57 and gap.min() >= 0.13 and amp.max() < 100.0 and edge.min() >= 0.1, (N, gamma.min(), gap.min())
        assert np.all(np.isnan(a).sum(axis=1) == want_nan) and np.isnan(a[:, len(phases) - want_nan:]).all()


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


def test_record_entry_is_a_test_hook():
    """doa_esprit_linear_array_record_debug: declared in the test header only, exported, bound, refused without a handle."""
    from doa import _lib
    name = "doa_esprit_linear_array_record_debug"
    assert name not in open(os.path.join(ROOT, "include", "doa_hip.h")).read()
    assert re.search(r"DOA_HIP_API\s+int\s+" + name + r"\s*\(", open(os.path.join(ROOT, "include", "doa_hip_test.h")).read())
    assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    buf = np.zeros(32)
    p = buf.ctypes.data
    assert _lib.lib.doa_esprit_linear_array_record_debug(None, 1, p, p, None, p, None) == -1
    assert "record_debug" in _lib.last_error()


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
