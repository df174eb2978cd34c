"""CPU tests of the Capon estimator: the numpy statement (tests/capon_ref.py) has the properties the feature is for -- on
well-conditioned items the literal Cholesky agrees with np.linalg.inv, the spectrum peaks at the true directions, a
rank-deficient covariance needs diagonal loading -- and the parts of the product that need no device (argument validation
in create, the GRC descriptor).  The figures are printed before they are asserted (run with -s)."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import doa_oracle as oracle
import capon_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = list(range(len(ref.TABLE)))


@pytest.mark.parametrize("row", ROWS)
def test_reference_properties(row):
    N, thetas, snr_db, K, delta, d = ref.TABLE[row]
    M = len(thetas)
    R = ref.row_covariance(row)
    cond = ref.condition_numbers(R, N, delta)
    spec, q, W, st = ref.capon(R, d, N, ref.P, delta)
    steer = oracle.music_steering(d, N, ref.P, "f64")
    rel = 0.0
    for i in range(R.shape[0]):
        A, _ = ref.loaded(R[i], N, delta)
        q_chol = oracle.music_null_spectrum(ref.inverse_cholesky(A), steer)
        rel = max(rel, float(np.abs(q_chol / q[i] - 1.0).max()))
    _, loc = oracle.find_local_max(spec, M, ref.P, 0.0, 180.0)
    err = ref.angle_error(loc, thetas)
    print("row %d (N=%d K=%d delta=%g): cond <= %.3g, Cholesky vs inv %.3g relative, max angle error %.3f deg"
          % (row, N, K, delta, cond.max(), rel, err))
    assert np.all(st == 0)
    assert cond.max() <= 1e5
    assert rel <= 1e-10
    assert err <= 0.6


def test_rank_deficient_row_needs_loading():
    """K = 8 snapshots of N = 16 antennas: the sample covariance has rank 8, and without loading every item fails a pivot."""
    N, thetas, snr_db, K, delta, d = ref.TABLE[ref.RANK_DEFICIENT_ROW]
    assert K < N and delta > 0
    R = ref.row_covariance(ref.RANK_DEFICIENT_ROW)
    spec, q, W, st = ref.capon(R, d, N, ref.P, 0.0)
    assert np.all(st == 1), st
    assert np.all(np.isnan(spec))


def test_reference_status_of_the_failure_items():
    for N in (4, 8, 16):
        ones = np.ones(N * N, np.complex64)
        assert ref.status(ones, N, 0.0) == 1 and ref.status(ones, N, 0.5) == 0
        assert ref.status(np.zeros(N * N, np.complex64), N, 0.0) == 1
        assert ref.status(-np.eye(N, dtype=np.complex64).reshape(-1), N, 0.0) == 1
        good = np.array(ref.row_covariance(0 if N == 4 else 2 if N == 8 else 3)[0])
        assert ref.status(good, N, 0.0) == 0
        bad = good.copy(); bad[0 + 1 * N] = np.nan
        assert ref.status(bad, N, 0.0) == 1
        bad = good.copy(); bad[1 + 1 * N] = np.inf
        assert ref.status(bad, N, 0.0) == 1


def test_create_validates_before_the_device():
    import doa
    for args in [(0.5, 1, 64, 0.0), (0.5, 17, 64, 0.0), (0.6, 4, 64, 0.0), (0.5, 4, 0, 0.0), (0.5, 4, 64, -1.0),
                 (0.5, 4, 64, float("nan"))]:
        with pytest.raises(doa.DoaError) as ei:
            doa.capon_lin_array(*args)
        assert ei.value.status == -1 and "no HIP device" not in str(ei.value), args


def test_grc_descriptor():
    root = ET.parse(os.path.join(ROOT, "gr-doa_amd", "grc", "doa_capon_lin_array.xml")).getroot()
    assert root.findtext("key") == "doa_capon_lin_array"
    keys = [p.findtext("key") for p in root.findall("param")]
    assert keys == ["norm_spacing", "inputs", "pspectrum_len", "diagonal_loading"]
    assert root.findtext("make") == "doa.capon_lin_array($norm_spacing, $inputs, $pspectrum_len, $diagonal_loading)"
    checks = [c.text for c in root.findall("check")]
    assert checks == ["$inputs > 1", "$norm_spacing <= 0.5", "$diagonal_loading >= 0"]
    sink, source = root.find("sink"), root.find("source")
    assert sink.findtext("type") == "complex" and sink.findtext("vlen") == "$inputs*$inputs"
    assert source.findtext("type") == "float" and source.findtext("vlen") == "$pspectrum_len"
