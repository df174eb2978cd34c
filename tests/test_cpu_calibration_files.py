"""CPU tests of the calibration-file side of the library: the two writers (doa_write_phase_config,
doa_write_antenna_calib), the three saver blocks on host arrays (the reference's own numpy reductions, restated in
calibration_ref.py) and the argument checks of the phase-offset estimator, which must reject bad arguments before they look
for a device.  No device is needed by anything here."""
import os
import re

import numpy as np
import pytest

import doa
import calibration_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_floats(n, seed):
    """normals scaled over 1e-6 .. 1e3, no exact zeros"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    assert np.all(v != 0)
    return v


def test_estimator_create_rejects_bad_arguments_before_the_device():
    for args in [(1, 0), (17, 0), (0, 8192), (2, -1), (4, -8192)]:
        with pytest.raises(doa.DoaError) as ei:
            doa.twinrx_phase_offset_est(*args)
        assert "no HIP device" not in str(ei.value), args
        assert "phase_offset_est" in str(ei.value)


def test_estimator_without_a_device_fails_like_every_block():
    if doa.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(doa.DoaError) as ei:
        doa.twinrx_phase_offset_est(4, 8192)
    assert "no CPU fallback" in str(ei.value)


def test_header_documents_the_new_entries():
    text = open(os.path.join(ROOT, "include", "doa_hip.h")).read()
    for name in ("doa_phase_offset_est_create", "doa_phase_offset_est_reset", "doa_phase_offset_est_set_input_format",
                 "doa_phase_offset_est_work", "doa_phase_offset_est_work_dev", "doa_phase_offset_est_estimate",
                 "doa_phase_offset_est_estimate_dev", "doa_calib_mean_work", "doa_calib_mean_work_dev",
                 "doa_calib_mean_complex_work", "doa_calib_mean_complex_work_dev", "doa_write_phase_config",
                 "doa_write_antenna_calib"):
        assert re.search(r"DOA_HIP_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in doa._lib.SIGNATURES
    assert doa._lib.lib.doa_hip_abi_version() == 1


def test_phase_file_round_trip_is_exact(tmp_path):
    v = _random_floats(1000, 1)
    path = str(tmp_path / "phases.cfg")
    doa.write_phase_config(path, v)
    back = np.array(doa.read_phase_config(path), dtype=np.float64)
    assert back.shape == v.shape and np.array_equal(back.astype(np.float32), v)
    assert len(open(path).read().splitlines()) == 1000
    doa.write_phase_config(path, v[:3])                                # truncates
    assert len(open(path).read().splitlines()) == 3


def test_antenna_file_round_trip_is_exact(tmp_path):
    g, p = _random_floats(1000, 2), _random_floats(1000, 3)
    path = str(tmp_path / "antenna.cfg")
    doa.write_antenna_calib(path, g, p)
    rows = [line.split() for line in open(path).read().splitlines()]
    assert len(rows) == 1000 and all(len(r) == 2 for r in rows)
    assert np.array_equal(np.array([float(r[0]) for r in rows]).astype(np.float32), g)
    assert np.array_equal(np.array([float(r[1]) for r in rows]).astype(np.float32), p)


def test_a_zero_phase_is_written_although_the_reference_reader_drops_it(tmp_path):
    path = str(tmp_path / "z.cfg")
    doa.write_phase_config(path, [0.5, 0.0, -1.25])
    assert open(path).read().splitlines() == ["0.5", "0", "-1.25"]
    assert doa.read_phase_config(path) == [0.5, -1.25]                 # python/phase_correct_hier.py:33-45


def test_unwritable_paths_raise_the_reference_text(tmp_path):
    bad = str(tmp_path / "no_such_dir" / "x.cfg")
    with pytest.raises(ValueError, match="Configuration " + re.escape(bad) + ", not writable"):
        doa.write_phase_config(bad, [1.0])
    with pytest.raises(ValueError, match="Configuration " + re.escape(bad) + ", not valid"):
        doa.write_antenna_calib(bad, [1.0], [0.0])
    with pytest.raises(ValueError, match=", not writable"):
        doa.findmax_and_save(16, 3, bad)
    with pytest.raises(ValueError, match=", not writable"):
        doa.average_and_save(16, 3, bad)
    with pytest.raises(ValueError, match=", not valid"):
        doa.save_antenna_calib(4, bad)
    with pytest.raises(ValueError, match=", not valid"):
        doa.save_antenna_calib(4)                                      # the reference's default file name ""


def test_constructors_truncate_the_file(tmp_path):
    for make in (lambda p: doa.findmax_and_save(8, 2, p), lambda p: doa.average_and_save(8, 2, p),
                 lambda p: doa.save_antenna_calib(2, p, 8)):
        path = tmp_path / "old.cfg"
        path.write_text("1.0\n2.0\n")
        make(str(path))
        assert path.read_text() == ""


@pytest.mark.parametrize("cls,restate", [(doa.findmax_and_save, ref.findmax), (doa.average_and_save, ref.average)])
def test_phase_savers_on_host_arrays_match_the_restatement(tmp_path, cls, restate):
    rng = np.random.default_rng(5)
    n_in, samples = 3, 1000
    streams = [rng.uniform(-6.2, 6.2, 1500).astype(np.float32) for _ in range(n_in)]
    streams[1][1200] = 100.0                                           # beyond the first `samples`: must not be seen
    path = str(tmp_path / "p.cfg")
    snk = cls(samples, n_in, path)
    assert snk.output_multiple() == samples
    assert snk.work(streams) == -1                                     # "stop the flowgraph"
    want = restate(streams, samples)
    assert np.array_equal(snk.values, want)
    assert np.array_equal(np.array(doa.read_phase_config(path), dtype=np.float32), want)
    # the reference's own text (str of a numpy float) parses to the same numbers
    assert [np.float32(t) for t in ref.phase_file_text(want).split()] == list(want)


def test_save_antenna_calib_averages_all_items_not_only_samples_to_average(tmp_path):
    rng = np.random.default_rng(6)
    N, n = 4, 300
    mag = rng.uniform(0.2, 1.0, (n, N)).astype(np.float32)
    ph = rng.uniform(-3.0, 3.0, (n, N)).astype(np.float32)
    path = str(tmp_path / "a.cfg")
    snk = doa.save_antenna_calib(N, path, samples_to_average=100)
    assert snk.output_multiple() == 100
    assert snk.work([mag, ph]) == -1
    g, p = ref.save_antenna_calib(mag, ph, N)                         # over all 300 items
    assert np.array_equal(snk.gains, g) and np.array_equal(snk.phases, p)
    assert not np.array_equal(g, ref.save_antenna_calib(mag[:100], ph[:100], N)[0])
    rows = np.array([[float(t) for t in line.split()] for line in open(path).read().splitlines()])
    assert np.array_equal(rows[:, 0].astype(np.float32), g) and np.array_equal(rows[:, 1].astype(np.float32), p)
