"""The calibration workflow end to end on the device: the files phase_correct_hier and antenna_correction read are produced
by this library and make MUSIC right again.

Phase file (reference apps/estimate_X310_TwinRX_constant_phase_offsets_and_save.grc: twinrx_phase_offset_est ->
findmax_and_save): a four-channel front end with constant phase offsets phi; uncorrected, MUSIC is off by tens of degrees; a
pilot capture -> fused estimate -> file -> phase_correct_hier -> fused into the covariance kernel brings it within the 2.0
degrees of the reference's own QA (python/qa_MUSIC_lin_array.py:96,152).

Antenna file (apps/run_calib_lin_array_simulation.grc: autocorrelate -> calibrate_lin_array -> complex_to_magphase ->
save_antenna_calib): per-element gains and phases, the recipe of test_gpu_calibrate.py restated.

The inputs were evaluated with the numpy restatement (calibration_ref.py) and the oracle alone, without a device, before the
bounds below were fixed; the figures are next to the assertions and the tests recompute them."""
import numpy as np
import pytest

import doa
import doa_oracle as oracle
import calibration_ref as ref

pytestmark = pytest.mark.gpu

N, D, K, NSNAP, P = 4, 0.5, 1024, 8, 1024
THETA = 60.0
PHI = np.array([0.7, -2.1, 1.3])
SKIP, SAMPLES = 8192, 4096
STREAM_BOUND = 4 * 2.0 ** -21             # the accuracy condition of the streaming form (test_gpu_phase_offset_est.py)
# |findmax - phi mod 2 pi| of the numpy restatement on exactly these pilot samples: the bias of a maximum over 4096 noisy
# differences at 30 dB (phase noise of a difference ~ 0.032 rad, its maximum ~ 3.8 sigma).  The bound is twice that.
RESTATED_MAX_ERR = 0.1215
PHASE_BOUND = 2 * RESTATED_MAX_ERR
# the same for the circular mean of the restatement, which has no such bias
RESTATED_CIRC_ERR = 4.8e-4
CIRC_BOUND = 2 * RESTATED_CIRC_ERR


def _circ_dist(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))))


def _music_angle(streams, correction=None):
    pipe = doa.music_pipeline(N, K, 0, 0, D, 1, P, NSNAP)
    if correction is not None:
        pipe.fuse_antenna_correction(correction)
    mx, am = np.empty((NSNAP, 1), np.float32), np.empty((NSNAP, 1), np.float32)
    assert pipe.work(NSNAP, [streams[k] for k in range(N)], mx, am) == NSNAP
    return am[:, 0]


def _offset_streams():
    x = doa.sim.make_streams(N, NSNAP * K, [THETA], D, snr_db=30.0, seed=7)
    return x, ref.apply_offsets(x, PHI)


def test_uncorrected_offsets_spoil_music():
    x, xo = _offset_streams()
    assert np.abs(_music_angle(x) - THETA).max() <= 2.0
    got = _music_angle(xo)
    assert np.abs(got - THETA).min() > 2.0                                   # restatement + oracle: off by 49.5 degrees
    _, _, _, loc = oracle.music_pipeline(xo, K, 0, 0, D, 1, P, precision="f64")
    assert np.abs(loc - THETA).min() > 2.0


@pytest.mark.parametrize("which,bound,restated", [(None, PHASE_BOUND, RESTATED_MAX_ERR), ("circ", CIRC_BOUND, RESTATED_CIRC_ERR)])
def test_pilot_capture_to_phase_file_to_corrected_music(tmp_path, which, bound, restated):
    _, xo = _offset_streams()
    pilot = ref.pilot_capture(N, SKIP + SAMPLES, PHI, snr_db=30.0, seed=11)
    # the restatement on these inputs gives the figure the bound is twice of
    diffs = ref.twinrx_phase_offset_est(pilot, SKIP)
    if which is None:
        rest = ref.findmax(diffs, SAMPLES).astype(np.float64)
        rest_err = np.abs(rest - np.mod(PHI, 2 * np.pi)).max()
    else:
        rest, cond = ref.circular_mean64(pilot, SKIP, SAMPLES)
        assert np.all(cond >= 1e-3)
        rest_err = _circ_dist(rest, PHI).max()
    print(f"{which or 'max'}: restatement error {rest_err:.4e} rad (recorded {restated:.4e}, bound {bound:.4e})")
    assert rest_err <= 1.02 * restated and rest_err >= 0.9 * restated

    path = str(tmp_path / "phases.cfg")
    est = doa.twinrx_phase_offset_est(N, SKIP)
    snk = doa.findmax_and_save(SAMPLES, N - 1, path)
    assert snk.from_estimator(est, SKIP + SAMPLES, [pilot[k] for k in range(N)], which=which) == -1
    blk = doa.phase_correct_hier(N, path)
    written = np.array(blk.phases)
    assert np.array_equal(written.astype(np.float32), snk.values)
    print(f"{which or 'max'}: file {written}, truth {np.mod(PHI, 2 * np.pi) if which is None else PHI}")
    # device against the restatement: items 4 / 5 of the estimator's conditions
    if which is None:
        max64 = ref.phase_differences64(pilot, SKIP)[:, :SAMPLES].max(axis=1)
        assert np.abs(written - max64).max() <= STREAM_BOUND
        assert np.all(written >= 0) and np.all(written < 2 * np.pi)
        assert np.abs(written - np.mod(PHI, 2 * np.pi)).max() <= bound
    else:
        assert _circ_dist(written, rest).max() <= 1e-6
        assert _circ_dist(written, PHI).max() <= bound
    # device against the truth
    got = _music_angle(xo, blk)
    print(f"{which or 'max'}: corrected angles {got.min():.3f} .. {got.max():.3f} (truth {THETA})")
    assert np.abs(got - THETA).max() <= 2.0


def test_findmax_from_device_resident_streams_writes_the_same_file(tmp_path):
    import torch
    pilot = ref.pilot_capture(N, SKIP + SAMPLES, PHI, snr_db=30.0, seed=11)
    a, b = str(tmp_path / "host.cfg"), str(tmp_path / "dev.cfg")
    doa.findmax_and_save(SAMPLES, N - 1, a).from_estimator(doa.twinrx_phase_offset_est(N, SKIP), SKIP + SAMPLES,
                                                          [pilot[k] for k in range(N)])
    dev = doa.sim.stream_slab_torch([torch.from_numpy(pilot[k]).cuda() for k in range(N)])
    doa.findmax_and_save(SAMPLES, N - 1, b).from_estimator_dev(doa.twinrx_phase_offset_est(N, SKIP), SKIP + SAMPLES,
                                                              [t.data_ptr() for t in dev])
    assert open(a).read() == open(b).read() and len(open(a).read().splitlines()) == N - 1


def test_average_and_save_reproduces_the_wrap_quirk(tmp_path):
    """Offsets close to pi: the unwrapped difference takes both branches, their mean is near 0 and says nothing about phi.
    The restatement alone (no device) gives means of 0.019, 0.014, 0.010 rad for these inputs, 3.0 to 3.1 rad from the truth."""
    phi = np.array([3.1, -3.12, 3.0])
    pilot = ref.pilot_capture(N, SKIP + SAMPLES, phi, snr_db=30.0, seed=13)
    rest = ref.average(ref.twinrx_phase_offset_est(pilot, SKIP), SAMPLES)
    assert _circ_dist(rest, phi).min() > 0.5
    path = str(tmp_path / "avg.cfg")
    snk = doa.average_and_save(SAMPLES, N - 1, path)
    assert snk.from_estimator(doa.twinrx_phase_offset_est(N, SKIP), SKIP + SAMPLES, [pilot[k] for k in range(N)]) == -1
    got = np.array(doa.read_phase_config(path))
    mean64 = ref.phase_differences64(pilot, SKIP)[:, :SAMPLES].mean(axis=1)
    print(f"average_and_save: device {got}, restatement {rest}, float64 {mean64}, truth {phi}")
    # every difference within the streaming bound of its float64 value, so is their mean; plus the rounding of the mean
    assert np.all(np.abs(got - mean64) <= STREAM_BOUND + ref.ulp32(mean64))
    # numpy's float32 pairwise mean of 4096 values below 2 pi: at most log2(4096 / 128) + 16 + 1 = 22 roundings of 2^-24 relative
    assert np.all(np.abs(got - rest.astype(np.float64)) <= 2 * STREAM_BOUND + 22 * 2.0 ** -24 * 2 * np.pi)
    assert _circ_dist(got, phi).min() > 0.5                                  # the quirk is reproduced, not repaired


# ---- antenna file --------------------------------------------------------------------------------------------------
PILOT, NCAL = 45.0, 16


def _perturbation():
    rng = np.random.default_rng(21)
    gains = np.concatenate([[1.0], rng.uniform(0.3, 1.0, N - 1)])                # music_test_input_gen.m:42-49
    phases = np.concatenate([[1.0], np.exp(-1j * np.pi * rng.uniform(0, 1, N - 1))])
    return gains * phases


def _perturbed_streams(theta, seed, freq, n_snap):
    x = doa.sim.make_streams(N, n_snap * K, [theta], D, snr_db=None, seed=seed, freqs=[freq])
    x = _perturbation()[:, None] * x
    r = np.random.default_rng(seed + 100)
    x = x + 10 ** (-30.0 / 20) * (r.standard_normal(x.shape) + 1j * r.standard_normal(x.shape)) / np.sqrt(2)
    return np.ascontiguousarray(x.astype(np.complex64))


def test_calibration_chain_to_antenna_file_to_corrected_music(tmp_path):
    import torch
    xp = _perturbed_streams(PILOT, 1, 1.0 / 6.0, NCAL)
    # autocorrelate -> calibrate_lin_array -> calib_mean_complex, all on device pointers
    dev = doa.sim.stream_slab_torch([torch.from_numpy(xp[k]).cuda() for k in range(N)])
    R = torch.empty((NCAL, N * N), dtype=torch.complex64, device="cuda")
    C = torch.empty((NCAL, N), dtype=torch.complex64, device="cuda")
    st = torch.cuda.current_stream()
    assert doa.autocorrelate(N, K, 0, 0).work_dev(NCAL, [t.data_ptr() for t in dev], R.data_ptr(), st) == NCAL
    assert doa.calibrate_lin_array(D, N, PILOT).work_dev(NCAL, R.data_ptr(), C.data_ptr(), st) == NCAL
    path = str(tmp_path / "antenna.cfg")
    snk = doa.save_antenna_calib(N, path, NCAL)
    assert snk.from_calibration_dev(NCAL, C.data_ptr(), st) == -1
    c = C.cpu().numpy()
    # the device means against float64 of |c| and angle: hypotf within 1 ulp (|c| <= 1), atan2f within 2 ulp of a value
    # below 4 (2^-21), the mean rounded once
    g64 = np.abs(c.astype(np.complex128)).mean(axis=0)
    p64 = ref.angle64(c).mean(axis=0)
    assert np.all(np.abs(snk.gains - g64) <= 2.0 ** -23 + ref.ulp32(g64))
    assert np.all(np.abs(snk.phases - p64) <= 2.0 ** -21 + ref.ulp32(p64))
    # the host entry of the same kernel gives the same bits, and the file holds them
    host_path = str(tmp_path / "antenna_host.cfg")
    assert doa.save_antenna_calib(N, host_path, NCAL).from_calibration(c) == -1
    assert open(host_path).read() == open(path).read()
    rows = np.array([[float(t) for t in line.split()] for line in open(path).read().splitlines()])
    assert np.array_equal(rows[:, 0].astype(np.float32), snk.gains) and np.array_equal(rows[:, 1].astype(np.float32), snk.phases)
    # the reference's sink on the same items (complex_to_magphase -> numpy.mean) agrees to float32 mean rounding
    rg, rp = ref.save_antenna_calib(np.abs(c), np.angle(c), N)
    assert np.abs(snk.gains - rg).max() <= 1e-6 and np.abs(snk.phases - rp).max() <= 2e-6
    # antenna_correction loads the file: g = (1/gain) exp(-j phase) (csrc/antenna_correction.hip, the reference's formula)
    blk = doa.antenna_correction(N, path)
    want = (1.0 / snk.gains.astype(np.float64)) * np.exp(-1j * snk.phases.astype(np.float64))
    assert np.abs(blk.gains() - want).max() <= 4e-7 * np.abs(want).max()
    # the correction undoes the perturbation up to one common factor, and MUSIC is right again
    prod = blk.gains() * _perturbation()
    assert np.abs(prod / prod[0] - 1).max() <= 0.01
    xs = _perturbed_streams(70.0, 5, 0.0419, NSNAP)
    assert np.abs(_music_angle(xs) - 70.0).min() > 2.0                       # restatement + oracle: off by 20 degrees
    got = _music_angle(xs, blk)
    print(f"antenna file: corrected angles {got.min():.3f} .. {got.max():.3f} (truth 70)")
    assert np.abs(got - 70.0).max() <= 2.0


@pytest.mark.parametrize("Nin,n", [(4, 1000), (16, 37), (1, 5000), (3, 1)])
def test_calib_mean_of_two_float_inputs(Nin, n):
    import torch
    rng = np.random.default_rng(Nin + n)
    mag = rng.uniform(0.1, 2.0, (n, Nin)).astype(np.float32)
    ph = rng.uniform(-3.14, 3.14, (n, Nin)).astype(np.float32)
    g, p = doa.calib_mean(mag, ph, Nin)
    g64, p64 = mag.astype(np.float64).mean(axis=0), ph.astype(np.float64).mean(axis=0)
    assert np.all(np.abs(g - g64) <= ref.ulp32(g64)) and np.all(np.abs(p - p64) <= ref.ulp32(p64))
    # numpy's float32 pairwise mean: at most log2(n / 128) + 16 + 1 <= 23 roundings of 2^-24 relative to the largest value
    rg, rp = ref.save_antenna_calib(mag, ph, Nin)
    assert np.abs(g - rg).max() <= 23 * 2.0 ** -24 * 2.0 and np.abs(p - rp).max() <= 23 * 2.0 ** -24 * 3.14
    # the device entry gives the same bits
    dm, dp = torch.from_numpy(mag).cuda(), torch.from_numpy(ph).cuda()
    out = torch.empty((2, Nin), dtype=torch.float32, device="cuda")
    assert doa.calib_mean_dev(n, Nin, dm.data_ptr(), dp.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                              torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(o[0].view(np.uint32), g.view(np.uint32)) and np.array_equal(o[1].view(np.uint32), p.view(np.uint32))


def test_calib_mean_rejects_bad_arguments_and_empty_input_is_nan():
    with pytest.raises(doa.DoaError):
        doa.calib_mean(np.zeros((2, 17), np.float32), np.zeros((2, 17), np.float32), 17)
    g, p = doa.calib_mean(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), 4)
    assert np.all(np.isnan(g)) and np.all(np.isnan(p))
