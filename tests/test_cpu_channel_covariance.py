"""CPU tests of doa.channel_covariance: the numpy definition (tests/channel_covariance_ref.py) against the time-domain
covariance and on the use case it exists for (five emitters on four antennas), what float32 arithmetic can reach, the
argument checks of the C entries (made before a device is looked for) and the GRC descriptor.  No device compute."""
import ctypes as C
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import doa
import doa_oracle as oracle
from doa import _lib

import channel_covariance_ref as ref
import test_cpu_bin_plan_refusals as refusals
from channel_covariance_ref import BINS, THETAS, five_emitters

DOA_ERR_INVALID_ARG = -1
GRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "grc")


def _rand_streams(N, T, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T))).astype(np.complex64)


@pytest.mark.parametrize("N,K,ovl,F", [(4, 1024, 0, 64), (3, 96, 32, 16), (8, 512, 128, 256)])
def test_rect_window_bins_average_to_the_time_domain_covariance(N, K, ovl, F):
    n = 5
    x = _rand_streams(N, (n - 1) * (K - ovl) + K, seed=F + N)
    R, power = ref.channel_covariance(x, K, ovl, F, "rect", n)
    want = oracle.autocorrelate(x, K, ovl, 0, n, precision="f64")
    # (the oracle returns complex64 items: compare against the float64 formula itself)
    S = K - ovl
    want64 = np.stack([(x[:, i * S:i * S + K].astype(np.complex128) @ x[:, i * S:i * S + K].astype(np.complex128).conj().T / K)
                       .reshape(-1, order="F") for i in range(n)])
    assert np.abs(want64 - want).max() <= 1e-6 * np.abs(want64).max()
    assert np.abs(R.mean(axis=1) - want64).max() <= 1e-12 * np.abs(want64).max()
    assert np.abs(power.mean(axis=1) - np.einsum("ikk->i", want64.reshape(n, N, N)).real).max() <= 1e-12 * np.abs(want64).max() * N


def test_white_noise_gives_its_variance_in_every_bin_for_any_window():
    x = _rand_streams(2, 64 * 4096, seed=1)                       # variance 2 per antenna
    for w in ref.WINDOWS:
        _, power = ref.channel_covariance(x, 64 * 4096, 0, 64, w, 1)
        assert np.abs(power[0] / 2 - 2.0).max() < 0.15


def test_five_emitters_on_four_antennas():
    n = 6
    x = five_emitters(n)
    # the time-domain covariance has no noise subspace: four large eigenvalues
    Rt = oracle.autocorrelate(x, 1024, 0, 0, n, precision="f64")[0].reshape(4, 4, order="F")
    assert np.linalg.eigvalsh(Rt).min() > 1.0
    R, power = ref.channel_covariance(x, 1024, 0, 64, "hann", n)
    worst = 0.0
    for i in range(n):
        for b, th in zip(BINS, THETAS):
            worst = max(worst, abs(ref.music_angle(R[i, b], 0.5, 4) - th))
    margin_db = 10 * np.log10(power[:, BINS].min(axis=1) / np.median(power, axis=1))
    print(f"five emitters: worst direction error {worst:.3f} deg, occupied bins {margin_db.min():.1f} dB over the median bin")
    assert worst <= 0.25
    assert margin_db.min() >= 20.0


@pytest.mark.parametrize("F,K,N", [(16, 64, 2), (64, 1024, 4), (256, 2048, 8)])
def test_float32_restatement_is_within_the_parity_bound(F, K, N):
    n = 3
    x = _rand_streams(N, n * K, seed=F)
    R64, p64 = ref.channel_covariance(x, K, 0, F, "hann", n)
    R32, p32 = ref.channel_covariance_f32(x, K, 0, F, "hann", n)
    err = np.abs(R32 - R64).reshape(n, -1).max(axis=1) / np.abs(R64).reshape(n, -1).max(axis=1)
    print(f"float32 restatement F={F} K={K} N={N}: {err.max():.2e} of max|R|")
    assert err.max() <= 2e-6
    assert np.abs(p32 - p64).max() <= 2e-6 * N * np.abs(R64).max()


def test_round_structures_follow_from_the_round_geometry():
    assert ref.round_structures(16) == [1, 3, 5, 15, 16, 17, 37, 48]
    assert ref.round_structures(32) == [1, 3, 7, 8, 9, 19, 24]
    for F in (64, 128, 256):
        assert ref.round_structures(F) == [1, 3, 4, 5, 10, 12]
    for F in ref.FFT_LENS:
        assert ref.partial_third_round(F) in ref.round_structures(F)
        assert max(ref.round_structures(F)) * F <= 3072


@pytest.mark.parametrize("kind", ["gaussian", "int16"])
@pytest.mark.parametrize("F", ref.FFT_LENS)
def test_float32_restatement_is_within_the_parity_bound_on_the_sweep_grid(F, kind):
    """The yardstick over the grid of test_gpu_channel_covariance_shapes.py: every round structure of F, N = 1, 3 and 8,
    the four named windows, on Gaussian samples and on the sweep's widened int16 samples.  Measured worst figures (of
    max|R| over 396 cases each; the bound is 2e-6): Gaussian 3.7e-7 (F = 256, B = 1, N = 3, blackman), int16 3.5e-7
    (F = 256, B = 1, N = 1, blackman) -- both under half the bound, so the int16 samples are a fair input for it."""
    n = 3
    worst = (0.0, None)
    for N in (1, 3, 8):
        for B in ref.round_structures(F):
            K = B * F
            if kind == "gaussian":
                x = _rand_streams(N, n * K, seed=F + 1000 * N + B)
            else:
                x = doa.sim.from_sc16(ref.sweep_samples(N, F, B, n))
            for w in ref.WINDOWS:
                R64, p64 = ref.channel_covariance(x, K, 0, F, w, n)
                R32, p32 = ref.channel_covariance_f32(x, K, 0, F, w, n)
                err = (np.abs(R32 - R64).reshape(n, -1).max(axis=1) / np.abs(R64).reshape(n, -1).max(axis=1)).max()
                worst = max(worst, (float(err), (N, B, w)))
                assert err <= 2e-6, (N, B, w)
                assert np.abs(p32 - p64).max() <= 2e-6 * N * np.abs(R64).max(), (N, B, w)
    print(f"float32 restatement F={F} {kind}: worst {worst[0]:.2e} of max|R| at (N, B, window) = {worst[1]}")


def _create(inputs, K, ovl, F, window="default"):
    w = np.ones(max(F, 1), np.float32) if isinstance(window, str) else np.asarray(window, np.float32)
    return _lib.lib.doa_channel_covariance_create(inputs, K, ovl, F, None if window is None else w.ctypes.data)


def test_create_refuses_bad_arguments_before_the_device():
    nan_w = np.ones(64, np.float32)
    nan_w[7] = np.nan
    bad = [(0, 1024, 0, 64, None), (9, 1024, 0, 64, None), (4, 960, 0, 48, None), (4, 1024, 0, 512, None),
           (4, 1000, 0, 64, None), (4, 0, 0, 64, None), (4, 1024, 1024, 64, None), (4, 1024, -1, 64, None),
           (4, 1024, 0, 64, nan_w), (4, 1024, 0, 64, np.zeros(64, np.float32)), (17, 1024, 0, 64, None), (4, 1024, 0, 8, None)]
    for args in bad:
        assert not _create(*args), args
        err = _lib.last_error()
        assert err.startswith("channel_covariance") and "no HIP device" not in err, (args, err)
        if 9 <= args[0] <= 16:
            assert "not built" in err, err
        else:
            assert "invalid argument" in err, (args, err)
    with pytest.raises(doa.DoaError):
        doa.channel_covariance(4, 1024, 0, 48)
    with pytest.raises(ValueError):
        doa.channel_covariance(4, 1024, 0, 64, window="kaiser")
    with pytest.raises(ValueError):
        doa.channel_covariance(4, 1024, 0, 64, window=np.ones(32))


def test_valid_create_needs_a_device_and_set_bins_refuses_bad_ranges():
    h = _create(4, 1024, 0, 64)
    if doa.device_count() == 0:
        assert not h and "no CPU fallback" in _lib.last_error()
        return
    assert h
    lib = _lib.lib
    assert lib.doa_channel_covariance_num_bins(h) == 64
    assert lib.doa_channel_covariance_set_bins(h, 61, 7) == 0 and lib.doa_channel_covariance_num_bins(h) == 7
    recorded = refusals.load_fixture()["set_bins"]             # the texts of the library before the rule was shared
    assert len(recorded) == len(refusals.SET_BINS) == 5
    for first, num in refusals.SET_BINS:                        # (-1, 4), (64, 1), (0, 0), (0, 65), (3, -2)
        assert lib.doa_channel_covariance_set_bins(h, first, num) == DOA_ERR_INVALID_ARG
        assert "channel_covariance_set_bins" in _lib.last_error()
        assert [DOA_ERR_INVALID_ARG, _lib.last_error()] == recorded[repr((first, num))]
        assert lib.doa_channel_covariance_num_bins(h) == 7           # the handle is as it was
    lib.doa_channel_covariance_destroy(h)


def test_every_entry_refuses_a_null_handle():
    lib = _lib.lib
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    for name in ("doa_channel_covariance_work", "doa_channel_covariance_work_dev"):
        argtypes = _lib.SIGNATURES[name][1]
        rest = [_lib.ptr_array([p] * 8) if t is not C.c_void_p else p for t in argtypes[2:]]     # never read: the handle is refused first
        for n in (1, 0):
            assert getattr(lib, name)(None, n, *rest) == DOA_ERR_INVALID_ARG
            assert name[len("doa_"):] in _lib.last_error()
    assert lib.doa_channel_covariance_set_bins(None, 0, 1) == DOA_ERR_INVALID_ARG
    assert "channel_covariance_set_bins" in _lib.last_error()
    assert lib.doa_channel_covariance_set_input_format(None, 0, 1.0) == DOA_ERR_INVALID_ARG
    assert "channel_covariance_set_input_format" in _lib.last_error()
    assert lib.doa_channel_covariance_num_bins(None) == DOA_ERR_INVALID_ARG
    assert lib.doa_channel_covariance_history(None) == DOA_ERR_INVALID_ARG
    assert lib.doa_channel_covariance_forecast(None, 1) == DOA_ERR_INVALID_ARG
    assert lib.doa_channel_covariance_input_span(None, 1) == 0
    lib.doa_channel_covariance_destroy(None)


def test_named_windows_match_the_reference_builders():
    from doa.blocks import _periodic_window
    for name in ref.WINDOWS:
        for F in (16, 64, 256):
            assert np.array_equal(_periodic_window(name, F), ref.window(name, F))
    assert ref.window("hann", 64)[0] == 0.0 and ref.window("hann", 64)[32] == 1.0     # periodic: the peak is at F/2


def test_grc_descriptor():
    root = ET.parse(os.path.join(GRC, "doa_channel_covariance.xml")).getroot()
    assert root.findtext("key") == "doa_channel_covariance"
    assert root.findtext("import") == "import doa"
    make = root.findtext("make").strip()
    assert make == "doa.channel_covariance($inputs, $snapshot_size, $overlap_size, $fft_len, $window)"
    params = [p.findtext("key") for p in root.findall("param")]
    assert set(re.findall(r"\$(\w+)", make)) == set(params) and len(params) == 5
    for c in root.findall("check"):
        assert set(re.findall(r"\$(\w+)", c.text)) <= set(params)
    ports = lambda tag: [(p.findtext("type"), p.findtext("vlen"), p.findtext("nports"), p.findtext("optional")) for p in root.findall(tag)]
    assert ports("sink") == [("complex", None, "$inputs", None)]
    assert ports("source") == [("complex", "$inputs*$inputs", None, None), ("float", "$fft_len", None, "1")]
    assert "fft_len items per snapshot" in root.findtext("doc")
