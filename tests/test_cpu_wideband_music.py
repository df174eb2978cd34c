"""CPU tests of doa.wideband_music: the float64 reference (tests/wideband_ref.py) against the oracle, the use case the block
exists for on the reference alone, doa_wideband_bin_spacing, and the C entries' argument checks.  No compute on a device.

The use case (wideband_ref.SCENARIOS; spacing 0.4 wavelengths at the carrier, sample rate 0.4 of the carrier, Hann, P = 1024,
seed 1; the largest angle error over the snapshots, in degrees), measured with this file:
    scenario   whole-band autocorrelate -> MUSIC   bins combined, one spacing   bins combined, per-bin spacing
    "two"      1.33                                0.96                         0.12
    "four"     3.57                                3.22                         0.23
    "split"    power_sum finds both sources within 0.25; null_mean puts the source at 110 at 108.1 .. 109.5 (off by 0.49 .. 1.89)
    "two" under power_sum, per snapshot: 0.08, 0.47, 0.45, 0.8, 35.1 (a source lost to the luckiest bin), 0.43; null_mean 0.12
The "split" sources are band-limited and scaled back to unit power (wideband_ref.make_streams); without that scaling power_sum
misses 50 degrees by 0.61 on one snapshot."""
import ctypes as C
import functools

import numpy as np
import pytest

import doa
import doa_oracle as oracle
import wideband_ref as wb
from doa import _lib

DOA_ERR_INVALID_ARG = -1


@functools.lru_cache(maxsize=None)
def _scenario(name):
    return wb.scenario_items(name)


@functools.lru_cache(maxsize=None)
def _errors(name, rho, combine):
    """Per snapshot and source |found - true| of the reference on the scenario ([n, sources], degrees)."""
    s = wb.SCENARIOS[name]
    _, items = _scenario(name)
    dB, _, status, _ = wb.wideband_music(items, wb.D, s["M"], s["N"], wb.P_USE, s["F"], rho=rho, combine=combine)
    assert not status.any()
    return np.abs(wb.peaks(dB, len(s["thetas"])) - np.sort(s["thetas"])[None, :])


def _whole_band_error(name):
    s = wb.SCENARIOS[name]
    x, _ = _scenario(name)
    R = oracle.autocorrelate(x, s["K"], 0, 0, s["n"], precision="f64").astype(np.complex64)
    dB = oracle.music_lin_array(R, wb.D, len(s["thetas"]), s["N"], wb.P_USE, "f64")
    return wb.worst_error(wb.peaks(dB, len(s["thetas"])), s["thetas"])


def test_reference_is_the_oracle_for_one_bin_at_the_carrier():
    """rho = 0 and one bin: Q is oracle.music_lin_array's to 1e-12 of its maximum (the two form the same phases in a different
    order of multiplication); the row differs from the oracle's float64 row only by the definition's q = (float) Q, two
    float32 roundings in the ratio: 2 * 2^-24 * 10 / ln 10 = 5.2e-7 dB."""
    N, M, F, P = 4, 2, 64, 257
    _, items = _scenario("two")
    for f in (3, 40):
        dB, Q, status, _ = wb.wideband_music(items[:, f:f + 1], wb.D, M, N, P, F, first_bin=f, num_bins=1, rho=0.0)
        s64, q64, _ = oracle.music_lin_array(items[:, f], wb.D, M, N, P, "f64", return_parts=True)
        assert not status.any()
        assert np.abs(Q - q64).max() <= 1e-12 * np.abs(q64).max()
        assert np.abs(dB - s64).max() <= 5.2e-7 + 1e-12
        assert np.all(dB.max(axis=1) == 0.0)


def test_bin_spacing_is_the_formula():
    d32 = float(np.float32(0.4))
    for F in (16, 64, 256):
        nu = np.fft.fftfreq(F)
        for f in (0, 1, F // 2 - 1, F // 2, F // 2 + 1, F - 1):
            want = d32 * (1.0 + nu[f] * 0.4)
            got = doa.wideband_bin_spacing(0.4, 0.4, F, f)
            assert abs(got - want) <= 2.0 ** -52 * want, (F, f, got, want)            # one rounding of a double
            assert got == wb.bin_spacing(0.4, 0.4, F, f)
    # the sign convention of numpy.fft.fftfreq: bin F/2 is -0.5
    assert doa.wideband_bin_spacing(0.4, 0.4, 64, 32) == d32 * (1.0 - 0.5 * 0.4)
    assert doa.wideband_bin_spacing(0.4, 0.0, 64, 17) == d32
    assert np.isnan(doa.wideband_bin_spacing(0.4, 0.4, 64, 64)) and np.isnan(doa.wideband_bin_spacing(0.4, 0.4, 64, -1))


@pytest.mark.parametrize("name, cap, floor", [("two", 0.5, 0.75), ("four", 0.5, 2.5)])
def test_per_bin_spacing_is_what_finds_a_wideband_source(name, cap, floor):
    per_bin = _errors(name, wb.RHO, "null_mean").max()
    one_spacing = _errors(name, 0.0, "null_mean").max()
    whole = _whole_band_error(name)
    print(f"{name}: whole band {whole:.2f}, one spacing {one_spacing:.2f}, per-bin spacing {per_bin:.2f} degrees")
    assert per_bin <= cap
    assert whole >= floor and one_spacing >= floor


def test_split_band_needs_the_power_sum():
    ps = _errors("split", wb.RHO, "power_sum")
    nm = _errors("split", wb.RHO, "null_mean")
    print(f"split: power_sum worst {ps.max():.2f}; null_mean misses 110 by {nm[:, 1].min():.2f} .. {nm[:, 1].max():.2f} degrees")
    assert ps.max() <= 0.5
    assert nm[:, 1].max() >= 0.75


def test_full_band_sources_need_the_null_mean():
    ps = _errors("two", wb.RHO, "power_sum").max(axis=1)            # per snapshot
    nm = _errors("two", wb.RHO, "null_mean")
    print(f"two: power_sum per snapshot {np.round(ps, 2).tolist()}; null_mean worst {nm.max():.2f} degrees")
    assert ps.max() >= 0.4
    assert nm.max() <= 0.5


# ---- create and the entries ---------------------------------------------------------------------------------------------------
#        norm_spacing, num_targets, num_ant_ele, pspectrum_len, fft_len, first_bin, num_bins, rate_over_carrier, combine
GOOD = (0.4, 2, 4, 1024, 64, 0, 64, 0.4, 0)
BAD = [
    (0.4, 0, 4, 1024, 64, 0, 64, 0.4, 0), (0.4, 4, 4, 1024, 64, 0, 64, 0.4, 0), (0.4, 2, 17, 1024, 64, 0, 64, 0.4, 0),    # M, N
    (0.0, 2, 4, 1024, 64, 0, 64, 0.4, 0), (0.6, 2, 4, 1024, 64, 0, 64, 0.0, 0),                                           # d
    (0.4, 2, 4, 0, 64, 0, 64, 0.4, 0), (0.4, 2, 4, 16385, 64, 0, 64, 0.4, 0),                                             # P
    (0.4, 2, 4, 1024, 48, 0, 48, 0.4, 0), (0.4, 2, 4, 1024, 512, 0, 64, 0.4, 0),                                          # F
    (0.4, 2, 4, 1024, 64, -1, 8, 0.4, 0), (0.4, 2, 4, 1024, 64, 64, 8, 0.4, 0),                                           # first_bin
    (0.4, 2, 4, 1024, 64, 0, 0, 0.4, 0), (0.4, 2, 4, 1024, 64, 0, 65, 0.4, 0),                                            # num_bins
    (0.4, 2, 4, 1024, 64, 0, 64, -0.1, 0), (0.4, 2, 4, 1024, 64, 0, 64, float("nan"), 0),                                 # rho
    (0.4, 2, 4, 1024, 64, 0, 64, float("inf"), 0),
    (0.5, 2, 4, 1024, 64, 0, 64, 0.4, 0), (0.4, 2, 4, 1024, 64, 0, 64, 3.0, 0),                                           # d_f
    (0.4, 2, 4, 1024, 64, 0, 64, 0.4, 2), (0.4, 2, 4, 1024, 64, 0, 64, 0.4, -1),                                          # combine
]


def test_create_refuses_bad_arguments_before_the_device():
    for args in BAD:
        assert not _lib.lib.doa_wideband_music_create(*args), args
        err = _lib.last_error()
        assert err and "wideband_music" in err and "no HIP device" not in err, (args, err)
    # the spacing rule names the bin: 0.5 at the carrier is too wide in every bin above it, first in bin 1
    assert not _lib.lib.doa_wideband_music_create(0.5, 2, 4, 1024, 64, 0, 64, 0.4, 0)
    assert "bin 1 " in _lib.last_error()
    # the Python class passes the library's refusal on, and refuses an unknown rule's name itself
    with pytest.raises(doa.DoaError) as ei:
        doa.wideband_music(0.6, 2, 4, 1024, 64)
    assert "no HIP device" not in str(ei.value)
    with pytest.raises(ValueError):
        doa.wideband_music(0.4, 2, 4, 1024, 64, combine="neither")


def test_valid_arguments_reach_the_device():
    """d = 0.4 with rho = 0.4 passes validation in every bin, and so does d = 0.5 over the bins at and below the carrier."""
    for args in (GOOD, (0.5, 2, 4, 1024, 64, 32, 33, 0.4, 1)):
        h = _lib.lib.doa_wideband_music_create(*args)
        if doa.device_count() > 0:
            assert h, _lib.last_error()
            _lib.lib.doa_wideband_music_destroy(h)
        else:
            assert not h and "no CPU fallback" in _lib.last_error(), _lib.last_error()


def test_every_entry_refuses_a_null_handle_and_names_itself():
    buf = np.zeros(4096, np.uint8)                      # never read: the NULL handle is refused first
    p = buf.ctypes.data
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("doa_wideband_music_work"))
    assert names == ["doa_wideband_music_work", "doa_wideband_music_work_counts", "doa_wideband_music_work_dev",
                     "doa_wideband_music_work_dev_counts"]
    for name in names:
        fn = getattr(_lib.lib, name)
        argtypes = _lib.SIGNATURES[name][1]
        assert argtypes[0] is C.c_void_p and argtypes[1] is C.c_int
        for n in (1, 0):
            assert fn(None, n, *([p] * (len(argtypes) - 2))) == DOA_ERR_INVALID_ARG, (name, n)
            assert name[len("doa_"):] in _lib.last_error(), (name, _lib.last_error())
    _lib.lib.doa_wideband_music_destroy(None)
    assert _lib.lib.doa_wideband_music_items_total(None) == 0


def test_the_block_is_exported():
    for name in ("wideband_music", "wideband_bin_spacing"):
        assert hasattr(doa, name)
