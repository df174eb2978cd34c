"""CPU tests of doa.focus_covariance: doa.rss_focusing_matrices (the C library's host routine, a Newton iteration for the polar
factor) against the numpy statement by singular value decomposition (tests/focus_ref.py), its refusals, the C entries'
argument checks, and the case for the block on the reference alone.  No compute on a device.

The case (focus_ref.SCENARIOS: one wideband source and its echo of gain 0.8; spacing 0.4 wavelengths at the carrier, sample
rate 0.4 of the carrier, F = 64, Hann, P = 1024, 15 dB, 6 snapshots; the largest angle error over snapshots and sources in
degrees, seeds 1 / 2 / 3), measured with this file:
    scenario     incoherent wideband_music     focused, fan of N angles   focused, second pass     lambda_2 / lambda_1
    echo4        4.38 / 2.75 / 4.73            0.94                       0.23                     focused >= 0.61, bin 5 <= 0.013
    echo4_half   loses a source (50.0)         0.78 / 0.96 / 0.78         0.25 / 0.43 / 0.25
    echo8        1.29 / 1.60 / 1.60            0.41                       0.23 / 0.20 / 0.20
The source and its echo are rank one in every bin, so no per-bin subspace holds two sources; the echo's phase turns across the
band, so the focused covariance has rank two.  The tests run at seed 2 (focus_ref.SEED)."""
import ctypes as C
import functools

import numpy as np
import pytest

import doa
import focus_ref as fr
import wideband_ref as wb
from doa import _lib

DOA_ERR_INVALID_ARG = -1
D = 0.4


# ---- (a) the helper against the SVD statement ------------------------------------------------------------------------------------
def _focus_angles(J):
    return np.array([77.0]) if J == 1 else np.linspace(20.0, 160.0, J)


@pytest.mark.parametrize("N", [2, 3, 4, 8, 16])
def test_helper_is_the_polar_factor_of_the_svd_statement(N):
    worst = unit = ident = 0.0
    for J in sorted({1, N - 2, N, N + 3}):
        if J < 1:
            continue
        ang = _focus_angles(J)
        for F in (16, 64):
            for rho in (0.0, 0.4):
                for first, nb, carrier in ((0, F, 0), (F - 2, 5, 2)):           # the full band; a selection that wraps
                    T = doa.rss_focusing_matrices(D, N, F, ang, first, nb, rho)
                    want = fr.rss_focusing_matrices(D, N, F, ang, first, nb, rho)
                    assert T.shape == (nb, N, N) and T.dtype == np.complex128
                    worst = max(worst, np.abs(T - want).max())
                    unit = max(unit, np.abs(T @ T.conj().transpose(0, 2, 1) - np.eye(N)).max())
                    ident = max(ident, np.abs(T[carrier] - np.eye(N)).max())
                    if rho == 0.0:                                              # every bin is at the carrier's spacing
                        ident = max(ident, np.abs(T - np.eye(N)).max())
    print(f"N = {N}: |T - T_svd| <= {worst:.1e}, |T T^H - I| <= {unit:.1e}, |T_carrier - I| <= {ident:.1e} (1e-12 allowed)")
    assert worst <= 1e-12 and unit <= 1e-12 and ident <= 1e-12


def test_helper_defaults_and_layout():
    """num_bins None is the full band from first_bin, regularization 1e-3; and T_j is the minimiser the header states: no
    unitary matrix near it (T_j exp(iS), S a small Hermitian matrix) nor the identity has a smaller objective."""
    N, F, ang, reg = 4, 16, np.linspace(20.0, 160.0, 3), 1e-3
    T = doa.rss_focusing_matrices(D, N, F, ang, rate_over_carrier=0.4)
    assert T.shape == (F, N, N)
    assert np.array_equal(T, doa.rss_focusing_matrices(D, N, F, list(ang), 0, F, 0.4, reg))
    A0 = fr.steering_at(float(np.float32(D)), N, ang)
    rng = np.random.default_rng(11)
    for j in (3, 11):
        Aj = fr.steering_at(wb.bin_spacing(D, 0.4, F, j), N, ang)

        def objective(U):
            return np.linalg.norm(A0 - U @ Aj) ** 2 + reg * ang.size * np.linalg.norm(np.eye(N) - U) ** 2

        best = objective(T[j])
        assert best < objective(np.eye(N))
        for _ in range(20):
            S = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
            lam, V = np.linalg.eigh(1e-3 * (S + S.conj().T))
            assert objective(T[j] @ (V * np.exp(1j * lam)) @ V.conj().T) >= best


REFUSED = [  # arguments of doa.rss_focusing_matrices after norm_spacing, inputs, fft_len; what the message names
    (dict(focus_angles=[]), "n_focus"),
    (dict(focus_angles=[30.0, float("nan")]), "focus angle 1"),
    (dict(focus_angles=[float("inf"), 30.0]), "focus angle 0"),
    (dict(focus_angles=[60.0], regularization=0.0), "regularization"),
    (dict(focus_angles=[60.0], regularization=-1e-3), "regularization"),
    (dict(focus_angles=[60.0], regularization=float("nan")), "regularization"),
    (dict(focus_angles=[60.0], regularization=float("inf")), "regularization"),
    (dict(focus_angles=[60.0], rate_over_carrier=3.0), "bin 6 "),           # 0.4 (1 + 3 f / 64) > 0.5 first in bin 6
    (dict(focus_angles=[60.0], rate_over_carrier=3.0, first_bin=32, num_bins=8), "bin 32 "),      # 0.4 (1 - 1.5) <= 0
    (dict(focus_angles=[60.0], first_bin=64), "first_bin"),
    (dict(focus_angles=[60.0], num_bins=65), "num_bins"),
    (dict(focus_angles=[60.0], rate_over_carrier=-0.1), "rate_over_carrier"),
]


def test_helper_refusals_name_the_bin_or_the_argument():
    for kw, named in REFUSED:
        with pytest.raises(doa.DoaError) as ei:
            doa.rss_focusing_matrices(D, 4, 64, **kw)
        assert "rss_focusing_matrices" in str(ei.value) and named in str(ei.value), (kw, str(ei.value))
    # the spacing rule as wideband_music's create states it: 0.5 at the carrier is too wide in every bin above it, first in bin 1
    with pytest.raises(doa.DoaError) as ei:
        doa.rss_focusing_matrices(0.5, 4, 64, [60.0], rate_over_carrier=0.4)
    assert "bin 1 " in str(ei.value)
    for args in ((D, 1, 64), (D, 17, 64), (0.0, 4, 64), (0.6, 4, 64), (D, 4, 48)):
        with pytest.raises(doa.DoaError):
            doa.rss_focusing_matrices(*args, [60.0])
    ang, out = np.array([60.0]), np.empty((64, 4, 4), np.complex128)
    fn = _lib.lib.doa_rss_focusing_matrices
    assert fn(D, 4, 64, 0, 64, 0.4, 1, None, 1e-3, out.ctypes.data) == DOA_ERR_INVALID_ARG
    assert fn(D, 4, 64, 0, 64, 0.4, 1, ang.ctypes.data, 1e-3, None) == DOA_ERR_INVALID_ARG
    assert fn(D, 4, 64, 0, 64, 0.4, 1, ang.ctypes.data, 1e-3, out.ctypes.data) == 0


# ---- (b) the case for the block, on the reference alone ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _incoherent_error(name):
    s = fr.SCENARIOS[name]
    _, items = fr.scenario_items(name)
    dB, _, status, _ = wb.wideband_music(items, fr.D, fr.M_USE, s["N"], fr.P_USE, fr.F_USE, rho=fr.RHO)
    assert not status.any()
    return wb.worst_error(wb.peaks(dB, fr.M_USE), s["thetas"])


def test_echo4_needs_focusing():
    s = fr.SCENARIOS["echo4"]
    first, angles, focused, second = fr.two_pass("echo4")
    inc, e1, e2 = _incoherent_error("echo4"), wb.worst_error(first, s["thetas"]), wb.worst_error(second, s["thetas"])
    _, items = fr.scenario_items("echo4")
    r_foc, r_bin = fr.eigenvalue_ratio(focused, s["N"]), fr.eigenvalue_ratio(items[:, 5], s["N"])
    print(f"echo4: incoherent {inc:.2f}, focused with the fan {e1:.2f}, second pass {e2:.2f} degrees (focus angles "
          f"{np.round(angles, 2).tolist()}); lambda_2 / lambda_1 focused >= {r_foc.min():.3f}, bin 5 <= {r_bin.max():.4f}")
    assert inc >= 2.0
    assert e1 <= 1.5
    assert e2 <= 0.5
    assert r_foc.min() >= 0.3 and r_bin.max() <= 0.05


@pytest.mark.parametrize("name, floor", [("echo4_half", 2.0), ("echo8", 1.0)])
def test_half_sample_echoes_need_focusing(name, floor):
    s = fr.SCENARIOS[name]
    first, _, _, second = fr.two_pass(name)
    inc, e1, e2 = _incoherent_error(name), wb.worst_error(first, s["thetas"]), wb.worst_error(second, s["thetas"])
    print(f"{name}: incoherent {inc:.2f}, focused with the fan {e1:.2f}, second pass {e2:.2f} degrees")
    assert inc >= floor
    assert e2 <= 0.5


def test_reference_structure():
    """The numpy statement itself: identities give the weighted mean of H(R), unused bins and the lower triangle do not count,
    and the status words."""
    rng = np.random.default_rng(3)
    n, nb, N = 3, 5, 3
    items = (rng.standard_normal((n, nb, N * N)) + 1j * rng.standard_normal((n, nb, N * N))).astype(np.complex64)
    w = (0.5 + rng.random((n, nb))).astype(np.float32)
    eye = np.broadcast_to(np.eye(N, dtype=np.complex128), (nb, N, N))
    out, st = fr.focus_covariance(items, eye, w)
    want = np.array([sum(w[i, j] * fr.hermitian(items[i, j], N) for j in range(nb)) / w[i].astype(np.float64).sum() for i in range(n)])
    assert not st.any() and np.abs(out.reshape(n, N, N).transpose(0, 2, 1) - want).max() <= 1e-14
    spoiled, w2 = items.copy(), w.copy()
    spoiled[0, 1], w2[0, 1] = np.nan, 0.0                       # NaN in a skipped bin
    spoiled[1, 2, 1] = np.nan                                   # element (1, 0): the lower triangle
    spoiled.imag[1, 3, 4] = np.nan                              # element (1, 1): the diagonal's imaginary part
    spoiled[2, 4, 3] = np.inf                                   # element (0, 1): a used item
    out2, st2 = fr.focus_covariance(spoiled, eye, w2)
    assert st2.tolist() == [0, 0, 3] and np.isnan(out2[2]).all() and np.array_equal(out2[1], out[1]) and np.isfinite(out2[0]).all()
    assert fr.focus_covariance(items, eye, np.zeros((n, nb)))[1].tolist() == [1, 1, 1]


# ---- create and the entries --------------------------------------------------------------------------------------------------------
def test_create_refuses_bad_arguments_before_the_device():
    T = np.broadcast_to(np.eye(4, dtype=np.complex128), (8, 4, 4)).copy()
    bad = T.copy()
    bad[5, 1, 2] = np.nan
    for args, named in (((1, 8, T.ctypes.data), "num_ant_ele"), ((17, 8, T.ctypes.data), "num_ant_ele"), ((4, 0, T.ctypes.data), "num_bins"),
                        ((4, 257, T.ctypes.data), "num_bins"), ((4, 8, None), "NULL"), ((4, 8, bad.ctypes.data), "bin slot 5")):
        assert not _lib.lib.doa_focus_covariance_create(*args), args
        err = _lib.last_error()
        assert err and "focus_covariance" in err and named in err and "no HIP device" not in err, (args, err)
    with pytest.raises(doa.DoaError) as ei:
        doa.focus_covariance(4, 8, bad)
    assert "no HIP device" not in str(ei.value)
    with pytest.raises(ValueError):
        doa.focus_covariance(4, 7, T)                                            # the table's size is checked in Python


def test_valid_arguments_reach_the_device():
    T = doa.rss_focusing_matrices(D, 4, 64, np.linspace(20.0, 160.0, 4), rate_over_carrier=0.4)
    h = _lib.lib.doa_focus_covariance_create(4, 64, T.ctypes.data)
    if doa.device_count() > 0:
        assert h, _lib.last_error()
        _lib.lib.doa_focus_covariance_destroy(h)
    else:
        assert not h and "no CPU fallback" in _lib.last_error(), _lib.last_error()


def test_every_entry_refuses_a_null_handle_and_names_itself():
    buf = np.zeros(4096, np.uint8)                      # never read: the NULL handle is refused first
    p = buf.ctypes.data
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("doa_focus_covariance_work"))
    assert names == ["doa_focus_covariance_work", "doa_focus_covariance_work_dev"]
    for name in names:
        fn = getattr(_lib.lib, name)
        argtypes = _lib.SIGNATURES[name][1]
        assert argtypes[0] is C.c_void_p and argtypes[1] is C.c_int
        for n in (1, 0):
            assert fn(None, n, *([p] * (len(argtypes) - 2))) == DOA_ERR_INVALID_ARG, (name, n)
            assert name[len("doa_"):] in _lib.last_error(), (name, _lib.last_error())
    _lib.lib.doa_focus_covariance_destroy(None)
    assert _lib.lib.doa_focus_covariance_items_total(None) == 0


def test_the_block_is_exported():
    for name in ("focus_covariance", "rss_focusing_matrices"):
        assert hasattr(doa, name)
    assert callable(doa.focus_covariance.for_ula)
