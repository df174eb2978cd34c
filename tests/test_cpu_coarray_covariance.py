"""CPU tests of doa.coarray_covariance: doa.coarray_lags (the C library's host helper) on known layouts, the refusals of create,
the numpy statement (tests/coarray_ref.py) on exact covariances, and the case for the block on the reference alone.  No
compute on a device.

The case (coarray_ref.SCENARIOS: unit-power complex Gaussian sources, white noise 10 dB below each, spacing 0.5, 16 snapshots,
float64 MUSIC on a 2048-point grid from the complex64 covariance items of oracle.autocorrelate; the largest angle error over
snapshots and sources in degrees at seeds 1 / 2 / 3), measured with this file:
    scenario    positions          sources  samples per snapshot  virtual size  largest angle error
    mra4_5      0 1 4 6            5        4096                  7             0.45 / 0.43 / 0.36
    mra4_6      0 1 4 6            6        8192                  7             0.50 / 0.59 / 0.50
    nested6_8   0 1 2 3 7 11       8        4096                  12            0.23 / 0.39 / 0.27
Every snapshot of every seed shows all its sources.  The tests run at seed 1 (coarray_ref.SEED)."""
import ctypes as C

import numpy as np
import pytest

import doa
import coarray_ref as cr
import doa_oracle as oracle
import esprit_ref
import wideband_ref as wb
from doa import _lib

DOA_ERR_INVALID_ARG = -1
ULA16 = tuple(range(16))
MRA7 = (0, 1, 4, 10, 12, 15, 17)


# ---- the layout helper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positions, size, counts", [
    ((0, 1, 4, 6), 7, [4, 1, 1, 1, 1, 1, 1]),
    ((0, 1, 2, 3, 7, 11), 12, None),
    ((6, 0, 4, 1), 7, [4, 1, 1, 1, 1, 1, 1]),                   # the order does not matter
    ((0, 1, 2, 6), 3, [4, 2, 1]),                               # a hole at lag 3 ends the run
    ((0, 2), 1, [2]),
    (MRA7, 18, None),
    (ULA16, 16, list(range(16, 0, -1))),
    ((-3, 5, -2), 2, [3, 1]),                                   # only differences count
])
def test_coarray_lags(positions, size, counts):
    got_size, got_counts = doa.coarray_lags(positions)
    assert got_size == size and len(got_counts) == size
    assert (got_size, got_counts) == cr.lags(positions)
    if counts is not None:
        assert got_counts == counts


def test_coarray_lags_refusals_and_null_counts():
    fn = _lib.lib.doa_coarray_lags
    p = np.array([0, 1, 4, 6], np.int32)
    size = C.c_int(-1)
    assert fn(p.ctypes.data, 4, C.byref(size), None) == 0 and size.value == 7
    assert fn(None, 4, C.byref(size), None) == DOA_ERR_INVALID_ARG and "positions" in _lib.last_error()
    assert fn(p.ctypes.data, 4, None, None) == DOA_ERR_INVALID_ARG and "contiguous_size" in _lib.last_error()
    for bad, named in (((), "num_ant_ele"), (tuple(range(17)), "num_ant_ele"), ((0, 3, 3), "distinct"), ((0, 256), "255")):
        with pytest.raises(doa.DoaError) as ei:
            doa.coarray_lags(bad)
        assert "coarray_lags" in str(ei.value) and named in str(ei.value), (bad, str(ei.value))
    assert doa.coarray_lags((0, 255))[0] == 1 and doa.coarray_lags((7,)) == (1, [1])
    with pytest.raises(ValueError):
        doa.coarray_lags((0, 1.5))


# ---- create ----------------------------------------------------------------------------------------------------------------------
REFUSED = [  # positions, virtual_size, mode, what the message names
    ((3,), 0, 0, "num_ant_ele"),
    (tuple(range(17)), 0, 0, "num_ant_ele"),
    ((0, 1, 4, 4), 0, 0, "distinct"),
    ((0, 1, 300), 0, 0, "255"),
    ((0, 2, 4), 0, 0, "contiguous size 1"),
    ((0, 1, 4, 6), 1, 0, "virtual_size"),
    ((0, 1, 4, 6), 8, 0, "virtual_size"),
    ((0, 1, 4, 6), -1, 0, "virtual_size"),
    (MRA7, 17, 0, "virtual_size"),
    ((0, 1, 4, 6), 0, 2, "mode"),
    ((0, 1, 4, 6), 0, -1, "mode"),
]


def test_create_refuses_bad_arguments_before_the_device():
    for positions, size, mode, named in REFUSED:
        p = np.array(positions, np.int32)
        assert not _lib.lib.doa_coarray_covariance_create(p.ctypes.data, p.size, size, mode), (positions, size, mode)
        err = _lib.last_error()
        assert err and "coarray_covariance" in err and named in err and "no HIP device" not in err, (positions, size, mode, err)
    assert not _lib.lib.doa_coarray_covariance_create(None, 4, 0, 0) and "NULL" in _lib.last_error()
    with pytest.raises(doa.DoaError) as ei:
        doa.coarray_covariance((0, 1, 4, 6), 8)
    assert "no HIP device" not in str(ei.value)
    with pytest.raises(ValueError):
        doa.coarray_covariance((0, 1, 4, 6), mode="squared")


@pytest.mark.parametrize("positions, size, mode", [((0, 1, 4, 6), 0, "smoothed"), (MRA7, 16, "toeplitz"), ((1, 0), 2, "smoothed")])
def test_valid_arguments_reach_the_device(positions, size, mode):
    if doa.device_count() > 0:
        blk = doa.coarray_covariance(positions, size, mode)
        assert blk.virtual_size == (size or cr.default_size(positions))
        assert blk.in_sig == [(np.complex64, len(positions) ** 2)] and blk.out_sig == [(np.complex64, blk.virtual_size ** 2)]
    else:
        with pytest.raises(doa.DoaError) as ei:
            doa.coarray_covariance(positions, size, mode)
        assert "no CPU fallback" in str(ei.value)


def test_every_entry_refuses_a_null_handle_and_names_itself():
    buf = np.zeros(4096, np.uint8)                      # never read: the NULL handle is refused first
    p = buf.ctypes.data
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("doa_coarray_covariance_work"))
    assert names == ["doa_coarray_covariance_work", "doa_coarray_covariance_work_dev"]
    for name in names:
        fn = getattr(_lib.lib, name)
        argtypes = _lib.SIGNATURES[name][1]
        for n in (1, 0):
            assert fn(None, n, *([p] * (len(argtypes) - 2))) == DOA_ERR_INVALID_ARG, (name, n)
            assert name[len("doa_"):] in _lib.last_error(), (name, _lib.last_error())
    _lib.lib.doa_coarray_covariance_destroy(None)
    assert _lib.lib.doa_coarray_covariance_virtual_size(None) == 0


def test_the_block_is_exported():
    assert hasattr(doa, "coarray_covariance") and callable(doa.coarray_lags)


def test_five_targets_on_four_elements_are_refused():
    """What the feature lifts, pinned: no estimator takes as many sources as it has elements."""
    for make in (lambda: doa.MUSIC_lin_array(cr.D, 5, 4, 64), lambda: doa.rootMUSIC_linear_array(cr.D, 5, 4),
                 lambda: doa.esprit_linear_array(cr.D, 5, 4)):
        with pytest.raises(doa.DoaError) as ei:
            make()
        assert "no HIP device" not in str(ei.value)


# ---- the numpy statement ---------------------------------------------------------------------------------------------------------
def _column_major(R):
    return np.asarray(R).T.reshape(1, -1)


def test_reference_on_an_exact_covariance():
    """For A diag(p) A^H + sigma^2 I of 0, 1, 4, 6 with SIX sources T is the 7-element uniform array's covariance, and the
    smoothed item has exactly six eigenvalues above the noise floor (sigma^2)^2 / 7."""
    thetas, powers, sigma2 = cr.SCENARIOS["mra4_6"]["thetas"], [1.0, 0.7, 1.3, 0.9, 1.1, 0.8], 0.1
    R = cr.exact_covariance(cr.MRA4, thetas, powers, sigma2, cr.D)
    want = cr.exact_covariance(range(7), thetas, powers, sigma2, cr.D)
    r = cr.lag_means(_column_major(R).astype(np.complex128), cr.MRA4, 7)         # (the statement reads complex64 or wider)
    T = cr.toeplitz_of(r)[0]
    assert np.abs(T - want).max() <= 1e-12
    out = cr.coarray64(_column_major(R), cr.MRA4, 7, "smoothed").reshape(7, 7).T
    assert np.abs(out - want @ want.conj().T / 7).max() <= 1e-12
    lam = np.linalg.eigvalsh(out)
    floor = sigma2 ** 2 / 7
    print("eigenvalues over the floor:", np.round(lam / floor, 7).tolist())
    assert int((lam > floor * (1 + 1e-6)).sum()) == 6
    assert lam.min() >= floor * (1 - 1e-9)


def test_reference_structure():
    """The statement itself: a uniform layout and a Toeplitz input come back in toeplitz mode, the order of the streams does
    not matter when the items are permuted with it, the lower triangle and the diagonal's imaginary parts are not read, and
    the output is exactly Hermitian."""
    rng = np.random.default_rng(4)
    r = (rng.standard_normal((3, 5)) + 1j * rng.standard_normal((3, 5))).astype(np.complex64)
    r.imag[:, 0] = 0.0
    T = cr.toeplitz_of(r.astype(np.complex128)).astype(np.complex64)              # [item][row][col]
    items = T.transpose(0, 2, 1).reshape(3, 25)
    assert np.array_equal(cr.coarray_covariance(items, range(5), 5, "toeplitz"), items)
    junk = items.reshape(3, 5, 5).copy()                         # [item][col][row]
    for col in range(5):
        junk[:, col, col + 1:] = np.nan
        junk.imag[:, col, col] = np.inf
    for mode in ("toeplitz", "smoothed"):
        a, b = cr.coarray_covariance(items, range(5), 4, mode), cr.coarray_covariance(junk.reshape(3, 25), range(5), 4, mode)
        assert a.tobytes() == b.tobytes()
        A = a.reshape(3, 4, 4)
        assert np.array_equal(A.real, A.real.transpose(0, 2, 1)) and np.array_equal(A.imag, -A.imag.transpose(0, 2, 1))
        assert not np.signbit(A.imag[:, np.arange(4), np.arange(4)]).any()
    x = rng.standard_normal((4, 64)) + 1j * rng.standard_normal((4, 64))
    R = x @ x.conj().T / 64
    perm = [2, 0, 3, 1]
    a = cr.coarray64(_column_major(R), cr.MRA4, 7, "toeplitz")
    b = cr.coarray64(_column_major(R[np.ix_(perm, perm)]), [cr.MRA4[k] for k in perm], 7, "toeplitz")
    assert np.abs(a - b).max() <= 1e-15


# ---- the case for the block, on the reference alone --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.SCENARIOS))
def test_more_sources_than_antennas(name):
    s = cr.SCENARIOS[name]
    M, N, Lv = len(s["thetas"]), len(s["positions"]), cr.default_size(s["positions"])
    assert M > N - 1 and M < Lv
    dB = oracle.music_lin_array(cr.scenario_coarray(name), cr.D, M, Lv, cr.P_USE, "f64")
    peaks = cr.count_peaks(dB)
    err = wb.worst_error(cr.scenario_music(name), s["thetas"])
    print(f"{name}: {N} antennas, {M} sources, virtual size {Lv}: {peaks.min()}..{peaks.max()} peaks, largest error {err:.2f} degrees")
    assert peaks.min() >= M
    assert err <= 1.0


def test_grid_free_references_on_mra4_5():
    """What the device chains of the GPU tests are compared with must itself meet the cap: float64 Root-MUSIC and ESPRIT on the
    reference's co-array items (measured: 0.45 and 0.45 degrees at seed 1, the default; no other seed was needed)."""
    s = cr.SCENARIOS["mra4_5"]
    items = cr.scenario_coarray("mra4_5")
    root = np.sort(oracle.root_music(items, cr.D, 5, 7, "f64").astype(np.float64), axis=1)
    ang, st, _, _ = esprit_ref.esprit(items, cr.D, 5, 7)
    e_root, e_esprit = wb.worst_error(root, s["thetas"]), wb.worst_error(np.sort(ang.astype(np.float64), axis=1), s["thetas"])
    print(f"mra4_5: float64 Root-MUSIC {e_root:.2f}, ESPRIT {e_esprit:.2f} degrees")
    assert not st.any()
    assert e_root <= 1.0 and e_esprit <= 1.0
