"""GPU tests of the steering-table scan that ends in the two-dimensional peak pick (array_scan_peaks2d_kernel, the launch of
music_pipeline's grid mode), through the hook doa_hip_array_grid_debug on supplied full records: the one launch against the two
launches it replaces, bit for bit on the spectrum and the three outputs, and the outputs against the numpy statement
(peaks2d_ref.py) applied to the device's own spectrum, exactly -- on every grid at which the kernel takes another path."""
import functools

import numpy as np
import pytest

import doa
import array_ref as ref
import peaks2d_ref as p2

pytestmark = pytest.mark.gpu

# (n_az, n_el) -> elements: single cells and short rows, a partial and a full wave, the last grid of the 8-item form (1024
# cells) and the first of the 4-item form, the scenarios' grid, the last grid of the 4-item form's 32 KiB size (2048) and
# the first of its 64 KiB size, its last grid (4096) and the first of the 1-item form, the last grid with its row in LDS
# (16384) and the first on the two-launch route
GRIDS = {(1, 1): 3, (1, 5): 4, (2, 3): 3, (64, 1): 4, (65, 1): 8, (63, 3): 3, (32, 32): 8, (41, 25): 4, (72, 18): 16,
         (64, 32): 4, (683, 3): 3, (64, 64): 8, (241, 17): 3, (128, 128): 16, (113, 145): 4}
MS = (1, 2, 3, 16)
AXES = (-10.0, 350.0, 5.0, 95.0)
N_PROJ, K = 6, 64
IDENTITY, ZERO, WITH_NAN, TINY = N_PROJ, N_PROJ + 1, N_PROJ + 2, N_PROJ + 3        # item indices after the projectors


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def pack(X):
    """[n, N, N] Hermitian complex128 -> [n, N^2] float64 full records (csrc/kernels.hpp): [r + r N] = X[r][r]; r < c:
    [r + c N] = Re X[r][c], [c + r N] = Im X[r][c]."""
    n, N, _ = X.shape
    rec = np.zeros((n, N * N), np.float64)
    for c in range(N):
        rec[:, c + c * N] = X[:, c, c].real
        for r in range(c):
            rec[:, r + c * N] = X[:, r, c].real
            rec[:, c + r * N] = X[:, r, c].imag
    return rec


@functools.lru_cache(maxsize=None)
def records(N):
    """[10, N^2] float64, read-only: six noise projectors of random covariance items (array_ref), the identity, an all-zero
    record (Q == 0: the general dB path), a record with a NaN, and the first projector scaled by 2^-60."""
    pos = ref.uca(N)
    x = ref.make_streams(pos, (70.3,), 15.0, N_PROJ * K, seed=100 + N)
    R = np.stack([(x[:, d * K:(d + 1) * K].astype(np.complex128) @ x[:, d * K:(d + 1) * K].astype(np.complex128).conj().T / K)
                  .reshape(-1, order="F") for d in range(N_PROJ)]).astype(np.complex64)
    _, _, X = ref.music(R, ref.planar_table(pos, 4), 1)
    rec = pack(X)
    eye = pack(np.eye(N, dtype=np.complex128)[None])
    nan = rec[1:2].copy(); nan[0, N + 1] = np.nan
    out = np.concatenate([rec, eye, np.zeros_like(eye), nan, rec[:1] * 2.0 ** -60])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table(N, n_az, n_el):
    t = doa.planar_steering_grid(ref.uca(N), n_az, n_el)           # unit modulus
    t.setflags(write=False)
    return t


def run(tab, n_az, n_el, rec, M, fused, wrap, spectrum=True):
    return doa.array_grid_debug(tab, n_az, n_el, rec, M, fused, *AXES, wrap, spectrum)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("n_az,n_el", sorted(GRIDS))
def test_one_launch_equals_the_two_and_the_statement(n_az, n_el, wrap):
    N = GRIDS[(n_az, n_el)]
    tab, rec = table(N, n_az, n_el), records(N)
    want = None
    for M in reversed(MS):
        two = run(tab, n_az, n_el, rec, M, False, wrap)
        one = run(tab, n_az, n_el, rec, M, True, wrap)
        for name, a, b in zip(("spectrum", "value", "azimuth", "elevation"), one, two):
            assert _same(a, b), (n_az, n_el, wrap, N, M, name)
        if want is None:                  # the statement on the device's own spectrum, once: a smaller M is its first columns
            want = p2.find_local_max_2d(two[0], MS[-1], n_az, n_el, *AXES, wrap)
        for name, a, w in zip(("value", "azimuth", "elevation"), one[1:], want):
            assert _same(a, np.ascontiguousarray(w[:, :M])), (n_az, n_el, wrap, N, M, name)
    # angles only: no spectrum pointer, the same three outputs
    lean = run(tab, n_az, n_el, rec, 3, True, wrap, spectrum=False)
    full = run(tab, n_az, n_el, rec, 3, True, wrap)
    assert lean[0] is None and all(_same(a, b) for a, b in zip(lean[1:], full[1:])), (n_az, n_el, wrap)
    # the identity on a unit-modulus table: a constant row, hence one peak, at cell 0
    spec, val, az, el = one
    assert (spec[IDENTITY] == 0.0).all()
    assert val[IDENTITY, 0] == 0.0 and az[IDENTITY, 0] == np.float32(AXES[0]) and el[IDENTITY, 0] == np.float32(AXES[2])
    assert np.isnan(val[IDENTITY, 1:]).all() and np.isnan(az[IDENTITY, 1:]).all() and np.isnan(el[IDENTITY, 1:]).all()
    # every row of a finite record has its maximum at exactly 0 dB, and it is the first value reported
    for k in list(range(N_PROJ)) + [TINY]:
        assert spec[k].max() == 0.0 and val[k, 0] == 0.0, (n_az, n_el, wrap, k)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("n_az,n_el,N", [(12, 6, 4), (72, 18, 8), (128, 16, 3), (128, 66, 4)])
def test_exact_plateaus_report_their_first_cell(n_az, n_el, N, wrap):
    """Neighbouring cells in azimuth, in elevation and across the wrap seam hold IDENTICAL table rows, so their Q and their
    dB agree bit for bit: cells come in 2 x 2 blocks, and the azimuth pairs are (2k - 1, 2k), so that the pair (n_az - 1, 0)
    straddles the seam."""
    base = table(N, n_az // 2, n_el // 2).reshape(n_el // 2, n_az // 2, N)
    e, a = np.meshgrid(np.arange(n_el), np.arange(n_az), indexing="ij")
    tab = np.ascontiguousarray(base[e // 2, ((a + 1) % n_az) // 2].reshape(n_az * n_el, N))
    rec = records(N)
    one = run(tab, n_az, n_el, rec, 16, True, wrap)
    two = run(tab, n_az, n_el, rec, 16, False, wrap)
    grid = one[0].reshape(-1, n_el, n_az)
    assert _same(grid[:, 0::2], grid[:, 1::2]) and _same(grid[:, :, 1:-1:2], grid[:, :, 2::2]) and _same(grid[:, :, -1], grid[:, :, 0])
    want = p2.find_local_max_2d(two[0], 16, n_az, n_el, *AXES, wrap)
    for name, x, y, w in zip(("value", "azimuth", "elevation"), one[1:], two[1:], want):
        assert _same(x, y) and _same(x, w), (n_az, n_el, N, wrap, name)
    assert _same(one[0], two[0])
    # every reported cell is the first of its block: an even elevation index and an odd azimuth index, or column 0 -- the
    # lower flat index of the seam pair (n_az - 1, 0); without the wrap that pair are two lone columns
    az_axis, el_axis = p2.axis(AXES[0], AXES[1], n_az), p2.axis(AXES[2], AXES[3], n_el)
    firsts_az = set(az_axis[(slice(1, -1, 2) if wrap else slice(1, None, 2))].tolist()) | {float(az_axis[0])}
    assert (one[1][:N_PROJ, 0] == 0.0).all()
    for k in range(rec.shape[0]):
        found = ~np.isnan(one[1][k])
        assert set(one[2][k, found].tolist()) <= firsts_az and set(one[3][k, found].tolist()) <= set(el_axis[0::2].tolist()), (k, wrap)


@pytest.mark.parametrize("n_az,n_el,sizes", [(32, 32, (1, 7, 8, 9, 63, 64, 65, 257)), (72, 18, (1, 3, 4, 5))])
def test_prefixes_of_a_batch_give_the_bits_of_the_full_batch(n_az, n_el, sizes):
    N, M = 4, 3
    tab, kinds = table(N, n_az, n_el), records(N)
    rng = np.random.default_rng(n_az)
    n = max(sizes)
    rec = np.ascontiguousarray(kinds[rng.integers(0, kinds.shape[0], n)] * rng.uniform(0.5, 2.0, (n, 1)))
    full = run(tab, n_az, n_el, rec, M, True, True)
    two = run(tab, n_az, n_el, rec, M, False, True)
    assert all(_same(a, b) for a, b in zip(full, two)), (n_az, n_el)
    for k in sizes:
        part = run(tab, n_az, n_el, rec[:k], M, True, True)
        assert all(_same(p, f[:k]) for p, f in zip(part, full)), (n_az, n_el, k)
        lean = run(tab, n_az, n_el, rec[:k], M, True, True, spectrum=False)
        assert all(_same(p, f[:k]) for p, f in zip(lean[1:], full[1:])), (n_az, n_el, k, "angles only")
