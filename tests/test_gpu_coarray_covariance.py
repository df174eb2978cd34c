"""GPU tests of doa.coarray_covariance against the numpy statement (tests/coarray_ref.py): parity in both modes over layouts,
virtual sizes and item counts around the kernel's tile, the three access forms, isolation of non-finite items, what the C
entries promise, and the chains autocorrelate -> coarray_covariance -> MUSIC / Root-MUSIC / ESPRIT with more sources than
antennas.

The bars.  "toeplitz" mode has no product feeding an addition: BIT FOR BIT the statement.  "smoothed" mode: every real and
imaginary component within 2^-23 max|component of that item's float64 result| of the float64 result -- one float rounding is
2^-24 relative to the component, the component is at most the item's maximum, and a factor two covers the order of the
double arithmetic.  In both modes the mirror is the bitwise conjugate and the diagonal's imaginary parts are +0.0.
The comparisons print their figures before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import coarray_ref as cr
import esprit_ref
import wideband_ref as wb
from doa import _lib

pytestmark = pytest.mark.gpu

DOA_ERR_INVALID_ARG = -1
MODES = ("toeplitz", "smoothed")
ULA16 = tuple(range(16))
ULA16_PERMUTED = (9, 2, 14, 0, 7, 11, 4, 15, 1, 12, 6, 3, 13, 8, 5, 10)
# positions, virtual_size (0: the default)
LAYOUTS = [((0, 1), 0), ((0, 1, 3), 0), ((0, 1, 4, 6), 0), ((6, 0, 4, 1), 0), ((0, 1, 2, 6), 0), ((0, 1, 4, 7, 9), 0),
           ((0, 1, 2, 3, 7, 11), 0), ((0, 1, 4, 10, 12, 15, 17), 0), ((0, 1, 4, 10, 12, 15, 17), 9), (ULA16, 0), (ULA16_PERMUTED, 0)]
N_MANY = 1000


def _id(layout):
    return "p" + "_".join(str(v) for v in layout[0]) + (f"_Lv{layout[1]}" if layout[1] else "")


def tile_range(N, Lv):
    """(least, most) items of one workgroup's tile (coarray_tile_items): most = what 8 KiB of input and 1024 lag slots hold, least
    = what gives each of the 256 threads a pair of output elements; both even.  A launch takes the even number between them
    that spreads its items over four tiles per compute unit."""
    most = min((1024 // (N * N)) & ~1, (1024 // (2 * Lv - 1)) & ~1)
    return min(most, (-(-512 // (Lv * Lv)) + 1) & ~1), most


def tile_items(N, Lv, n):
    least, most = tile_range(N, Lv)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(least, min(most, (-(-n // (4 * cus)) + 1) & ~1))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _random_items(N, n=N_MANY, seed=0):
    """Seeded complex normal entries, NOT Hermitian; the strict lower triangle and the diagonal's imaginary parts hold junk
    (NaN, Inf, large numbers) that must have no effect; read-only."""
    rng = np.random.default_rng([seed, N])
    R = (rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))).astype(np.complex64)     # [item][col][row]
    junk = np.array([np.nan, np.inf, -np.inf, 3e38, -1e30], np.float32)
    for col in range(N):
        k = N - 1 - col
        R.real[:, col, col + 1:] = junk[rng.integers(0, junk.size, (n, k))]
        R.imag[:, col, col + 1:] = junk[rng.integers(0, junk.size, (n, k))]
        R.imag[:, col, col] = junk[rng.integers(0, junk.size, n)]
    R = R.reshape(n, N * N)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _reference(layout, mode):
    """(float64 result, what the block writes) for the N_MANY random items of the layout, computed once, read-only."""
    positions, size = layout
    out64 = cr.coarray64(_random_items(len(positions)), positions, size, mode)
    out = cr.coarray_covariance(_random_items(len(positions)), positions, size, mode)
    out64.setflags(write=False)
    out.setflags(write=False)
    return out64, out


@functools.lru_cache(maxsize=None)
def _block(layout, mode):
    return doa.coarray_covariance(layout[0], layout[1], mode)


def _work_dev(blk, items, offset8=False):
    """work_dev on device buffers; offset8: both bases 8 bytes past a 256-byte boundary (the 8-byte form)."""
    items = np.array(items, order="C")                          # a copy: the cached inputs are read-only
    n, NN, LL = items.shape[0], blk.num_ant_ele ** 2, blk.virtual_size ** 2
    lead = 1 if offset8 else 0
    buf_in = torch.zeros(n * NN + lead, dtype=torch.complex64, device="cuda")
    buf_out = torch.full((n * LL + lead,), -7.0, dtype=torch.complex64, device="cuda")
    assert buf_in.data_ptr() % 256 == 0 and buf_out.data_ptr() % 256 == 0
    buf_in[lead:] = torch.from_numpy(items.reshape(-1)).cuda()
    assert blk.work_dev(n, buf_in.data_ptr() + 8 * lead, buf_out.data_ptr() + 8 * lead, torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    got = buf_out.cpu().numpy()
    assert not lead or got[0] == np.complex64(-7.0)
    return got[lead:].reshape(n, LL)


def _work(blk, items):
    n = items.shape[0]
    out = np.full((n, blk.virtual_size ** 2), -7.0, np.complex64)
    assert blk.work(n, [items], [out]) == n
    return out


def _assert_exactly_hermitian(out, Lv):
    A = out.reshape(-1, Lv, Lv)                                 # [i, col, row]
    d = np.arange(Lv)
    assert _same(A.imag[:, d, d], np.zeros((A.shape[0], Lv), np.float32))         # +0.0, not -0.0
    mirrored, negated = A.imag.transpose(0, 2, 1).copy(), -A.imag
    mirrored[:, d, d] = negated[:, d, d] = 0.0
    assert _same(A.real.transpose(0, 2, 1), A.real) and _same(mirrored, negated)


def _fraction(got, out64):
    """The largest |c - c_ref| over 2^-23 max|component of the item|, over the components of [n, Lv*Lv] items."""
    top = np.maximum(np.abs(out64.real), np.abs(out64.imag)).max(axis=1)[:, None]
    err = np.maximum(np.abs(got.real.astype(np.float64) - out64.real), np.abs(got.imag.astype(np.float64) - out64.imag))
    return float((err / (2.0 ** -23 * top)).max())


# ---- parity and the access forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=_id)
def test_parity_and_access_forms(layout, mode):
    positions, size = layout
    N = len(positions)
    blk = _block(layout, mode)
    Lv = blk.virtual_size
    assert Lv == (size or cr.default_size(positions))
    out64, want = _reference(layout, mode)
    assert np.all(np.isfinite(out64.view(np.float64)))          # the junk is never read
    items = _random_items(N)
    least, most = tile_range(N, Lv)
    assert most + 1 <= N_MANY                   # (counts this small run on tiles of `least` items; test_full_tiles has the others)
    worst = 0.0
    for n in sorted({1, 3, least - 1, least, least + 1, most - 1, most, most + 1, N_MANY}):
        got = _work_dev(blk, items[:n])
        if mode == "toeplitz":
            assert _same(got, want[:n]), (positions, Lv, n)
        else:
            worst = max(worst, _fraction(got, out64[:n]))
        _assert_exactly_hermitian(got, Lv)
        assert _same(_work_dev(blk, items[:n], offset8=True), got), (positions, Lv, n, "8-byte form")
        assert _same(_work(blk, items[:n]), got), (positions, Lv, n, "host entry")
    if mode == "smoothed":
        print(f"{positions} -> {Lv}: at {worst:.3f} of the bound")
        assert worst <= 1.0


def test_a_uniform_layout_returns_a_toeplitz_input():
    rng = np.random.default_rng(9)
    r = (rng.standard_normal((5, 16)) + 1j * rng.standard_normal((5, 16))).astype(np.complex64)
    r.imag[:, 0] = 0.0
    items = cr.toeplitz_of(r.astype(np.complex128)).astype(np.complex64).transpose(0, 2, 1).reshape(5, 256)
    assert _same(_work_dev(_block((ULA16, 0), "toeplitz"), items), items)


def test_more_tiles_than_the_grid_holds():
    """20 001 items of the 16-element array are 5001 tiles of four, past the grid cap of four workgroups per compute unit: the
    grid-stride rounds, with a last tile of one item."""
    layout = (ULA16_PERMUTED, 0)
    assert tile_range(16, 16) == (2, 4) and tile_items(16, 16, 20001) == 4
    items = np.tile(_random_items(16), (21, 1))[:20001]
    want = np.tile(_reference(layout, "toeplitz")[1], (21, 1))[:20001]
    assert _same(_work_dev(_block(layout, "toeplitz"), items), want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2]], ids=_id)
def test_full_tiles(layout, mode):
    """Enough items that the launch takes tiles of the largest size (256 items of N = 2, 64 of N = 4), one tile minus one,
    one tile and one tile plus one more than fill the grid; every item has the bits it has in a small batch."""
    positions, size = layout
    N, blk = len(positions), _block(layout, mode)
    least, most = tile_range(N, blk.virtual_size)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = 4 * cus * (most - 2) + 1                             # the smallest count that spreads into tiles of `most` items
    assert tile_items(N, blk.virtual_size, full) == most > tile_items(N, blk.virtual_size, full - 1) >= least
    small = _work_dev(blk, _random_items(N))
    for n in (full + most - 2, full + most - 1, full + most):
        reps = -(-n // N_MANY)
        got = _work_dev(blk, np.tile(_random_items(N), (reps, 1))[:n])
        assert _same(got, np.tile(small, (reps, 1))[:n]), (positions, n)


# ---- isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", [LAYOUTS[2], LAYOUTS[6]], ids=_id)
def test_non_finite_items_leave_the_neighbours_alone(layout, mode):
    """Items 0, 17 and 63 of 64 hold NaN, Inf and zeros.  The arithmetic is the definition's by IEEE rules, so the NaN item is
    NaN in every element; of the Inf item no element is finite (a sum of +Inf alone is +Inf: the statement decides which
    elements are Inf and which NaN, and the device agrees); the zero item is zero.  Every other item has the bits it has in
    a batch without them."""
    positions, size = layout
    N, blk = len(positions), _block(layout, mode)
    Lv = blk.virtual_size
    items = np.array(_random_items(N)[:64])
    clean = _work_dev(blk, items)
    items[0] = np.nan + 1j * np.nan
    items[17] = np.inf + 1j * np.inf
    items[63] = 0.0
    got = _work_dev(blk, items)
    want = cr.coarray_covariance(items, positions, size, mode)
    assert np.isnan(got[0]).all()
    assert not (np.isfinite(got[17].real) & np.isfinite(got[17].imag)).any()
    if mode == "toeplitz":
        for part in (np.real, np.imag):
            assert np.array_equal(np.isnan(part(got[17])), np.isnan(part(want[17])))
            assert np.array_equal(np.isposinf(part(got[17])), np.isposinf(part(want[17])))
    assert np.all(got[63] == 0.0) and _same(got[63], want[63])
    others = [i for i in range(64) if i not in (0, 17, 63)]
    assert _same(got[others], clean[others])
    _assert_exactly_hermitian(got[others + [63]], Lv)


# ---- what the entries promise ----------------------------------------------------------------------------------------------------
def test_zero_items_refusals_and_use_after_a_failed_call():
    layout = LAYOUTS[2]
    blk = doa.coarray_covariance(*layout, "smoothed")
    items = _random_items(4)[:5]
    want = _work_dev(_block(layout, "smoothed"), items)
    untouched = np.full((2, 49), -7.0, np.complex64)
    assert blk.work(0, [items], [untouched]) == 0 and np.all(untouched == -7.0)
    assert blk.work_dev(0, 0, 0, torch.cuda.current_stream()) == 0
    d_in = torch.from_numpy(np.array(items)).cuda()
    d_out = torch.full((5, 49), -7.0, dtype=torch.complex64, device="cuda")
    for args in ((-1, d_in.data_ptr(), d_out.data_ptr()), (5, 0, d_out.data_ptr()), (5, d_in.data_ptr(), 0)):
        with pytest.raises(doa.DoaError) as ei:
            blk.work_dev(*args, torch.cuda.current_stream())
        assert ei.value.status == DOA_ERR_INVALID_ARG and "coarray_covariance_work_dev" in str(ei.value), args
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == -7.0)                  # refused before any launch
    out = np.full((5, 49), -7.0, np.complex64)
    host = _lib.lib.doa_coarray_covariance_work
    for args in ((-1, items.ctypes.data, out.ctypes.data), (5, None, out.ctypes.data), (5, items.ctypes.data, None)):
        assert host(blk._h, *args) == DOA_ERR_INVALID_ARG, args
        assert "coarray_covariance_work" in _lib.last_error()
    assert np.all(out == -7.0)
    assert _same(_work(blk, items), want) and _same(_work_dev(blk, items), want)          # the handle still works


def test_two_handles_on_two_streams():
    la, lb = LAYOUTS[2], LAYOUTS[6]
    a, b = doa.coarray_covariance(*la, "smoothed"), doa.coarray_covariance(*lb, "toeplitz")
    ia, ib = _random_items(4), _random_items(6)
    want_a, want_b = _work_dev(_block(la, "smoothed"), ia), _reference(lb, "toeplitz")[1]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = torch.from_numpy(np.array(ia)).cuda(), torch.from_numpy(np.array(ib)).cuda()
    oa = [torch.full((N_MANY, 49), -7.0, dtype=torch.complex64, device="cuda") for _ in range(4)]
    ob = [torch.full((N_MANY, 144), -7.0, dtype=torch.complex64, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for k in range(4):
        assert a.work_dev(N_MANY, da.data_ptr(), oa[k].data_ptr(), sa) == N_MANY
        assert b.work_dev(N_MANY, db.data_ptr(), ob[k].data_ptr(), sb) == N_MANY
    torch.cuda.synchronize()
    for k in range(4):
        assert _same(oa[k].cpu().numpy(), want_a) and _same(ob[k].cpu().numpy(), want_b), k


# ---- the chains on the device ----------------------------------------------------------------------------------------------------
P = cr.P_USE
STEP = 180.0 / P + 180.0 * 2.0 ** -23       # one grid step, and the float32 rounding of the two locations compared
GRID_FREE_BOUND = 1e-3                      # the Root-MUSIC / ESPRIT parity bound (tests/test_gpu_root_music.py, test_gpu_esprit.py)


@functools.lru_cache(maxsize=None)
def _device_coarray(name):
    """autocorrelate -> coarray_covariance on the scenario's streams: [16, Lv*Lv] complex64."""
    s = cr.SCENARIOS[name]
    N, n = len(s["positions"]), cr.N_SNAP
    x = cr.scenario_streams(name)
    R = np.empty((n, N * N), np.complex64)
    produced, _ = doa.autocorrelate(N, s["K"], 0, 0).general_work(n, [x[k] for k in range(N)], [R])
    assert produced == n
    blk = doa.coarray_covariance(s["positions"])
    out = np.empty((n, blk.virtual_size ** 2), np.complex64)
    assert blk.work(n, [R], [out]) == n
    _assert_exactly_hermitian(out, blk.virtual_size)
    return out


@pytest.mark.parametrize("name", sorted(cr.SCENARIOS))
def test_music_finds_more_sources_than_antennas(name):
    s = cr.SCENARIOS[name]
    M, Lv, n = len(s["thetas"]), cr.default_size(s["positions"]), cr.N_SNAP
    items = _device_coarray(name)
    spec = np.empty((n, P), np.float32)
    assert doa.MUSIC_lin_array(cr.D, M, Lv, P).work(n, [items], [spec]) == n
    val, loc = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
    assert doa.find_local_max(M, P, 0.0, 180.0).work(n, [spec], [val, loc]) == n
    found = np.sort(loc.astype(np.float64), axis=1)
    apart, err = np.abs(found - cr.scenario_music(name)).max(), wb.worst_error(found, s["thetas"])
    print(f"{name}: {len(s['positions'])} antennas, {M} sources: largest distance from the reference chain {apart:.4f} "
          f"(one step {STEP:.4f}), largest error {err:.2f} degrees")
    assert apart <= STEP
    assert err <= 1.0


def test_grid_free_estimators_on_mra4_5():
    s = cr.SCENARIOS["mra4_5"]
    n, items, ref_items = cr.N_SNAP, _device_coarray("mra4_5"), cr.scenario_coarray("mra4_5")
    root_ref = np.sort(oracle.root_music(ref_items, cr.D, 5, 7, "f64").astype(np.float64), axis=1)
    esprit_ang, esprit_st, _, _ = esprit_ref.esprit(ref_items, cr.D, 5, 7)
    esprit_want = np.sort(esprit_ang.astype(np.float64), axis=1)
    assert not esprit_st.any()
    assert wb.worst_error(root_ref, s["thetas"]) <= 1.0 and wb.worst_error(esprit_want, s["thetas"]) <= 1.0    # the reference first
    ang = np.empty((n, 5), np.float32)
    assert doa.rootMUSIC_linear_array(cr.D, 5, 7).work(n, [items], [ang]) == n
    root = np.sort(ang.astype(np.float64), axis=1)
    ang_e, st_e = np.empty((n, 5), np.float32), np.empty(n, np.int32)
    assert doa.esprit_linear_array(cr.D, 5, 7).work(n, [items], [ang_e, st_e]) == n
    esp = np.sort(ang_e.astype(np.float64), axis=1)
    print(f"mra4_5: Root-MUSIC {np.abs(root - root_ref).max():.2e} from the reference (bound {GRID_FREE_BOUND}), "
          f"{wb.worst_error(root, s['thetas']):.2f} degrees from the truth; ESPRIT {np.abs(esp - esprit_want).max():.2e}, "
          f"{wb.worst_error(esp, s['thetas']):.2f}")
    assert np.abs(root - root_ref).max() <= GRID_FREE_BOUND and wb.worst_error(root, s["thetas"]) <= 1.0
    assert not st_e.any()
    assert np.abs(esp - esprit_want).max() <= GRID_FREE_BOUND and wb.worst_error(esp, s["thetas"]) <= 1.0
