"""GPU tests of doa.channel_covariance through the C ABI, against the float64 definition in tests/channel_covariance_ref.py.

Parity bound: |R_hip - R_f64| <= 2e-6 * max|R|, the maximum taken over all bins of the snapshot -- the bound
tests/test_gpu_autocorrelate.py sets for K1; the float32 restatement of the same steps (test_cpu_channel_covariance.py)
measures 1.9e-7 to 2.3e-7, a tenfold margin.  Everything the block promises bit for bit (Hermitian symmetry, the power
port, the bin selection, independence of the call's size and position, sc16 against fc32, the two load routes) is
compared with array_equal on the raw bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import doa
import doa_oracle as oracle
from doa._lib import lib, ptr_array, check

import channel_covariance_ref as ref

pytestmark = pytest.mark.gpu

N_SNAP = 9


def _rand_streams(N, T, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T))).astype(np.complex64)


def _window(name, F):
    if name == "custom":
        return (0.25 + np.random.default_rng(F).random(F)).astype(np.float32)        # random, positive
    return name


_bits = ref.bits


def _run(blk, x, n, power=True):
    """Host entry: (cov [n, num_bins, N, N] complex64 as [i, j, q, p] column-major items, power [n, F])."""
    N = blk.inputs
    cov = np.full((n * blk.num_bins(), N * N), np.nan, np.complex64)
    pw = np.full((n, blk.fft_len), np.nan, np.float32) if power else None
    produced, consumed = blk.general_work(n, [x[k] for k in range(N)], [cov, pw])
    assert produced == n and consumed == n * (blk.snapshot_size - blk.overlap_size)
    return cov.reshape(n, blk.num_bins(), N * N), pw


@functools.lru_cache(maxsize=None)
def _case(N, K, ovl, F, wname):
    """Streams, the block's output on them and the float64 reference: computed once, shared, never modified."""
    x = _rand_streams(N, (N_SNAP - 1) * (K - ovl) + K, seed=K + 7 * N + F)
    w = _window(wname, F)
    blk = doa.channel_covariance(N, K, ovl, F, w)
    cov, pw = _run(blk, x, N_SNAP)
    R64, p64 = ref.channel_covariance(x, K, ovl, F, w, N_SNAP)
    for a in (x, cov, pw, R64, p64):
        a.setflags(write=False)
    return x, cov, pw, R64, p64


# (N, K, overlap, F, window): B = 1, B = 3 (not a multiple of the four waves), one antenna, S = 1, odd S (scalar loads)
CASES = [(2, 64, 0, 16, "rect"), (3, 48, 16, 16, "hann"), (4, 1024, 0, 64, "hann"), (4, 64, 0, 64, "rect"),
         (5, 192, 64, 64, "hamming"), (1, 256, 0, 32, "hann"), (8, 512, 128, 128, "blackman"), (8, 1024, 0, 256, "hann"),
         (7, 96, 95, 32, "rect"), (4, 256, 33, 64, "custom")]


@pytest.mark.parametrize("N,K,ovl,F,wname", CASES)
def test_matches_the_float64_definition(N, K, ovl, F, wname):
    x, cov, pw, R64, p64 = _case(N, K, ovl, F, wname)
    # parity, exactly Hermitian items, power the in-order float sum of the stored diagonals: one helper, shared with the
    # shape sweep (test_gpu_channel_covariance_shapes.py)
    ref.assert_items_match(cov, pw, R64, p64, N, F, label=f"N={N} K={K} overlap={ovl} F={F} {wname}")


def test_bin_selection_wraps_and_keeps_the_power_port():
    N, K, F = 4, 256, 64
    x, cov, pw, _, _ = _case(N, K, 0, F, "hann")
    blk = doa.channel_covariance(N, K, 0, F, "hann")
    blk.set_bins(F - 3, 7)
    assert blk.num_bins() == 7
    assert np.array_equal(blk.bin_frequencies(2.0), np.fft.fftfreq(F)[[61, 62, 63, 0, 1, 2, 3]] * 2.0)
    sel, pw_sel = _run(blk, x, N_SNAP)
    assert np.array_equal(_bits(sel), _bits(cov[:, [61, 62, 63, 0, 1, 2, 3]]))
    assert np.array_equal(_bits(pw_sel), _bits(pw))               # all F bins whatever the selection
    sel2, none = _run(blk, x, N_SNAP, power=False)                # out_power = NULL
    assert none is None and np.array_equal(_bits(sel2), _bits(sel))
    with pytest.raises(doa.DoaError):
        blk.set_bins(F, 1)
    with pytest.raises(doa.DoaError):
        blk.set_bins(0, F + 1)
    assert blk.num_bins() == 7                                     # a refused call leaves the handle as it was


def test_streams_offset_by_one_sample_take_the_scalar_route():
    # stream pointers that are only 8-byte aligned: the raw ABI keeps the caller's offset inside 16 bytes on the device
    N, K, ovl, F = 4, 256, 64, 64
    n, S = 5, K - ovl
    T = (n - 1) * S + K
    src = _rand_streams(N, T, seed=3)
    keep = []
    for k in range(N):
        buf = np.zeros(T + 2, np.complex64)
        off = 1 if buf.ctypes.data % 16 == 0 else 0               # the view starts 8 bytes past a 16-byte boundary
        buf[off:off + T] = src[k]
        keep.append(buf[off:off + T])
    assert all(v.ctypes.data % 16 == 8 for v in keep)
    blk = doa.channel_covariance(N, K, ovl, F, "hann")
    cov = np.empty((n, F, N * N), np.complex64)
    pw = np.empty((n, F), np.float32)
    check(lib.doa_channel_covariance_work(blk._h, n, ptr_array([v.ctypes.data for v in keep]), C.c_void_p(cov.ctypes.data),
                                          C.c_void_p(pw.ctypes.data)))
    R64, _ = ref.channel_covariance(np.stack(keep), K, ovl, F, "hann", n)
    err = np.abs(cov - R64).reshape(n, -1).max(axis=1) / np.abs(R64).reshape(n, -1).max(axis=1)
    assert err.max() <= 2e-6
    # both routes do the same arithmetic in the same order
    aligned, pw_aligned = _run(blk, np.ascontiguousarray(np.stack(keep)), n)
    assert np.array_equal(_bits(cov), _bits(aligned)) and np.array_equal(_bits(pw), _bits(pw_aligned))


def test_items_do_not_depend_on_the_size_of_the_call():
    N, K, F = 2, 64, 16
    x9, cov9, pw9, _, _ = _case(N, K, 0, F, "rect")
    blk = doa.channel_covariance(N, K, 0, F, "rect")
    x300 = np.concatenate([x9, _rand_streams(N, 291 * K, seed=5)], axis=1)       # more workgroups than compute units
    cov300, pw300 = _run(blk, x300, 300)
    assert np.array_equal(_bits(cov300[:N_SNAP]), _bits(cov9)) and np.array_equal(_bits(pw300[:N_SNAP]), _bits(pw9))
    cov1, pw1 = _run(blk, x9, 1)
    assert np.array_equal(_bits(cov1[0]), _bits(cov9[0])) and np.array_equal(_bits(pw1[0]), _bits(pw9[0]))


def test_nine_calls_of_one_snapshot_equal_one_call_of_nine():
    import torch
    N, K, F = 2, 64, 16
    x9, cov9, pw9, _, _ = _case(N, K, 0, F, "rect")
    S = K
    assert (S * 8) % 16 == 0
    blk = doa.channel_covariance(N, K, 0, F, "rect")
    dev = [torch.from_numpy(x9[k].copy()).cuda() for k in range(N)]
    cov = torch.empty((N_SNAP, F, N * N), dtype=torch.complex64, device="cuda")
    pw = torch.empty((N_SNAP, F), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    for i in range(N_SNAP):
        assert blk.work_dev(1, [t.data_ptr() + i * S * 8 for t in dev], cov[i].data_ptr(), pw[i].data_ptr(), st) == 1
    torch.cuda.synchronize()
    assert np.array_equal(_bits(cov.cpu().numpy()), _bits(cov9)) and np.array_equal(_bits(pw.cpu().numpy()), _bits(pw9))


@pytest.mark.parametrize("N,K,ovl,F", [(4, 256, 64, 64), (3, 48, 16, 16)])
def test_sc16_is_bit_identical_to_fc32_on_the_widened_samples(N, K, ovl, F):
    n = N_SNAP
    T = (n - 1) * (K - ovl) + K
    q = np.random.default_rng(K + F).integers(-32768, 32768, size=(N, T, 2), dtype=np.int16)
    blk = doa.channel_covariance(N, K, ovl, F, "hann")
    want, pw_want = _run(blk, doa.sim.from_sc16(q), n)
    blk.set_input_format("sc16", 2.0 ** -15)
    got, pw_got = _run(blk, q, n)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(pw_got), _bits(pw_want))


def test_a_nan_sample_stays_inside_its_snapshot():
    N, K, F = 4, 256, 64
    x, cov, pw, _, _ = _case(N, K, 0, F, "hann")
    bad = x.copy()
    bad[2, 4 * K + 100] = np.nan
    blk = doa.channel_covariance(N, K, 0, F, "hann")
    got, pw_got = _run(blk, bad, N_SNAP)
    assert np.isnan(got[4]).any(axis=1).all() and np.isnan(pw_got[4]).all()       # every bin of item 4
    others = [i for i in range(N_SNAP) if i != 4]
    assert np.array_equal(_bits(got[others]), _bits(cov[others])) and np.array_equal(_bits(pw_got[others]), _bits(pw[others]))


def test_five_emitters_on_four_antennas_on_the_device():
    """channel_covariance -> MUSIC_lin_array -> find_local_max on device buffers: five emitters at different frequencies,
    one more than a 4-element array can separate in the whole-band covariance."""
    import torch
    from channel_covariance_ref import BINS, THETAS, five_emitters
    n, N, K, F, P = 6, 4, 1024, 64, 1024
    x = five_emitters(n)
    dev = [torch.from_numpy(x[k]).cuda() for k in range(N)]
    st = torch.cuda.current_stream()
    front = doa.channel_covariance(N, K, 0, F, "hann")
    music = doa.MUSIC_lin_array(0.5, 1, N, P)
    peak = doa.find_local_max(1, P, 0.0, 180.0)

    def chain(n_items):
        cov = torch.empty((n_items, N * N), dtype=torch.complex64, device="cuda")
        pw = torch.empty((n, F), dtype=torch.float32, device="cuda")
        spec = torch.empty((n_items, P), dtype=torch.float32, device="cuda")
        mx = torch.empty((n_items, 1), dtype=torch.float32, device="cuda")
        am = torch.empty((n_items, 1), dtype=torch.float32, device="cuda")
        assert front.work_dev(n, [t.data_ptr() for t in dev], cov.data_ptr(), pw.data_ptr(), st) == n
        music.work_dev(n_items, cov.data_ptr(), spec.data_ptr(), st)
        peak.work_dev(n_items, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
        torch.cuda.synchronize()
        return am.cpu().numpy().reshape(n, -1), pw.cpu().numpy()

    angles, power = chain(n * F)
    R64, _ = ref.channel_covariance(x, K, 0, F, "hann", n)
    s64 = oracle.music_lin_array(R64[:, BINS].reshape(n * len(BINS), N * N), 0.5, 1, N, P, "f64")
    _, want = oracle.find_local_max(s64.astype(np.float32), 1, P, 0.0, 180.0)
    got = angles[:, BINS]
    assert np.abs(got - want.reshape(n, len(BINS))).max() <= 180.0 / P + 1e-4
    assert np.abs(got - np.asarray(THETAS)[None, :]).max() <= 0.25
    assert (10 * np.log10(power[:, BINS].min(axis=1) / np.median(power, axis=1))).min() >= 20.0
    # the selection writes the same matrices: one bin at a time, the same angles bit for bit
    for j, b in enumerate(BINS):
        front.set_bins(b, 1)
        one, _ = chain(n)
        assert np.array_equal(_bits(one[:, 0]), _bits(got[:, j]))
