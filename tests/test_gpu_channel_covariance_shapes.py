"""GPU sweep of doa.channel_covariance over every array size, transform length, round structure, sample format and load
route, against the float64 definition and against each other (tests/channel_covariance_ref.py states the grid).

csrc/channel_covariance.hip compiles 8 array sizes x 2 LDS image sizes (F <= 64, F >= 128) x 2 load routes (pair, scalar)
x 2 sample formats (fc32, sc16) = 64 kernels.  test_every_round_structure_format_and_route runs for each N = 1..8 and each
F in {16, 32, 64} (small image) and {128, 256} (large image) the fc32 and the sc16 entry on aligned (pair route) and on
offset (scalar route) pointers: all 64, each at every block count of round_structures(F).

Bounds: the parity bound |R_hip - R_f64| <= 2e-6 max|R| of test_gpu_channel_covariance.py, unchanged; everything else is
compared bit for bit.  Measured worst parity errors on this grid, as a fraction of max|R|:
    float32 restatement on the CPU (test_cpu_channel_covariance.py): 3.7e-7 Gaussian, 3.5e-7 widened int16 samples;
    device (MI355X), worst over N = 1..8 per F: 2.7e-7 (F = 16), 2.7e-7 (32), 3.4e-7 (64), 4.6e-7 (128, at N = 4), 3.9e-7 (256):
    at most 0.23 of the bound, beside the yardstick's 0.19."""
import ctypes as C

import numpy as np
import pytest

import doa
from doa._lib import lib, ptr_array, check

import channel_covariance_ref as ref
from channel_covariance_ref import bits

pytestmark = pytest.mark.gpu

N_SNAP = 3


def _place(samples, off):
    """Every stream in a torch allocation of its own, T + 1 samples long, the data from element `off` on and a NaN (int16:
    32767) in the spare element.  Returns (tensors to keep alive, pointers to the first sample)."""
    import torch
    keep, ptrs = [], []
    for a in samples:
        src = torch.from_numpy(np.ascontiguousarray(a))
        src = torch.view_as_real(src) if src.is_complex() else src                 # [T, 2] float32 or int16
        T = src.shape[0]
        buf = torch.full((T + 1, 2), float("nan") if src.is_floating_point() else 32767, dtype=src.dtype, device="cuda")
        buf[off:off + T].copy_(src)
        assert buf.data_ptr() % 16 == 0
        keep.append(buf)
        ptrs.append(buf.data_ptr() + off * 2 * buf.element_size())
    return keep, ptrs


def _call(blk, ptrs):
    """work_dev on N_SNAP snapshots into NaN-filled outputs: (cov [n, num_bins, N*N], power [n, F]) as numpy arrays."""
    import torch
    N, F = blk.inputs, blk.fft_len
    cov = torch.full((N_SNAP, blk.num_bins(), N * N), float("nan"), dtype=torch.complex64, device="cuda")
    pw = torch.full((N_SNAP, F), float("nan"), dtype=torch.float32, device="cuda")
    assert blk.work_dev(N_SNAP, ptrs, cov.data_ptr(), pw.data_ptr(), torch.cuda.current_stream()) == N_SNAP
    torch.cuda.synchronize()
    return cov.cpu().numpy(), pw.cpu().numpy()


def _same_bits(got, want):
    return np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("F", ref.FFT_LENS)
@pytest.mark.parametrize("N", range(1, 9))
def test_every_round_structure_format_and_route(N, F):
    """For every block count of round_structures(F): fc32 on aligned pointers against float64 and the item contract, then
    fc32 offset by a sample, sc16 aligned and offset, fc32 with only the last stream offset, all bit-identical to it; a
    call with overlap 1 (odd snapshot step) against float64 on its own layout; once per (N, F) the wrapped bin selection.

    The test cannot see which kernel ran; the launcher's rule (doa_channel_covariance_work_dev) is
        vec2 = every pointer a multiple of two samples && (K - overlap) even,
    so off 0 with overlap 0 is the pair route and a stream at off 1, or overlap 1, is the scalar route."""
    worst = 0.0
    for case, B in enumerate(ref.round_structures(F)):
        K = B * F
        q = ref.sweep_samples(N, F, B, N_SNAP)                     # [N, 3 K, 2] int16
        x = doa.sim.from_sc16(q)                                   # the same values, widened by 2^-15
        wname, w = ref.sweep_window(case + N, F)
        tag = f"N={N} F={F} B={B} {wname}"
        R64, p64 = ref.channel_covariance(x, K, 0, F, w, N_SNAP)
        blk = doa.channel_covariance(N, K, 0, F, w)

        fc0, fc0_ptrs = _place(x, 0)
        fc1, fc1_ptrs = _place(x, 1)
        base = _call(blk, fc0_ptrs)                                # fc32, pair route
        worst = max(worst, ref.assert_items_match(*base, R64, p64, N, F, label=tag))
        assert _same_bits(_call(blk, fc1_ptrs), base), f"{tag}: fc32 off 1"
        if N >= 2:                                                 # one misaligned stream: the whole call goes scalar
            assert _same_bits(_call(blk, fc0_ptrs[:-1] + fc1_ptrs[-1:]), base), f"{tag}: fc32, last stream off 1"

        if B == ref.partial_third_round(F):                        # the un-permutation of the bins, for this lg F
            rows = [F - 3, F - 2, F - 1, 0, 1, 2, 3]
            blk.set_bins(F - 3, 7)
            sel, sel_pw = _call(blk, fc0_ptrs)
            assert sel.shape == (N_SNAP, 7, N * N)
            assert np.array_equal(bits(sel), bits(base[0][:, rows])), f"{tag}: bins {rows}"
            assert np.array_equal(bits(sel_pw), bits(base[1])), f"{tag}: power port under a selection"
            blk.set_bins(0, F)

        blk.set_input_format("sc16", 2.0 ** -15)
        sc0, sc0_ptrs = _place(q, 0)
        sc1, sc1_ptrs = _place(q, 1)
        assert _same_bits(_call(blk, sc0_ptrs), base), f"{tag}: sc16 off 0"
        assert _same_bits(_call(blk, sc1_ptrs), base), f"{tag}: sc16 off 1"

        # an odd snapshot step on aligned pointers: the scalar route by step; snapshots 1 and 2 start one sample earlier each
        blk1 = doa.channel_covariance(N, K, 1, F, w)
        R64o, p64o = ref.channel_covariance(x, K, 1, F, w, N_SNAP)
        odd = _call(blk1, fc0_ptrs)
        worst = max(worst, ref.assert_items_match(*odd, R64o, p64o, N, F, label=tag + " overlap 1"))
        assert np.array_equal(bits(odd[0][0]), bits(base[0][0])) and np.array_equal(bits(odd[1][0]), bits(base[1][0])), \
            f"{tag}: snapshot 0 does not depend on the step"
    print(f"N={N} F={F}: worst {worst:.2e} of max|R|, {worst / 2e-6:.3f} of the bound")


def _host(blk, x):
    """The host entry on contiguous streams, NaN-filled outputs."""
    N, F = blk.inputs, blk.fft_len
    cov = np.full((N_SNAP * F, N * N), np.nan, np.complex64)
    pw = np.full((N_SNAP, F), np.nan, np.float32)
    produced, _ = blk.general_work(N_SNAP, [x[k] for k in range(N)], [cov, pw])
    assert produced == N_SNAP
    return cov.reshape(N_SNAP, F, N * N), pw


def _scaled(a, s):
    """a times the float32 s component by component (no complex product: zeros keep their sign)."""
    a = np.ascontiguousarray(a)
    return (a.view(np.float32) * np.float32(s)).view(a.dtype)


@pytest.mark.parametrize("wname", ["rect", "hann"])
@pytest.mark.parametrize("N,F,B", [(4, 64, 5), (8, 256, 3)])
def test_power_of_two_scaling_is_exact(N, F, B, wname):
    K = B * F
    q = ref.sweep_samples(N, F, B, N_SNAP)
    x = doa.sim.from_sc16(q)
    blk = doa.channel_covariance(N, K, 0, F, wname)
    base = _host(blk, x)
    # precondition: no subnormal at the smaller scale, no overflow at the larger one; zeros stay zeros
    for a in (base[0].view(np.float32), base[1]):
        mag = np.abs(a[a != 0]).astype(np.float64)
        assert np.isfinite(a).all() and mag.size and mag.min() * 2.0 ** -40 >= 2.0 ** -126 and mag.max() * 2.0 ** 40 < 2.0 ** 127
    for e in (20, -20):
        got = _host(blk, _scaled(x, 2.0 ** e))
        assert np.array_equal(bits(got[0]), bits(_scaled(base[0], 2.0 ** (2 * e)))), f"samples x 2^{e}: covariance"
        assert np.array_equal(bits(got[1]), bits(_scaled(base[1], 2.0 ** (2 * e)))), f"samples x 2^{e}: power"
    # sc16: the scale is applied once, to the sample at load
    blk.set_input_format("sc16", 2.0 ** -15)
    assert _same_bits(_host(blk, q), base)
    blk.set_input_format("sc16", 1.0)
    raw = _host(blk, q)
    assert np.array_equal(bits(raw[0]), bits(_scaled(base[0], 2.0 ** 30)))
    assert np.array_equal(bits(raw[1]), bits(_scaled(base[1], 2.0 ** 30)))


def _host_views(samples, offsets):
    """Copies of the streams whose first sample lies offsets[k] bytes past a 16-byte boundary."""
    views = []
    for a, want in zip(samples, offsets):
        sb = a[0].nbytes                                           # bytes per sample: 8 (complex64) or 4 (int16 pair)
        buf = np.zeros((a.shape[0] + 16 // sb,) + a.shape[1:], a.dtype)
        lead = ((want - buf.ctypes.data) % 16) // sb
        v = buf[lead:lead + a.shape[0]]
        v[...] = a
        views.append(v)
    assert [v.ctypes.data % 16 for v in views] == list(offsets)
    return views


def _host_raw(blk, views):
    """doa_channel_covariance_work on raw host pointers."""
    N, F = blk.inputs, blk.fft_len
    cov = np.full((N_SNAP, F, N * N), np.nan, np.complex64)
    pw = np.full((N_SNAP, F), np.nan, np.float32)
    assert check(lib.doa_channel_covariance_work(blk._h, N_SNAP, ptr_array([v.ctypes.data for v in views]),
                                                 C.c_void_p(cov.ctypes.data), C.c_void_p(pw.ctypes.data))) == N_SNAP
    return cov, pw


@pytest.mark.parametrize("fmt,offsets", [("sc16", (0, 4, 8, 12)), ("fc32", (0, 8))])
def test_the_host_entry_keeps_the_callers_offset_inside_16_bytes(fmt, offsets):
    """The device copy of a stream starts as many bytes past a 16-byte boundary as the caller's pointer, so the route follows
    the caller's alignment: sc16 offsets 4 and 12 (an odd sample) take the scalar route, 0 and 8 the pair route; fc32 offset
    8 takes the scalar route.  Every placement, the mixed ones included, gives the bits of the aligned run."""
    N, F, B = 3, 32, 9
    K = B * F
    q = ref.sweep_samples(N, F, B, N_SNAP)
    x = doa.sim.from_sc16(q)
    samples = q if fmt == "sc16" else x
    blk = doa.channel_covariance(N, K, 0, F, "hann")
    if fmt == "sc16":
        blk.set_input_format("sc16", 2.0 ** -15)
    R64, p64 = ref.channel_covariance(x, K, 0, F, "hann", N_SNAP)
    aligned = _host_raw(blk, _host_views(samples, (0,) * N))
    ref.assert_items_match(*aligned, R64, p64, N, F, label=f"{fmt} host entry, aligned")
    mixed = [(4, 8, 12), (8, 0, 8)] if fmt == "sc16" else [(8, 0, 8), (0, 0, 8)]
    for offs in [(o,) * N for o in offsets[1:]] + mixed:
        assert _same_bits(_host_raw(blk, _host_views(samples, offs)), aligned), f"{fmt} streams at byte offsets {offs}"
