"""sc16 (complex int16) streams through autocorrelate: on int16 streams q the covariance is BIT-IDENTICAL to the fc32
handle's on doa.sim.from_sc16(q, scale) = float32(q) * float32(scale), on every route of the covariance kernel (include/
doa_hip.h, DOA_SAMPLE_SC16): the wave kernel N <= 8 in pair-load and scalar form, the read-once overlap path, the matrix
core kernel 8 < N <= 16 in both forms (+ its forward-backward kernel), the fused antenna correction, odd K; host and device
entries; the format switched back and forth on one handle; every error case of the setter."""
import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
from doa.sim import from_sc16, to_sc16

pytestmark = pytest.mark.gpu

S15 = 2.0 ** -15


def _sc16_streams(N, T, seed, level=0.25, scale=S15):
    """int16 [N, T, 2]: tones + noise at `level` of full scale."""
    x = doa.sim.make_streams(N, T, [57.3, 121.0][: 1 + (N > 2)], 0.5, snr_db=10.0, seed=seed)
    x = x / np.abs(x).max() * level * 32767 * scale
    return to_sc16(x, scale)


def _device(arrays, offset):
    """One device buffer per stream, the stream starting `offset` bytes past a 256-byte boundary; (pointers, buffers)."""
    ptrs, keep = [], []
    for a in arrays:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = torch.empty(raw.size + 512, dtype=torch.uint8, device="cuda")
        base = (-buf.data_ptr()) % 256 + offset
        buf[base:base + raw.size].copy_(torch.from_numpy(raw))
        ptrs.append(buf.data_ptr() + base)
        keep.append(buf)
    return ptrs, keep


def _gains(N, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.5, N) * np.exp(1j * rng.uniform(-np.pi, np.pi, N))).astype(np.complex64)


def _cov_dev(h, n, ptrs):
    out = torch.empty((n, h.inputs ** 2), dtype=torch.complex64, device="cuda")
    h.work_dev(n, ptrs, out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _pair(N, K, ovl, fb, n, q, scale=S15, form="vec", gains=None):
    """(sc16 covariance, fc32 covariance on the widened samples), both from work_dev with matching alignment classes."""
    x = from_sc16(q, scale)
    off16, off32 = {"vec": (0, 0), "offset": (4, 8), "odd_s": (0, 0)}[form]
    a16 = doa.autocorrelate(N, K, ovl, fb)
    a16.set_input_format("sc16", scale)
    a32 = doa.autocorrelate(N, K, ovl, fb)
    if gains is not None:
        a16.fuse_antenna_correction(gains)
        a32.fuse_antenna_correction(gains)
    p16, k16 = _device([q[k] for k in range(N)], off16)
    p32, k32 = _device([x[k] for k in range(N)], off32)
    r16, r32 = _cov_dev(a16, n, p16), _cov_dev(a32, n, p32)
    del k16, k32
    return r16, r32


def _span(K, ovl, n):
    return (n - 1) * (K - ovl) + K


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 9, 12, 16])
@pytest.mark.parametrize("form", ["vec", "offset", "odd_s"])
def test_every_route_bit_identical(N, form):
    K = 1023 if form == "odd_s" else 1024                 # S = K: odd S forces the scalar form
    n = 37
    fb = N % 2
    q = _sc16_streams(N, _span(K, 0, n), seed=N)
    r16, r32 = _pair(N, K, 0, fb, n, q, form=form, gains=_gains(N) if N in (3, 8, 12) else None)
    assert np.array_equal(r16, r32)
    assert np.abs(r16).max() > 0


@pytest.mark.parametrize("N", [2, 4, 8])
@pytest.mark.parametrize("K,ovl", [(2048, 512), (1000, 300)])
@pytest.mark.parametrize("fb,gain", [(0, False), (1, True)])
@pytest.mark.parametrize("form", ["vec", "offset"])
def test_overlap_read_once_path_bit_identical(N, K, ovl, fb, gain, form):
    """K = 2048 / 512: the flowgraph shape; K = 1000 / 300: K is not a multiple of S = 700, r = 300 even -> still the
    read-once path in the vector form (pieces A_j, B_j of unequal length)."""
    n = 29
    q = _sc16_streams(N, _span(K, ovl, n), seed=100 + N)
    r16, r32 = _pair(N, K, ovl, fb, n, q, form=form, gains=_gains(N) if gain else None)
    assert np.array_equal(r16, r32)


@pytest.mark.parametrize("N,K,ovl", [(4, 1025, 1), (4, 1025, 0), (12, 1025, 1), (12, 1021, 0), (6, 333, 0)])
@pytest.mark.parametrize("fb", [0, 1])
def test_odd_k_bit_identical(N, K, ovl, fb):
    n = 19
    q = _sc16_streams(N, _span(K, ovl, n), seed=K + N)
    for form in ("vec", "offset"):
        r16, r32 = _pair(N, K, ovl, fb, n, q, form=form)
        assert np.array_equal(r16, r32), form


@pytest.mark.parametrize("scale", [S15, 1.0 / 32767, 1.0])
@pytest.mark.parametrize("N", [4, 16])
def test_scales_bit_identical(scale, N):
    n = 23
    q = _sc16_streams(N, _span(1024, 0, n), seed=7, scale=scale)
    for form in ("vec", "offset"):
        r16, r32 = _pair(N, 1024, 0, 1, n, q, scale=scale, form=form)
        assert np.array_equal(r16, r32), form


@pytest.mark.parametrize("N", [4, 8, 16])
@pytest.mark.parametrize("scale", [S15, 1.0])
def test_full_scale_and_zero_streams(N, scale):
    n, K = 9, 512
    T = _span(K, 0, n)
    rng = np.random.default_rng(N)
    q = rng.choice(np.array([32767, -32767, -32768], np.int16), size=(N, T, 2))
    r16, r32 = _pair(N, K, 0, 0, n, q, scale=scale)
    assert np.array_equal(r16, r32)
    z = np.zeros((N, T, 2), np.int16)
    r16, r32 = _pair(N, K, 0, 1, n, z, scale=scale)
    assert np.array_equal(r16, r32) and not np.any(r16)


@pytest.mark.parametrize("N,K,ovl,fb", [(4, 1024, 0, 0), (4, 2048, 512, 1), (3, 1000, 300, 0), (16, 256, 32, 1)])
def test_host_entry_equals_fc32_and_device_entry(N, K, ovl, fb):
    n = 33
    q = _sc16_streams(N, _span(K, ovl, n), seed=N + K)
    x = from_sc16(q)
    a16 = doa.autocorrelate_sc16(N, K, ovl, fb)
    assert a16.in_sig == [(np.int16, 2)] * N
    a32 = doa.autocorrelate(N, K, ovl, fb)
    r16 = np.empty((n, N * N), np.complex64)
    r32 = np.empty((n, N * N), np.complex64)
    a16.general_work(n, [q[k] for k in range(N)], [r16])
    a32.general_work(n, [x[k] for k in range(N)], [r32])
    assert np.array_equal(r16, r32)
    flat = np.empty_like(r16)                                     # flat 2n int16 streams are the same samples
    a16.general_work(n, [q[k].reshape(-1) for k in range(N)], [flat])
    assert np.array_equal(flat, r16)
    # the device entry on the slab layout the library recommends (int16 streams)
    dev = doa.sim.stream_slab_torch([torch.from_numpy(q[k]).cuda() for k in range(N)])
    assert all(t.dtype == torch.int16 and t.shape == q[k].shape for k, t in enumerate(dev))
    assert np.array_equal(_cov_dev(a16, n, [t.data_ptr() for t in dev]), r16)
    with pytest.raises(TypeError):
        a16.general_work(n, [x[k] for k in range(N)], [r16])     # complex arrays are not sc16 streams


def test_format_switch_on_one_handle_equals_fresh_handles():
    N, K, ovl, fb, n = 4, 2048, 512, 1, 21
    q = _sc16_streams(N, _span(K, ovl, n), seed=5)
    x = from_sc16(q)
    p16, k16 = _device([q[k] for k in range(N)], 0)
    p32, k32 = _device([x[k] for k in range(N)], 0)
    fresh32 = _cov_dev(doa.autocorrelate(N, K, ovl, fb), n, p32)
    h = doa.autocorrelate(N, K, ovl, fb)
    assert np.array_equal(_cov_dev(h, n, p32), fresh32)
    h.set_input_format("sc16")
    assert h.input_format == "sc16" and h.scale == S15
    r16 = _cov_dev(h, n, p16)
    assert np.array_equal(r16, fresh32)
    h.set_input_format("fc32")
    assert h.scale == 1.0
    assert np.array_equal(_cov_dev(h, n, p32), fresh32)
    # the host entry follows the handle's format as well
    out = np.empty((n, N * N), np.complex64)
    h.set_input_format("sc16", S15)
    h.general_work(n, [q[k] for k in range(N)], [out])
    assert np.array_equal(out, fresh32)
    del k16, k32


def test_setter_and_alignment_errors():
    from doa import _lib
    N, K, n = 4, 256, 4
    h = doa.autocorrelate(N, K, 0, 0)
    fn = _lib.lib.doa_autocorrelate_set_input_format
    for fmt, scale in [(2, 1.0), (-1, 1.0), (1, float("nan")), (1, float("inf")), (1, 0.0), (1, -S15), (0, S15),
                       (0, 2.0), (0, float("nan"))]:
        assert fn(h._h, fmt, scale) == -1, (fmt, scale)
        assert "set_input_format" in _lib.last_error()
    for blk in (doa.music_pipeline(N, K, 0, 0, 0.5, 1, 64, 8), doa.root_pipeline(N, K, 0, 0, 0.5, 1, 8)):
        f = blk._set_format
        assert f(blk._h, 1, float("nan")) == -1 and f(blk._h, 0, 0.5) == -1 and f(blk._h, 7, 1.0) == -1
        assert f(blk._h, 1, S15) == 0 and f(blk._h, 0, 1.0) == 0
    with pytest.raises(ValueError):
        h.set_input_format("cs8")
    with pytest.raises(doa.DoaError):
        h.set_input_format("sc16", -1.0)
    with pytest.raises(doa.DoaError):
        doa.autocorrelate_sc16(N, K, 0, 0, scale=0.0)
    assert h.input_format == "fc32"                                # a rejected call leaves the format as it was
    # sc16 device streams must be 4-byte aligned; the message names the stream
    q = _sc16_streams(N, K * n, seed=1)
    h.set_input_format("sc16")
    ptrs, keep = _device([q[k] for k in range(N)], 0)
    ptrs[2] += 2
    out = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    with pytest.raises(doa.DoaError) as ei:
        h.work_dev(n, ptrs, out.data_ptr())
    assert ei.value.status == -1 and "input stream 2" in str(ei.value) and "4-byte" in str(ei.value)
    ptrs[2] -= 2
    ptrs[0] += 4                                                   # 4-byte aligned: accepted (scalar form)
    h.work_dev(n, ptrs, out.data_ptr())
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("N,K,ovl,fb", [(4, 1024, 0, 0), (4, 2048, 512, 1), (12, 512, 64, 1)])
def test_oracle_anchor(N, K, ovl, fb):
    """One direct anchor beside the bit-identity: the fp64 evaluation of the reference's formula on the widened samples,
    within test_gpu_autocorrelate.py's bar."""
    n = 16
    q = _sc16_streams(N, _span(K, ovl, n), seed=9)
    a = doa.autocorrelate_sc16(N, K, ovl, fb)
    R = np.empty((n, N * N), np.complex64)
    a.general_work(n, [q[k] for k in range(N)], [R])
    R64 = oracle.autocorrelate(from_sc16(q), K, ovl, fb, n, precision="f64")
    assert np.abs(R - R64).max() <= 2e-6 * np.abs(R64).max()
