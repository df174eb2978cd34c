"""GPU tests of what the host entries of the six stream blocks promise (gr-doa_amd/csrc/block_host.hpp), entry by entry; the
counterpart of test_gpu_block_host_contract.py for the blocks that take or give N sample streams:
  (a) the host entry gives bit for bit what the device entry gives on device buffers laid out as the host entry lays them out
      (streams doa_stream_stride_bytes apart in one allocation; outputs at the block's own distance),
  (b) one handle called with 3, 70 and 3 items gives what a fresh handle gives each time (at 70 items the staged buffers grow
      past their 4096-byte floor; the second 3-item call then runs in buffers larger than it needs).  Blocks with a position
      (sim_source: seek, the phase estimator: reset) are put back between the calls,
  (c) 0 items returns 0 and writes nothing; compass_mean is the exception, it runs and writes NaN.  `estimate` has no
      zero-item call (it needs at least one sample): there it is the refusal that must write nothing,
  (d) an absent optional port (channel_covariance's power port; each of estimate's three outputs) leaves the bits of the
      ports that are present as they were,
  (e) a host call whose last input port is NULL returns DOA_ERR_INVALID_ARG, names the port, writes nothing, and leaves the
      handle as it was: its next call gives the fresh handle's bits (for the phase estimator that includes the samples its
      skip still owes).  sim_source has no input port and compass_mean has one pointer, not a port list; neither is in (e),
  (f) a channel_covariance host call from streams whose addresses differ modulo 16 equals the device entry on the same
      offsets.
Shapes are the smallest that exercise the staging: 4 streams (2 as well for the phase estimator, there in sc16), K = 64,
overlap 0 and 16 (the overlapping autocorrelate shape takes the read-once piece path), fft_len 16.  Samples come from one
fixed seed.  Nothing here provokes a device fault: every failing call is refused on the host before any launch."""
import ctypes as C
import functools
import re
import tempfile

import numpy as np
import pytest
import torch

import doa
from doa._lib import last_error, lib, ptr_array

pytestmark = pytest.mark.gpu

N, K, F, M = 4, 64, 16, 2
N_MAX = 70
GROWTH = (3, N_MAX, 3)
SKIP = 2                        # samples the phase estimator drops first: an even number keeps the pair alignment
SENTINEL = -7
DOA_ERR_INVALID_ARG = -1
_C64, _F32, _I16 = np.complex64, np.float32, np.int16


@functools.lru_cache(maxsize=None)
def _samples():
    """(streams [4, 70 * 64] complex64, the same as sc16 [4, 70 * 64, 2] int16, angle items [70, 2] float32), read-only."""
    rng = np.random.default_rng(20250217)
    T = N_MAX * K
    x = (0.25 * (rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T)))).astype(_C64)
    q = np.ascontiguousarray(doa.sim.to_sc16(x))
    angles = rng.uniform(0.0, 180.0, (N_MAX, M)).astype(_F32)
    for a in (x, q, angles):
        a.setflags(write=False)
    return x, q, angles


def _placed(a, offset=0):
    """A writable copy of `a` whose first byte lies `offset` bytes past a 16-byte boundary."""
    sb = a[0].nbytes
    buf = np.zeros((a.shape[0] + 16 // sb,) + a.shape[1:], a.dtype)
    lead = ((offset - buf.ctypes.data) % 16) // sb
    v = buf[lead:lead + a.shape[0]]
    v[...] = a
    assert v.ctypes.data % 16 == offset
    return v


def _streams(fmt, n_streams, length, offsets=None):
    """The first `length` samples (at least one) of the first n_streams streams, as host arrays at the given byte offsets."""
    x, q, _ = _samples()
    src = q if fmt == "sc16" else x
    return [_placed(src[k][:max(length, 1)], 0 if offsets is None else offsets[k]) for k in range(n_streams)]


def _upload(arrs, keep_offsets=False):
    """Device copies of host arrays, laid out as the host entries stage them: one allocation, stream k at k times
    doa_stream_stride_bytes; keep_offsets: the stride takes 16 bytes more and every stream keeps its host address modulo 16
    (channel_covariance).  Returns (the allocation, the device pointers)."""
    nbytes = arrs[0].nbytes
    stride = int(lib.doa_stream_stride_bytes(nbytes + (16 if keep_offsets else 0)))
    slab = torch.zeros(len(arrs) * stride + 4096, dtype=torch.uint8, device="cuda")
    off0 = (-slab.data_ptr()) % 4096
    ptrs = []
    for k, a in enumerate(arrs):
        o = off0 + k * stride + (a.ctypes.data % 16 if keep_offsets else 0)
        slab[o:o + nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        ptrs.append(slab.data_ptr() + o)
    return slab, ptrs


class _OutSlab:
    """n_streams device output streams of `count` `dtype` elements, `stride` bytes apart in one sentinel-filled allocation."""

    def __init__(self, n_streams, count, dtype, stride):
        self.count, self.dtype, self.stride = count, dtype, stride
        fill = np.full(1, SENTINEL, dtype).view(np.uint8)
        self.t = torch.from_numpy(np.tile(fill, (n_streams * stride + 4096) // fill.size)).cuda()
        self.off0 = (-self.t.data_ptr()) % 4096
        self.ptrs = [self.t.data_ptr() + self.off0 + k * stride for k in range(n_streams)]

    def read_into(self, outs):
        host = self.t.cpu().numpy()
        for k, o in enumerate(outs):
            b = host[self.off0 + k * self.stride:][:self.count * np.dtype(self.dtype).itemsize]
            o.reshape(-1)[:self.count] = b.view(self.dtype)


def _vp(a):
    return C.c_void_p(0 if a is None else a.ctypes.data)


def _sync_stream():
    return torch.cuda.current_stream()


class _Entry:
    """One host entry: make() a fresh block; outs(n) sentinel-filled host outputs; host(blk, n[, present]) -> (rc, outs);
    dev(blk, n) -> (rc, outs) through the device entry; rc(n): what a good call returns; rewind(blk): put a block with a
    position back to the start; raw(blk, n, in_ptrs, outs) -> rc: the C entry itself, for blocks with input ports."""
    optional = ()               # indices of optional output ports
    raw = None

    def rc(self, n):
        return n

    def rewind(self, blk):
        pass


class _Autocorrelate(_Entry):
    def __init__(self, fmt, ovl):
        self.fmt, self.ovl = fmt, ovl

    def make(self):
        blk = doa.autocorrelate(N, K, self.ovl, 1 if self.ovl else 0)
        if self.fmt == "sc16":
            blk.set_input_format("sc16")
        return blk

    def ins(self, n, offsets=None):
        return _streams(self.fmt, N, (n - 1) * (K - self.ovl) + K if n > 0 else 0, offsets)

    def outs(self, n):
        return [np.full((max(n, 1), N * N), SENTINEL, _C64)]

    def host(self, blk, n, present=None):
        outs = self.outs(n)
        return blk.general_work(n, self.ins(n), outs)[0], outs

    def dev(self, blk, n):
        outs = self.outs(n)
        slab, ptrs = _upload(self.ins(n))
        d = torch.from_numpy(outs[0]).cuda()
        rc = blk.work_dev(n, ptrs, d.data_ptr(), _sync_stream())
        torch.cuda.synchronize()
        return rc, [d.cpu().numpy()]

    def raw(self, blk, n, in_ptrs, outs):
        return lib.doa_autocorrelate_work(blk._h, n, ptr_array(in_ptrs), _vp(outs[0]))


class _ChannelCovariance(_Entry):
    optional = (1,)

    def __init__(self, fmt, ovl, power):
        self.fmt, self.ovl, self.power = fmt, ovl, power

    def make(self):
        blk = doa.channel_covariance(N, K, self.ovl, F, "hann")
        if self.fmt == "sc16":
            blk.set_input_format("sc16")
        return blk

    ins = _Autocorrelate.ins

    def outs(self, n):
        return [np.full((max(n, 1) * F, N * N), SENTINEL, _C64)] + ([np.full((max(n, 1), F), SENTINEL, _F32)] if self.power else [])

    def host(self, blk, n, present=None, offsets=None):
        outs = self.outs(n)
        if present is not None:
            outs = [o if p else None for o, p in zip(outs, present)]
        ins = self.ins(n, offsets)
        rc = blk.general_work(n, ins, outs)[0]
        return rc, outs

    def dev(self, blk, n, offsets=None):
        outs = self.outs(n)
        slab, ptrs = _upload(self.ins(n, offsets), keep_offsets=True)
        d = [torch.from_numpy(o).cuda() for o in outs]
        rc = blk.work_dev(n, ptrs, d[0].data_ptr(), d[1].data_ptr() if self.power else None, _sync_stream())
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy() for t in d]

    def raw(self, blk, n, in_ptrs, outs):
        return lib.doa_channel_covariance_work(blk._h, n, ptr_array(in_ptrs), _vp(outs[0]), _vp(outs[1] if self.power else None))


@functools.lru_cache(maxsize=None)
def _calibration_file():
    """An antenna_correction config file of N "gain phase" lines; the directory lives as long as the module."""
    d = tempfile.TemporaryDirectory()
    path = d.name + "/antenna.cfg"
    with open(path, "w") as f:
        for g, p in zip((1.0, 0.8, 1.3, 0.9), (0.0, 0.4, -1.1, 2.0)):
            f.write(f"{g} {p}\n")
    return d, path


def _even(n):
    return (n + 1) & ~1


class _AntennaCorrection(_Entry):
    def make(self):
        return doa.antenna_correction(N, _calibration_file()[1])

    def ins(self, n):
        return _streams("fc32", N, n)

    def outs(self, n):
        return [np.full(max(n, 1), SENTINEL, _C64) for _ in range(N)]

    def host(self, blk, n, present=None):
        outs = self.outs(n)
        return blk.work(n, self.ins(n), outs), outs

    def dev(self, blk, n):
        outs = self.outs(n)
        d_in = torch.zeros(N * _even(n), dtype=torch.complex64, device="cuda")
        for k, a in enumerate(self.ins(n)):
            d_in[k * _even(n):k * _even(n) + n].copy_(torch.from_numpy(a))
        d_out = _OutSlab(N, n, _C64, _even(n) * 8)
        rc = blk.work_dev(n, [d_in.data_ptr() + k * _even(n) * 8 for k in range(N)], d_out.ptrs, _sync_stream())
        torch.cuda.synchronize()
        d_out.read_into(outs)
        return rc, outs

    def raw(self, blk, n, in_ptrs, outs):
        return lib.doa_antenna_correction_work(blk._h, n, ptr_array(in_ptrs), ptr_array([o.ctypes.data for o in outs]))


class _PhaseOffset(_Entry):
    """twinrx_phase_offset_est with a skip of SKIP samples; ports = 4 in fc32, 2 in sc16."""

    def __init__(self, ports):
        self.ports, self.fmt = ports, "fc32" if ports == N else "sc16"

    def make(self):
        blk = doa.twinrx_phase_offset_est(self.ports, SKIP)
        if self.fmt == "sc16":
            blk.set_input_format("sc16")
        return blk

    def ins(self, n):
        return _streams(self.fmt, self.ports, n)

    def rewind(self, blk):
        blk.reset()


class _PhaseOffsetWork(_PhaseOffset):
    def rc(self, n):
        return max(n - SKIP, 0)

    def outs(self, n):
        return [np.full(max(n, 1), SENTINEL, _F32) for _ in range(self.ports - 1)]

    def host(self, blk, n, present=None):
        outs = self.outs(n)
        return blk.work(n, self.ins(n), outs), outs

    def dev(self, blk, n):
        outs = self.outs(n)
        slab, ptrs = _upload(self.ins(n))
        d_out = _OutSlab(self.ports - 1, self.rc(n), _F32, (self.rc(n) * 4 + 15) & ~15)
        rc = blk.work_dev(n, ptrs, d_out.ptrs, _sync_stream())
        torch.cuda.synchronize()
        d_out.read_into(outs)
        return rc, outs

    def raw(self, blk, n, in_ptrs, outs):
        return lib.doa_phase_offset_est_work(blk._h, n, ptr_array(in_ptrs), ptr_array([o.ctypes.data for o in outs]))


class _PhaseOffsetEstimate(_PhaseOffset):
    optional = (0, 1, 2)

    def rc(self, n):
        return 0

    def outs(self, n):
        return [np.full(self.ports - 1, SENTINEL, _F32) for _ in range(3)]

    def host(self, blk, n, present=None):
        got = blk.estimate(n, self.ins(n), n - SKIP, *((True,) * 3 if present is None else present))
        return 0, list(got)

    def dev(self, blk, n):
        outs = self.outs(n)
        slab, ptrs = _upload(self.ins(n))
        d = [torch.from_numpy(o).cuda() for o in outs]
        blk.estimate_dev(n, ptrs, n - SKIP, *[t.data_ptr() for t in d], _sync_stream())
        torch.cuda.synchronize()
        return 0, [t.cpu().numpy() for t in d]

    def raw(self, blk, n, in_ptrs, outs):
        return lib.doa_phase_offset_est_estimate(blk._h, n, ptr_array(in_ptrs), max(n - SKIP, 1), *[_vp(o) for o in outs])


class _SimSource(_Entry):
    def make(self):
        return doa.sim_source(N, 0.5, [60.0, 110.0], [0.01, 0.03], source_noise_ampl=[0.05, 0.1], antenna_noise_sigma=0.2,
                              seed=11)

    def rewind(self, blk):
        blk.seek(0)

    def outs(self, n):
        return [np.full(max(n, 1), SENTINEL, _C64) for _ in range(N)]

    def host(self, blk, n, present=None):
        outs = self.outs(n)
        rc = blk.work(n, outs)
        assert blk.tell() == n
        return rc, outs

    def dev(self, blk, n):
        outs = self.outs(n)
        d_out = _OutSlab(N, n, _C64, _even(n) * 8)
        rc = blk.work_dev(n, d_out.ptrs, _sync_stream())
        torch.cuda.synchronize()
        d_out.read_into(outs)
        return rc, outs


class _CompassMean(_Entry):
    def make(self):
        return doa.compass_mean(M)

    def outs(self, n):
        return [np.full(M, SENTINEL, _F32)]

    def host(self, blk, n, present=None):
        blk.next_angle[:] = SENTINEL
        rc = blk.work(n, [_samples()[2][:max(n, 1)]])
        return rc, [blk.next_angle.copy()]

    def dev(self, blk, n):
        d_in = torch.from_numpy(np.array(_samples()[2][:n])).cuda()
        d_out = torch.from_numpy(self.outs(n)[0]).cuda()
        rc = blk.work_dev(n, d_in.data_ptr(), d_out.data_ptr(), _sync_stream())
        torch.cuda.synchronize()
        return rc, [d_out.cpu().numpy()]


ENTRIES = {
    "autocorrelate.general_work[fc32]": _Autocorrelate("fc32", 0),
    "autocorrelate.general_work[sc16]": _Autocorrelate("sc16", 0),
    "autocorrelate.general_work[pieces]": _Autocorrelate("fc32", 16),
    "channel_covariance.general_work[power]": _ChannelCovariance("fc32", 16, True),
    "channel_covariance.general_work[no power]": _ChannelCovariance("sc16", 0, False),
    "antenna_correction.work": _AntennaCorrection(),
    "twinrx_phase_offset_est.work[4]": _PhaseOffsetWork(4),
    "twinrx_phase_offset_est.work[2]": _PhaseOffsetWork(2),
    "twinrx_phase_offset_est.estimate[4]": _PhaseOffsetEstimate(4),
    "twinrx_phase_offset_est.estimate[2]": _PhaseOffsetEstimate(2),
    "sim_source.work": _SimSource(),
    "compass_mean.work": _CompassMean(),
}
ALL = sorted(ENTRIES)
WITH_OPTIONAL_PORT = [(k, p) for k in ALL for p in ENTRIES[k].optional if len(ENTRIES[k].outs(1)) > p]
WITH_INPUT_PORTS = [k for k in ALL if ENTRIES[k].raw is not None]


def test_the_table_covers_the_six_blocks():
    assert len({k.split(".")[0] for k in ENTRIES}) == 6
    assert len(WITH_OPTIONAL_PORT) == 7 and len(WITH_INPUT_PORTS) == 10


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _untouched(outs):
    return all(np.array_equal(a, np.full_like(a, SENTINEL)) for a in outs)


@functools.lru_cache(maxsize=None)
def _fresh(key, n):
    """What a fresh handle's host entry gives for n items, every port present (computed once, read-only)."""
    e = ENTRIES[key]
    rc, outs = e.host(e.make(), n)
    assert rc == e.rc(n)
    for a in outs:
        assert not np.array_equal(a, np.full_like(a, SENTINEL)), (key, "an output port was not written")
        a.setflags(write=False)
    return outs


@pytest.mark.parametrize("key", ALL)
def test_host_entry_equals_device_entry(key):
    e = ENTRIES[key]
    rc, outs = e.dev(e.make(), N_MAX)
    assert rc == e.rc(N_MAX)
    for port, (a, b) in enumerate(zip(outs, _fresh(key, N_MAX))):
        assert _same(a, b), (key, port)


@pytest.mark.parametrize("key", ALL)
def test_buffers_grow_and_are_reused(key):
    e = ENTRIES[key]
    blk = e.make()
    for n in GROWTH:
        e.rewind(blk)
        rc, outs = e.host(blk, n)
        assert rc == e.rc(n)
        for port, (a, b) in enumerate(zip(outs, _fresh(key, n))):
            assert _same(a, b), (key, n, port)


@pytest.mark.parametrize("key", ALL)
def test_zero_items_return_zero_and_write_nothing(key):
    e = ENTRIES[key]
    blk = e.make()
    if isinstance(e, _PhaseOffsetEstimate):          # no zero-item call: at least one sample is required
        outs = e.outs(0)
        assert e.raw(blk, 0, [a.ctypes.data for a in e.ins(0)], outs) == DOA_ERR_INVALID_ARG
        assert "phase_offset_est_estimate" in last_error() and _untouched(outs)
        return
    rc, outs = e.host(blk, 0)
    assert rc == 0
    if isinstance(e, _CompassMean):                  # numpy.mean of nothing
        assert np.isnan(outs[0]).all()
    else:
        assert _untouched(outs), key


@pytest.mark.parametrize("key,port", WITH_OPTIONAL_PORT)
def test_optional_port_may_be_absent(key, port):
    e = ENTRIES[key]
    present = tuple(p != port for p in range(len(e.outs(1))))
    rc, outs = e.host(e.make(), N_MAX, present)
    assert rc == e.rc(N_MAX) and outs[port] is None
    for p, (a, b) in enumerate(zip(outs, _fresh(key, N_MAX))):
        assert p == port or _same(a, b), (key, port, p)


@pytest.mark.parametrize("key", WITH_INPUT_PORTS)
def test_null_last_input_port_is_refused_and_the_handle_stays_usable(key):
    e = ENTRIES[key]
    blk = e.make()
    ins, outs = e.ins(N_MAX), e.outs(N_MAX)
    ptrs = [a.ctypes.data for a in ins]
    last = len(ptrs) - 1
    ptrs[last] = 0
    assert e.raw(blk, N_MAX, ptrs, outs) == DOA_ERR_INVALID_ARG
    assert re.search(r"(input_items\[%d\]|port %d) is NULL" % (last, last), last_error()), last_error()
    assert _untouched(outs), key
    rc, outs = e.host(blk, N_MAX)                    # no rewind: the refused call must not have moved the handle
    assert rc == e.rc(N_MAX)
    for port, (a, b) in enumerate(zip(outs, _fresh(key, N_MAX))):
        assert _same(a, b), (key, port)


@pytest.mark.parametrize("fmt,offsets", [("fc32", (0, 8, 0, 8)), ("sc16", (4, 8, 12, 0))])
def test_channel_covariance_host_entry_follows_host_offsets_like_the_device_entry(fmt, offsets):
    e = _ChannelCovariance(fmt, 16, True)
    rc_h, host = e.host(e.make(), N_MAX, offsets=offsets)
    rc_d, dev = e.dev(e.make(), N_MAX, offsets=offsets)
    assert rc_h == rc_d == N_MAX
    for port, (a, b) in enumerate(zip(host, dev)):
        assert not np.array_equal(a, np.full_like(a, SENTINEL)) and _same(a, b), (fmt, offsets, port)
