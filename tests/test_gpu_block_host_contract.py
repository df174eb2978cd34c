"""GPU tests of what the host entries of the ten item blocks promise (gr-doa_amd/csrc/block_host.hpp), entry by entry:
  (a) the host `work` / `work_counts` gives bit for bit what `work_dev` / `work_dev_counts` gives on device buffers,
  (b) one handle called with 3, 70 and 3 items gives what a fresh handle gives (at 70 items every host buffer grows past its
      4096-byte floor; the second 3-item call then runs on buffers larger than it needs),
  (c) 0 items returns 0 and writes nothing,
  (d) a call without the optional port gives port 0 of a call with it,
  (e) the 64-bit-only entries refuse a handle created at internal precision 32 with DOA_ERR_UNSUPPORTED, on the host, and a
      handle created afterwards works.
Shapes are the smallest the blocks take: 4 antennas, 64-bin spectra, subarray 3.  The inputs are sample covariances of two
tones 20 dB above the noise (64 snapshots, one fixed seed), so no status flag fires.  Nothing here provokes a device fault:
every failing call is refused before any launch."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import doa

pytestmark = pytest.mark.gpu

N, P, K, S, D = 4, 64, 64, 3, 0.5
N_MAX = 70
GROWTH = (3, N_MAX, 3)
DOA_ERR_UNSUPPORTED = -4
_C64, _F32, _I32 = np.complex64, np.float32, np.int32


@functools.lru_cache(maxsize=None)
def _inputs():
    """(covariance items [70, 16] complex64, spectra [70, 64] float32, counts [70] int32), read-only."""
    rng = np.random.default_rng(20241019)
    A = np.exp(-2j * np.pi * D * np.outer(np.arange(N), np.cos(np.deg2rad([60.0, 110.0]))))

    def cnormal(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    R = np.empty((N_MAX, N * N), _C64)
    for i in range(N_MAX):
        x = A @ cnormal(2, K) + 0.1 * cnormal(N, K)
        R[i] = (x @ x.conj().T / K).T.reshape(-1)               # column-major items
    spectra = rng.standard_normal((N_MAX, P)).astype(_F32)
    counts = (1 + np.arange(N_MAX) % 2).astype(_I32)             # 1, 2, 1, 2, ...: usable by every counts entry here
    for a in (R, spectra, counts):
        a.setflags(write=False)
    return R, spectra, counts


@functools.lru_cache(maxsize=None)
def _table():
    xy = np.stack([D * np.arange(N), np.zeros(N)], axis=1)
    return doa.planar_steering_table(xy, P, 0.0, 180.0)


# make: a fresh block; spectra: the input is spectra, not covariances; counted: the *_counts entries; outs: (dtype, width) of
# every output port, the first n_req of them required by the host entry; dev_pad: optional ports only the device entry has;
# status: index of a status port that must stay 0; only64: refuses internal precision 32
Entry = namedtuple("Entry", "make spectra counted outs n_req dev_pad status only64")
_SPEC, _ST = (_F32, P), (_I32, 1)
ENTRIES = {
    "MUSIC_lin_array.work": Entry(lambda: doa.MUSIC_lin_array(D, 1, N, P), False, False, [_SPEC], 1, 0, None, False),
    "MUSIC_lin_array.work_counts": Entry(lambda: doa.MUSIC_lin_array(D, 1, N, P), False, True, [_SPEC], 1, 0, None, True),
    "capon_lin_array.work": Entry(lambda: doa.capon_lin_array(D, N, P, 0.0), False, False, [_SPEC, _ST], 1, 0, 1, True),
    "MUSIC_array.work": Entry(lambda: doa.MUSIC_array(1, _table()), False, False, [_SPEC], 1, 0, None, True),
    "capon_array.work": Entry(lambda: doa.capon_array(_table(), 0.0), False, False, [_SPEC, _ST], 1, 0, 1, True),
    "rootMUSIC_linear_array.work": Entry(lambda: doa.rootMUSIC_linear_array(D, 2, N), False, False, [(_F32, 2)], 1, 0, None, False),
    "rootMUSIC_linear_array.work_counts": Entry(lambda: doa.rootMUSIC_linear_array(D, 2, N), False, True, [(_F32, 2)], 1, 1, None, True),
    "esprit_linear_array.work": Entry(lambda: doa.esprit_linear_array(D, 2, N), False, False, [(_F32, 2), _ST], 1, 0, 1, True),
    "esprit_linear_array.work_counts": Entry(lambda: doa.esprit_linear_array(D, 2, N), False, True, [(_F32, 2), _ST], 1, 0, 1, True),
    "source_count.work": Entry(lambda: doa.source_count(N, K, "mdl"), False, False, [_ST, (_F32, N)], 1, 0, None, True),
    "spatial_smooth.work": Entry(lambda: doa.spatial_smooth(N, S, True), False, False, [(_C64, S * S)], 1, 0, None, False),
    "calibrate_lin_array.work": Entry(lambda: doa.calibrate_lin_array(D, N, 45.0), False, False, [(_C64, N)], 1, 0, None, False),
    "find_local_max.work": Entry(lambda: doa.find_local_max(2, P, 0.0, 180.0), True, False, [(_F32, 2), (_F32, 2)], 2, 0, None, False),
    "find_local_max.work_counts": Entry(lambda: doa.find_local_max(2, P, 0.0, 180.0), True, True, [(_F32, 2), (_F32, 2)], 2, 0, None, False),
}
ALL = sorted(ENTRIES)
WITH_OPTIONAL_PORT = [k for k in ALL if ENTRIES[k].n_req < len(ENTRIES[k].outs)]
ONLY64 = [k for k in ALL if ENTRIES[k].only64]
SENTINEL = -7


def test_the_table_covers_the_ten_blocks():
    assert len({k.split(".")[0] for k in ENTRIES}) == 10
    assert len(WITH_OPTIONAL_PORT) == 5 and len(ONLY64) == 8


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _sentinels(e, n, ports):
    return [np.full((max(n, 1), w), SENTINEL, dt) for dt, w in e.outs[:ports]]


def _host(key, blk, n, ports=None):
    """The host entry on n items -> (return value, output arrays), `ports` output ports passed (default: all)."""
    e = ENTRIES[key]
    R, spectra, counts = _inputs()
    outs = _sentinels(e, n, len(e.outs) if ports is None else ports)
    args = [[(spectra if e.spectra else R)[:max(n, 1)]]] + ([counts[:max(n, 1)]] if e.counted else []) + [outs]
    return getattr(blk, key.split(".")[1])(n, *args), outs


def _dev(key, blk, n):
    """The device entry on torch buffers, every optional port present, copied back."""
    e = ENTRIES[key]
    R, spectra, counts = _inputs()
    ins = [torch.from_numpy(np.array((spectra if e.spectra else R)[:n])).cuda()]
    if e.counted:
        ins.append(torch.from_numpy(np.array(counts[:n])).cuda())
    outs = [torch.from_numpy(a).cuda() for a in _sentinels(e, n, len(e.outs))]
    method = getattr(blk, key.split(".")[1].replace("work", "work_dev"))
    rc = method(n, *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], *([None] * e.dev_pad), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in outs]


@functools.lru_cache(maxsize=None)
def _fresh(key, n):
    """What a fresh handle's host entry gives for n items, every port present (computed once, read-only)."""
    rc, outs = _host(key, ENTRIES[key].make(), n)
    assert rc == n
    e = ENTRIES[key]
    if e.status is not None:
        assert not outs[e.status].any(), (key, "a status flag fired on the two-tone inputs", outs[e.status].ravel())
    for a in outs:
        assert not np.array_equal(a, np.full_like(a, SENTINEL)), (key, "an output port was not written")
        a.setflags(write=False)
    return outs


@pytest.mark.parametrize("key", ALL)
def test_host_entry_equals_device_entry(key):
    rc, outs = _dev(key, ENTRIES[key].make(), N_MAX)
    assert rc == N_MAX
    for port, (a, b) in enumerate(zip(outs, _fresh(key, N_MAX))):
        assert _same(a, b), (key, port)


@pytest.mark.parametrize("key", ALL)
def test_buffers_grow_and_are_reused(key):
    blk = ENTRIES[key].make()
    for n in GROWTH:
        rc, outs = _host(key, blk, n)
        assert rc == n
        for port, (a, b) in enumerate(zip(outs, _fresh(key, n))):
            assert _same(a, b), (key, n, port)


@pytest.mark.parametrize("key", ALL)
def test_zero_items_return_zero_and_write_nothing(key):
    rc, outs = _host(key, ENTRIES[key].make(), 0)
    assert rc == 0
    for a in outs:
        assert np.array_equal(a, np.full_like(a, SENTINEL)), key


@pytest.mark.parametrize("key", WITH_OPTIONAL_PORT)
def test_optional_port_may_be_absent(key):
    e = ENTRIES[key]
    rc, outs = _host(key, e.make(), N_MAX, ports=e.n_req)
    assert rc == N_MAX and len(outs) == e.n_req
    for port, (a, b) in enumerate(zip(outs, _fresh(key, N_MAX))):
        assert _same(a, b), (key, port)


@pytest.mark.parametrize("key", ONLY64)
def test_precision_32_is_refused_on_the_host(key):
    e = ENTRIES[key]
    assert doa.get_internal_precision() == 64
    doa.set_internal_precision(32)
    try:
        blk32 = e.make()
    finally:
        doa.set_internal_precision(64)
    with pytest.raises(doa.DoaError) as ei:
        _host(key, blk32, 3)
    assert ei.value.status == DOA_ERR_UNSUPPORTED and "precision 64" in str(ei.value)
    rc, outs = _host(key, e.make(), 3)
    assert rc == 3
    for port, (a, b) in enumerate(zip(outs, _fresh(key, 3))):
        assert _same(a, b), (key, port)
