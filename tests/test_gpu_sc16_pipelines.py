"""sc16 (complex int16) streams through music_pipeline and root_pipeline: on int16 streams q every output -- covariance,
spectrum, peaks, angles, status -- is BIT-IDENTICAL to the fc32 handle's on doa.sim.from_sc16(q, scale), through every entry:
work_dev, work_dev_batches (1 and 4 lanes, attached and detached) and the host entry on its staged (one copy) and chunked
(~32 MiB) paths; shapes: the benchmark's, the flowgraph's, N = 16 / P = 4096, angles-only mode, and full-scale data at
scale 1.0 (R ~ 1e9: the eigen stage's prescaling)."""
import numpy as np
import pytest
import torch

import doa
from doa.sim import from_sc16, to_sc16

pytestmark = pytest.mark.gpu

S15 = 2.0 ** -15
# name: (N, K, ovl, fb, d, M, P)
SHAPES = {
    "bench": (4, 1024, 0, 0, 0.5, 1, 1024),
    "flowgraph": (4, 2048, 512, 1, 0.4, 2, 1024),
    "n16": (16, 1024, 0, 0, 0.5, 3, 4096),
}


def _streams(N, K, ovl, n, seed, scale=S15, level=0.25):
    """int16 [N, span, 2]: back-to-back snapshots with their own random directions (the benchmark's workload)."""
    span = (n - 1) * (K - ovl) + K
    nb = -(-span // K)
    x, _ = doa.sim.make_batch_streams(N, K, nb, 0.5, num_targets=2, snr_db=15.0, seed=seed)
    x = x[:, :span]
    x = x / max(np.abs(x.real).max(), np.abs(x.imag).max()) * (level * 32767 * scale)
    return to_sc16(x, scale)


def _dev(arrays):
    return doa.sim.stream_slab_torch([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays])


def _music_dev(p, n, ptrs, spectrum=True):
    N, P, M = p.inputs, p.pspectrum_len, p.num_targets
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((n, P), dtype=torch.float32, device="cuda") if spectrum else None
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    p.work_dev(n, ptrs, cov.data_ptr(), spec.data_ptr() if spectrum else 0, mx.data_ptr(), am.data_ptr(),
               torch.cuda.current_stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (cov, spec, mx, am) if t is not None]


def _root_dev(p, n, ptrs):
    N, M = p.inputs, p.num_targets
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    ang = torch.empty((n, M), dtype=torch.float32, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    p.work_dev(n, ptrs, cov.data_ptr(), ang.data_ptr(), st.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (cov, ang, st)]


def _equal(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8))


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("spectrum", [True, False])
def test_music_work_dev(shape, spectrum):
    N, K, ovl, fb, d, M, P = SHAPES[shape]
    n = 4096 if shape == "bench" else 256
    q = _streams(N, K, ovl, n, seed=1)
    p16 = doa.music_pipeline_sc16(N, K, ovl, fb, d, M, P, max_batch=n)
    p32 = doa.music_pipeline(N, K, ovl, fb, d, M, P, max_batch=n)
    a = _music_dev(p16, n, [t.data_ptr() for t in _dev(q)], spectrum)
    b = _music_dev(p32, n, [t.data_ptr() for t in _dev(from_sc16(q))], spectrum)
    _equal(a, b)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_root_work_dev(shape):
    N, K, ovl, fb, d, M, _ = SHAPES[shape]
    n = 4096 if shape == "bench" else 256
    q = _streams(N, K, ovl, n, seed=2)
    p16 = doa.root_music_pipeline_sc16(N, K, ovl, fb, d, M, max_batch=n)
    p32 = doa.root_pipeline(N, K, ovl, fb, d, M, max_batch=n)
    _equal(_root_dev(p16, n, [t.data_ptr() for t in _dev(q)]), _root_dev(p32, n, [t.data_ptr() for t in _dev(from_sc16(q))]))


def _batches_music(p, n, nb, dev_batches, stream):
    N, P, M = p.inputs, p.pspectrum_len, p.num_targets
    cov = [torch.empty((n, N * N), dtype=torch.complex64, device="cuda") for _ in range(nb)]
    spec = [torch.empty((n, P), dtype=torch.float32, device="cuda") for _ in range(nb)]
    mx = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
    am = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    p.work_dev_batches(n, [ptr(b) for b in dev_batches], ptr(cov), ptr(spec), ptr(mx), ptr(am), stream)
    if stream == doa.DETACHED:
        p.synchronize()
    torch.cuda.synchronize()
    return [np.stack([t.cpu().numpy() for t in ts]) for ts in (cov, spec, mx, am)]


def _batches_root(p, n, nb, dev_batches, stream):
    N, M = p.inputs, p.num_targets
    cov = [torch.empty((n, N * N), dtype=torch.complex64, device="cuda") for _ in range(nb)]
    ang = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
    st = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(nb)]
    ptr = lambda ts: [t.data_ptr() for t in ts]
    p.work_dev_batches(n, [ptr(b) for b in dev_batches], ptr(cov), ptr(ang), ptr(st), stream)
    if stream == doa.DETACHED:
        p.synchronize()
    torch.cuda.synchronize()
    return [np.stack([t.cpu().numpy() for t in ts]) for ts in (cov, ang, st)]


@pytest.mark.parametrize("shape", ["bench", "flowgraph"])
@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("detached", [False, True])
def test_work_dev_batches(shape, lanes, detached):
    N, K, ovl, fb, d, M, P = SHAPES[shape]
    n, nb = 256, 6
    qs = [_streams(N, K, ovl, n, seed=10 + b) for b in range(nb)]
    d16 = [_dev(q) for q in qs]
    d32 = [_dev(from_sc16(q)) for q in qs]
    stream = doa.DETACHED if detached else torch.cuda.current_stream()
    for cls16, cls32, run, args in [
            (doa.music_pipeline_sc16, doa.music_pipeline, _batches_music, (N, K, ovl, fb, d, M, P)),
            (doa.root_music_pipeline_sc16, doa.root_pipeline, _batches_root, (N, K, ovl, fb, d, M))]:
        p16, p32 = cls16(*args, max_batch=n), cls32(*args, max_batch=n)
        p16.set_lanes(lanes)
        p32.set_lanes(lanes)
        _equal(run(p16, n, nb, d16, stream), run(p32, n, nb, d32, stream))


@pytest.mark.parametrize("shape,n", [("bench", 64), ("flowgraph", 48), ("bench", 4096), ("flowgraph", 2000), ("n16", 600)])
def test_host_entries_staged_and_chunked(shape, n):
    """n = 64 / 48: the staged one-copy path (< 2 MiB of sc16 input); 4096 / 2000 / 600: the chunked path, sc16 chunks
    sized by bytes (twice the fc32 chunk in snapshots)."""
    N, K, ovl, fb, d, M, P = SHAPES[shape]
    q = _streams(N, K, ovl, n, seed=3)
    x = from_sc16(q)
    p16 = doa.music_pipeline_sc16(N, K, ovl, fb, d, M, P, max_batch=n)
    p32 = doa.music_pipeline(N, K, ovl, fb, d, M, P, max_batch=n)
    outs = []
    for p, s in ((p16, [q[k] for k in range(N)]), (p32, [x[k] for k in range(N)])):
        mx, am = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
        cov, spec = np.empty((n, N * N), np.complex64), np.empty((n, P), np.float32)
        assert p.work(n, s, mx, am, cov_out=cov, spectrum_out=spec) == n
        mx2, am2 = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
        p.work(n, s, mx2, am2)                                       # angles only
        outs.append([cov, spec, mx, am, mx2, am2])
    _equal(*outs)
    r16 = doa.root_music_pipeline_sc16(N, K, ovl, fb, d, M, max_batch=n)
    r32 = doa.root_pipeline(N, K, ovl, fb, d, M, max_batch=n)
    outs = []
    for p, s in ((r16, [q[k] for k in range(N)]), (r32, [x[k] for k in range(N)])):
        ang, cov = np.empty((n, M), np.float32), np.empty((n, N * N), np.complex64)
        try:
            rc = p.work(n, s, ang, cov_out=cov)
        except doa.DoaError as e:                                  # an item without an interior root: same in both
            rc = e.status
        outs.append([np.array([rc]), ang, cov])
    _equal(*outs)


def test_general_work_takes_sc16_items():
    N, K, ovl, fb, d, M, P = SHAPES["flowgraph"]
    n = 40
    q = _streams(N, K, ovl, n, seed=4)
    p16 = doa.music_pipeline_sc16(N, K, ovl, fb, d, M, P, max_batch=16)       # several max_batch rounds
    assert p16.in_sig == [(np.int16, 2)] * N
    p32 = doa.music_pipeline(N, K, ovl, fb, d, M, P, max_batch=16)
    o16 = [np.empty((n, M), np.float32), np.empty((n, M), np.float32), np.empty((n, P), np.float32)]
    o32 = [np.empty((n, M), np.float32), np.empty((n, M), np.float32), np.empty((n, P), np.float32)]
    assert p16.general_work(n, [q[k].reshape(-1) for k in range(N)], o16) == (n, n * (K - ovl))
    p32.general_work(n, [from_sc16(q[k]) for k in range(N)], o32)
    _equal(o16, o32)


@pytest.mark.parametrize("N,M,P", [(4, 1, 1024), (8, 2, 1024), (16, 3, 4096)])
def test_full_scale_at_scale_one(N, M, P):
    """scale 1.0 on full-scale int16 data: covariance entries ~1e9; the eigen stage's prescaling must keep the fc32 and sc16
    paths on the same bits (they see the same floats)."""
    K, n = 1024, 128
    q = _streams(N, K, 0, n, seed=N, scale=1.0, level=1.0)
    assert np.abs(q.astype(np.int32)).max() == 32767
    p16 = doa.music_pipeline_sc16(N, K, 0, 1, 0.5, M, P, scale=1.0, max_batch=n)
    p32 = doa.music_pipeline(N, K, 0, 1, 0.5, M, P, max_batch=n)
    a = _music_dev(p16, n, [t.data_ptr() for t in _dev(q)])
    b = _music_dev(p32, n, [t.data_ptr() for t in _dev(from_sc16(q, 1.0))])
    assert np.abs(a[0]).max() > 1e8
    _equal(a, b)
    r16 = doa.root_music_pipeline_sc16(N, K, 0, 1, 0.5, M, scale=1.0, max_batch=n)
    r32 = doa.root_pipeline(N, K, 0, 1, 0.5, M, max_batch=n)
    _equal(_root_dev(r16, n, [t.data_ptr() for t in _dev(q)]), _root_dev(r32, n, [t.data_ptr() for t in _dev(from_sc16(q, 1.0))]))


def test_fused_correction_composes_with_sc16():
    N, K, ovl, fb, d, M, P = SHAPES["flowgraph"]
    n = 128
    q = _streams(N, K, ovl, n, seed=6)
    rng = np.random.default_rng(0)
    g = (rng.uniform(0.7, 1.3, N) * np.exp(1j * rng.uniform(-1, 1, N))).astype(np.complex64)
    res = []
    for cls, streams in ((doa.music_pipeline_sc16, q), (doa.music_pipeline, from_sc16(q))):
        p = cls(N, K, ovl, fb, d, M, P, max_batch=n)
        p.fuse_antenna_correction(g)
        res.append(_music_dev(p, n, [t.data_ptr() for t in _dev(streams)]))
    _equal(*res)
    res = []
    for cls, streams in ((doa.root_music_pipeline_sc16, q), (doa.root_pipeline, from_sc16(q))):
        p = cls(N, K, ovl, fb, d, M, max_batch=n)
        p.fuse_antenna_correction(g)
        res.append(_root_dev(p, n, [t.data_ptr() for t in _dev(streams)]))
    _equal(*res)
