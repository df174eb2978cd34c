"""GPU tests of the device-resident pipeline (doa.music_pipeline = autocorrelate -> MUSIC_lin_array
-> find_local_max on device pointers), the entry point bench.py drives."""
import numpy as np
import pytest

import doa
import doa_oracle as oracle
from scenarios import make_input

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["bench_cfg2", "grc_music_sim", "three_ant_fb", "qa_music_aoa23", "five_ant", "bench_cfg4",
                                  "twelve_ant", "xml_default_p20", "two_ant"])
def test_pipeline_equals_chained_blocks_and_oracle(name):
    c, x = make_input(name)
    N, M, P, n = c["N"], c["M"], c["P"], c["n"]
    streams = [_dev(x[k]) for k in range(N)]
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    pipe = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
    st = torch.cuda.current_stream()
    assert pipe.work_dev(n, [s.data_ptr() for s in streams], cov.data_ptr(), spec.data_ptr(), mx.data_ptr(),
                         am.data_ptr(), st) == n
    torch.cuda.synchronize()
    # the same through the three block objects on host buffers
    a = doa.autocorrelate(N, c["K"], c["ovl"], c["fb"])
    R = np.empty((n, N * N), np.complex64)
    a.general_work(n, [x[k] for k in range(N)], [R])
    m = doa.MUSIC_lin_array(c["d"], M, N, P)
    S = np.empty((n, P), np.float32)
    m.work(n, [R], [S])
    f = doa.find_local_max(M, P, 0.0, 180.0)
    v0 = np.empty((n, M), np.float32)
    v1 = np.empty((n, M), np.float32)
    f.work(n, [S], [v0, v1])
    assert np.array_equal(cov.cpu().numpy(), R)
    # the pipeline's lean kernel evaluates Q through a different (equally exact) double formula than the
    # block's general kernel: identical to float rounding, not necessarily bit for bit
    assert np.all(np.abs(spec.cpu().numpy() - S) <= 2e-6 + 5e-7 * np.abs(S))    # a few ulp of the dB value
    assert np.all(np.abs(mx.cpu().numpy() - v0) <= 2e-6 + 5e-7 * np.abs(v0)) and np.array_equal(am.cpu().numpy(), v1)
    # and against the oracle: covariance to rounding, angles on the grid
    R64 = oracle.autocorrelate(x, c["K"], c["ovl"], c["fb"], n, precision="f64")
    assert np.abs(R - R64).max() <= 2e-6 * np.abs(R64).max()
    _, _, _, loc = oracle.music_pipeline(x, c["K"], c["ovl"], c["fb"], c["d"], M, P, n)
    assert np.abs(v1 - loc).max() <= 180.0 / P + 1e-3


def test_pipeline_full_batch_recovers_directions():
    """BASELINE.json configs[1] at full size (N=4, K=1024, P=1024, batch 4096, SNR 20 dB): the
    estimated angle of every snapshot is within a grid step (+ the estimator's own spread) of the
    direction it was generated with, and a sample of rows equals the oracle."""
    N, K, P, M, B = 4, 1024, 1024, 1, 4096
    streams, thetas = doa.sim.make_batch_streams_torch(N, K, B, 0.5, M, 20.0, seed=123)
    mx = torch.empty((B, M), dtype=torch.float32, device="cuda")
    am = torch.empty((B, M), dtype=torch.float32, device="cuda")
    spec = torch.empty((B, P), dtype=torch.float32, device="cuda")
    pipe = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=B)
    assert pipe.work_dev(B, [s.data_ptr() for s in streams], 0, spec.data_ptr(), mx.data_ptr(), am.data_ptr(),
                         torch.cuda.current_stream()) == B
    torch.cuda.synchronize()
    est = am.cpu().numpy()[:, 0]
    assert np.abs(est - thetas[:, 0]).max() <= 1.0
    assert np.all(mx.cpu().numpy() == 0.0)                     # M == 1: the global maximum is 0 dB
    sample = slice(0, 64)
    x = np.stack([s[: 64 * K].cpu().numpy() for s in streams])
    _, s32, v0, loc = oracle.music_pipeline(x, K, 0, 0, 0.5, M, P, 64)
    assert np.abs(est[sample] - loc[:, 0]).max() <= 180.0 / P + 1e-3
    # the lean scan+peak kernel of the pipeline against the fp64 evaluation on the same covariances
    cov = torch.empty((64, N * N), dtype=torch.complex64, device="cuda")
    sp64 = torch.empty((64, P), dtype=torch.float32, device="cuda")
    pipe.work_dev(64, [s.data_ptr() for s in streams], cov.data_ptr(), sp64.data_ptr(), mx.data_ptr(), am.data_ptr(),
                  torch.cuda.current_stream())
    torch.cuda.synchronize()
    s64 = oracle.music_lin_array(cov.cpu().numpy(), 0.5, M, N, P, "f64")
    got = sp64.cpu().numpy()
    assert np.all(got.max(axis=1) == 0.0)
    assert np.all(np.abs(got - s64) <= 2e-5 + 2e-6 * np.abs(s64))
    assert np.array_equal(np.argmax(got, axis=1), np.argmax(s64, axis=1))


def test_pipeline_rejects_oversized_batch():
    pipe = doa.music_pipeline(4, 64, 0, 0, 0.5, 1, 64, max_batch=8)
    with pytest.raises(doa.DoaError):
        pipe.work_dev(9, [1, 1, 1, 1], 0, 0, 1, 1, None)


@pytest.mark.parametrize("name", ["bench_cfg2", "grc_music_sim", "three_ant_fb", "five_ant", "bench_cfg4", "twelve_ant"])
def test_pipeline_host_entry_equals_device_entry(name):
    # doa_music_pipeline_work (host buffers, what a GNU Radio hier block would call) against the
    # device-pointer entry point on the same samples: bit for bit, optional outputs optional
    c, x = make_input(name)
    N, M, P, n = c["N"], c["M"], c["P"], c["n"]
    pipe = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
    streams = [_dev(x[k]) for k in range(N)]
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    pipe.work_dev(n, [s.data_ptr() for s in streams], cov.data_ptr(), spec.data_ptr(), mx.data_ptr(), am.data_ptr(),
                  torch.cuda.current_stream())
    torch.cuda.synchronize()
    h_mx, h_am = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
    h_cov, h_spec = np.empty((n, N * N), np.complex64), np.empty((n, P), np.float32)
    assert pipe.work(n, [x[k] for k in range(N)], h_mx, h_am, cov_out=h_cov, spectrum_out=h_spec) == n
    assert np.array_equal(h_cov, cov.cpu().numpy()) and np.array_equal(h_spec, spec.cpu().numpy())
    assert np.array_equal(h_mx, mx.cpu().numpy()) and np.array_equal(h_am, am.cpu().numpy())
    a_mx, a_am = np.full((n, M), np.nan, np.float32), np.full((n, M), np.nan, np.float32)
    assert pipe.work(n - 1, [x[k] for k in range(N)], a_mx, a_am) == n - 1           # angles only, fewer items
    assert np.array_equal(a_mx[:n - 1], h_mx[:n - 1]) and np.array_equal(a_am[:n - 1], h_am[:n - 1])
    assert np.isnan(a_mx[n - 1]).all()
    with pytest.raises(ValueError):
        pipe.work(n, [x[k][:-1] for k in range(N)], h_mx, h_am)
    with pytest.raises(doa.DoaError):
        pipe.work(n + 1, [np.zeros(x.shape[1] + c["K"], np.complex64)] * N, np.empty((n + 1, M), np.float32),
                  np.empty((n + 1, M), np.float32))


@pytest.mark.parametrize("K,ovl,fb,M", [(1024, 0, 0, 1), (2048, 512, 1, 2)])
def test_pipeline_host_entry_multi_chunk(K, ovl, fb, M):
    # enough snapshots for several 32 MiB transfer chunks on both copy/compute lanes, with and without
    # overlapping windows (a chunk's first window re-reads the previous chunk's last `ovl` samples)
    N, P, d = 4, 1024, 0.5
    n = 2 * ((32 << 20) // ((K - ovl) * N * 8)) + 301
    T = (n - 1) * (K - ovl) + K
    x = doa.sim.make_streams(N, T, [40.0, 115.0][:M], d, snr_db=15.0, seed=5)
    pipe = doa.music_pipeline(N, K, ovl, fb, d, M, P, max_batch=n)
    h_mx, h_am = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
    h_spec = np.empty((n, P), np.float32)
    assert pipe.work(n, [x[k] for k in range(N)], h_mx, h_am, spectrum_out=h_spec) == n
    streams = [_dev(x[k]) for k in range(N)]
    spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    pipe.work_dev(n, [s.data_ptr() for s in streams], 0, spec.data_ptr(), mx.data_ptr(), am.data_ptr(),
                  torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(h_spec, spec.cpu().numpy())
    assert np.array_equal(h_mx, mx.cpu().numpy()) and np.array_equal(h_am, am.cpu().numpy())


def test_pipeline_as_one_flowgraph_block_equals_the_three_block_chain():
    """doa.music_pipeline wired as a block (grc/doa_music_pipeline.xml: N streams in, locations / values / spectrum
    out) against autocorrelate -> MUSIC_lin_array -> find_local_max in the same mini flowgraph runtime, with
    scheduler-sized calls: every port bit for bit (history pre-roll, forecast and consume_each included)."""
    c, x = make_input("grc_music_sim")
    N, M, P, K, ovl = c["N"], c["M"], c["P"], c["K"], c["ovl"]
    S = K - ovl
    x_new = x[:, : (x.shape[1] // S) * S]

    def run(chain):
        tb = doa.runtime.top_block(max_noutput_items=5)
        srcs = [doa.runtime.vector_source_c(x_new[k]) for k in range(N)]
        sinks = [doa.runtime.vector_sink_f(M), doa.runtime.vector_sink_f(M), doa.runtime.vector_sink_f(P)]
        if chain:
            a = doa.autocorrelate(N, K, ovl, c["fb"])
            m = doa.MUSIC_lin_array(c["d"], M, N, P)
            f = doa.find_local_max(M, P, 0.0, 180.0)
            for k in range(N):
                tb.connect((srcs[k], 0), (a, k))
            tb.connect((a, 0), (m, 0))
            tb.connect((m, 0), (f, 0))
            tb.connect((f, 1), (sinks[0], 0))
            tb.connect((f, 0), (sinks[1], 0))
            tb.connect((m, 0), (sinks[2], 0))
        else:
            p = doa.music_pipeline(N, K, ovl, c["fb"], c["d"], M, P)         # the GRC make string's seven arguments
            for k in range(N):
                tb.connect((srcs[k], 0), (p, k))
            for port in range(3):
                tb.connect((p, port), (sinks[port], 0))
        tb.run()
        return [s.data() for s in sinks]

    one, three = run(False), run(True)
    assert one[0].shape[0] == (x_new.shape[1] // S) * M
    for a, b in zip(one, three):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["bench_cfg2", "grc_music_sim", "three_ant_fb", "two_ant", "five_ant", "bench_cfg4"])
def test_angles_only_mode_equals_the_full_pipeline(name):
    """No spectrum pointer = nobody wants the spectrum: the lean scan kernel then neither converts the row to dB nor writes
    it (other shapes write into the handle's scratch).  Peaks and angles must not change by a bit, irregular rows included."""
    c, x = make_input(name)
    N, M, P, n = c["N"], c["M"], c["P"], c["n"]
    x = [np.array(x[k]) for k in range(N)]
    S = c["K"] - c["ovl"]
    if n > 3:                                           # two rows with a non-finite null spectrum
        x[0][1 * S + 5] = np.nan
        x[N - 1][(n - 1) * S + 2] = np.inf
    streams = [_dev(a) for a in x]
    ptrs = [s.data_ptr() for s in streams]
    st = torch.cuda.current_stream()
    out = {}
    for mode in ("full", "angles"):
        pipe = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
        spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
        mx = torch.full((n, M), 7.0, dtype=torch.float32, device="cuda")
        am = torch.full((n, M), 7.0, dtype=torch.float32, device="cuda")
        assert pipe.work_dev(n, ptrs, 0, spec.data_ptr() if mode == "full" else 0, mx.data_ptr(), am.data_ptr(), st) == n
        torch.cuda.synchronize()
        out[mode] = (mx.cpu().numpy(), am.cpu().numpy())
    assert np.array_equal(out["full"][0], out["angles"][0], equal_nan=True)
    assert np.array_equal(out["full"][1], out["angles"][1], equal_nan=True)
    # and through the host entry point (small-call and chunked paths)
    pipe = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
    h0, h1 = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
    try:
        pipe.work(n, x, h0, h1)
    except doa.DoaError:
        pass                                            # non-finite rows are reported after the results are in place
    assert np.array_equal(h0, out["full"][0], equal_nan=True) and np.array_equal(h1, out["full"][1], equal_nan=True)


def _host_entry_handle(handle, N, K, d, M, P, n):
    """One of the fused handles with its host entry in a common form: (handle, a function that makes its output arrays with
    every optional output, a function that runs work() on them, the index of the angles among them)."""
    if handle == "music":
        pipe = doa.music_pipeline(N, K, 0, 0, d, M, P, max_batch=n)
        outs = lambda: [np.full((n, M), -7.0, np.float32), np.full((n, M), -7.0, np.float32), np.zeros((n, N * N), np.complex64),
                        np.zeros((n, P), np.float32)]
        return pipe, outs, lambda h, x, o: h.work(n, x, o[0], o[1], cov_out=o[2], spectrum_out=o[3]), 1
    pipe = doa.root_pipeline(N, K, 0, 0, d, M, max_batch=n)
    if handle == "root_esprit":
        pipe.set_estimator("esprit")
    outs = lambda: [np.full((n, M), -7.0, np.float32), np.zeros((n, N * N), np.complex64)]
    return pipe, outs, lambda h, x, o: h.work(n, x, o[0], cov_out=o[1]), 0


_HOST_FAILURES = [(0, False), (1, False), (2, False), (0, True)]


# (the music handle's cases keep the ids they had before the root handle's joined them)
@pytest.mark.parametrize("fail_chunk,small,handle",
                         [c + ("music",) for c in _HOST_FAILURES] + [c + ("root",) for c in _HOST_FAILURES] + [(0, True, "root_esprit")],
                         ids=[f"{c}-{s}" for c, s in _HOST_FAILURES] + [f"root-{c}-{s}" for c, s in _HOST_FAILURES] + ["root_esprit-0-True"])
def test_host_entry_failure_leaves_no_copy_in_flight(fail_chunk, small, handle):
    """VERDICT r2 #7 / ADVICE r2: a failure inside doa_music_pipeline_work / doa_root_pipeline_work -- in any chunk of the
    two-lane chunk loop, or in the staged scheduler-sized path -- must not return while the other lane (or the staging
    upload) is still copying to or from the caller's host buffers.  inject_failure makes chunk `fail_chunk` fail after its
    uploads were enqueued; the call must report DOA_ERR_HIP, both lanes must be idle on return, and the next call on the
    same handle must succeed and match a call on a fresh handle bit for bit.  Both handles share the transport
    (csrc/pipeline_front.hpp); each runs the four cases, the root handle the staged one in ESPRIT mode as well."""
    N, K, P, d, M = 4, 1024, 1024, 0.5, 1
    n = 24 if small else 2 * ((32 << 20) // (K * N * 8)) + 77            # three chunks over two lanes, or one staged call
    x = doa.sim.make_streams(N, n * K, [64.0], d, snr_db=15.0, seed=11)
    pipe, outs, work, angles = _host_entry_handle(handle, N, K, d, M, P, n)
    out = outs()
    pipe.inject_failure(fail_chunk)
    with pytest.raises(doa.DoaError) as ei:
        work(pipe, [x[k] for k in range(N)], out)
    assert ei.value.status == -3 and "injected failure" in str(ei.value)
    assert pipe.lanes_idle()                                           # nothing pending: the caller may reuse its buffers
    # the buffers really are the caller's again: scribble over the inputs, then run a clean call on fresh copies
    x2 = x.copy()
    x[:] = 0
    out2 = outs()
    assert work(pipe, [x2[k] for k in range(N)], out2) == n             # one-shot: disarmed
    ref, _, _, _ = _host_entry_handle(handle, N, K, d, M, P, n)
    out3 = outs()
    assert work(ref, [x2[k] for k in range(N)], out3) == n
    for got, want in zip(out2, out3):
        assert np.array_equal(got, want)
    assert np.abs(out2[angles] - 64.0).max() <= 1.0


def test_host_entry_short_snapshot_long_spectrum_takes_the_chunked_path():
    """the staged one-copy path is gated on BOTH directions; a short-K, long-P call whose spectra exceed the
    gate must not grow the page-locked staging buffer to hundreds of MiB -- and either path gives the same bits."""
    N, K, P, d, M = 4, 16, 4096, 0.5, 1
    n = 1500                                                            # in: 96 KiB per stream, out: 24 MiB of spectra
    x = doa.sim.make_streams(N, n * K, [100.0], d, snr_db=25.0, seed=3)
    pipe = doa.music_pipeline(N, K, 0, 0, d, M, P, max_batch=n)
    mx, am, spec = np.empty((n, M), np.float32), np.empty((n, M), np.float32), np.empty((n, P), np.float32)
    assert pipe.work(n, [x[k] for k in range(N)], mx, am, spectrum_out=spec) == n
    # small calls of the same stream (staged path: 64 items -> 1 MiB of spectra) give the same rows
    m = 64
    mx_s, am_s, spec_s = np.empty((m, M), np.float32), np.empty((m, M), np.float32), np.empty((m, P), np.float32)
    assert pipe.work(m, [x[k][:m * K] for k in range(N)], mx_s, am_s, spectrum_out=spec_s) == m
    assert np.array_equal(spec_s, spec[:m]) and np.array_equal(am_s, am[:m]) and np.array_equal(mx_s, mx[:m])


@pytest.mark.parametrize("name,lanes", [("bench_cfg2", 4), ("grc_music_sim", 3), ("bench_cfg4", 2), ("five_ant", 4), ("bench_cfg2", 1)])
def test_batches_entry_equals_single_calls_bit_for_bit(name, lanes):
    """doa_music_pipeline_work_dev_batches -- K batches in one call, overlapped over the handle's own lanes,
    one fork and one join on the caller's stream -- gives exactly the bits of K work_dev calls (same kernels, same
    launch shapes), whatever mix of optional outputs the batches ask for."""
    c, x = make_input(name)
    N, M, P, n = c["N"], c["M"], c["P"], c["n"]
    nb = 7
    S = c["K"] - c["ovl"]
    span = (n - 1) * S + c["K"]
    rng = np.random.default_rng(3)
    # batch b = the scenario's streams with a different scale and noise added: distinct inputs per batch
    xs = [(x * np.float32(1.0 + 0.25 * b) + (0.02 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))).astype(np.complex64)).astype(np.complex64)
          for b in range(nb)]
    d_in = [[_dev(xb[k][:span]) for k in range(N)] for xb in xs]
    mk = lambda shape, dt: [torch.full(shape, -3.0 if dt != torch.complex64 else 0, dtype=dt, device="cuda") for _ in range(nb)]
    ref = dict(cov=mk((n, N * N), torch.complex64), spec=mk((n, P), torch.float32), mx=mk((n, M), torch.float32), am=mk((n, M), torch.float32))
    got = dict(cov=mk((n, N * N), torch.complex64), spec=mk((n, P), torch.float32), mx=mk((n, M), torch.float32), am=mk((n, M), torch.float32))
    one = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
    st = torch.cuda.current_stream()
    # optional outputs per batch: covariance wanted for even batches, spectrum for all but batch 2 and 5
    want_cov = [b % 2 == 0 for b in range(nb)]
    want_spec = [b not in (2, 5) for b in range(nb)]
    for b in range(nb):
        one.work_dev(n, [t.data_ptr() for t in d_in[b]], ref["cov"][b].data_ptr() if want_cov[b] else 0,
                     ref["spec"][b].data_ptr() if want_spec[b] else 0, ref["mx"][b].data_ptr(), ref["am"][b].data_ptr(), st)
    torch.cuda.synchronize()
    pipe = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
    pipe.set_lanes(lanes)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # the fork must order the lanes behind what the caller's stream holds: refresh batch 0's inputs ON that stream right
        # before the call, and read batch nb-1's result on it right after (the join)
        fresh = [t.clone() for t in d_in[0]]
        for t in d_in[0]:
            t.zero_()
        torch.cuda._sleep(2_000_000)
        for t, f in zip(d_in[0], fresh):
            t.copy_(f)
        produced = pipe.work_dev_batches(n, [[t.data_ptr() for t in d_in[b]] for b in range(nb)],
                                         [got["cov"][b].data_ptr() if want_cov[b] else 0 for b in range(nb)],
                                         [got["spec"][b].data_ptr() if want_spec[b] else 0 for b in range(nb)],
                                         [t.data_ptr() for t in got["mx"]], [t.data_ptr() for t in got["am"]], side)
        last = got["am"][nb - 1].clone()
    assert produced == nb * n
    side.synchronize()
    assert torch.equal(last, ref["am"][nb - 1])
    torch.cuda.synchronize()
    for b in range(nb):
        assert torch.equal(got["mx"][b], ref["mx"][b]) and torch.equal(got["am"][b], ref["am"][b]), b
        if want_cov[b]:
            assert torch.equal(torch.view_as_real(got["cov"][b]), torch.view_as_real(ref["cov"][b])), b
        if want_spec[b]:
            assert torch.equal(got["spec"][b], ref["spec"][b]), b
        else:
            assert bool((got["spec"][b] == -3.0).all())                 # angles-only batches leave the caller's buffer alone
    # whole arrays omitted: angles only, no covariance copies
    am2 = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
    mx2 = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
    assert pipe.work_dev_batches(n, [[t.data_ptr() for t in d_in[b]] for b in range(nb)], None, None, [t.data_ptr() for t in mx2],
                                 [t.data_ptr() for t in am2], st) == nb * n
    torch.cuda.synchronize()
    for b in range(nb):
        assert torch.equal(am2[b], ref["am"][b]) and torch.equal(mx2[b], ref["mx"][b]), b


def test_batches_entry_argument_checks():
    pipe = doa.music_pipeline(4, 64, 0, 0, 0.5, 1, 256, max_batch=8)
    z = torch.zeros(8 * 64, dtype=torch.complex64, device="cuda")
    o = torch.empty((8, 1), dtype=torch.float32, device="cuda")
    ins = [[z.data_ptr()] * 4]
    with pytest.raises(doa.DoaError):
        pipe.work_dev_batches(9, ins, None, None, [o.data_ptr()], [o.data_ptr()])          # > max_batch
    with pytest.raises(doa.DoaError):
        pipe.work_dev_batches(8, ins, None, None, [0], [o.data_ptr()])                     # missing peak output
    with pytest.raises(doa.DoaError):
        pipe.set_lanes(0)
    assert pipe.work_dev_batches(0, ins, None, None, [o.data_ptr()], [o.data_ptr()]) == 0


def test_batches_entry_detached_and_adopted_streams():
    """The detached form (no ordering on a caller stream, joined by doa_music_pipeline_synchronize) and lanes on
    caller-created streams give the same bits as single calls; lanes keep rotating from call to call."""
    c, x = make_input("bench_cfg2")
    N, M, P, n = c["N"], c["M"], c["P"], c["n"]
    nb = 6
    d_in = [[_dev(x[k] * np.float32(1.0 + 0.125 * b)) for k in range(N)] for b in range(nb)]
    one = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
    ref_am, ref_sp = [], []
    for b in range(nb):
        am = torch.empty((n, M), dtype=torch.float32, device="cuda"); mx = torch.empty_like(am)
        sp = torch.empty((n, P), dtype=torch.float32, device="cuda")
        one.work_dev(n, [t.data_ptr() for t in d_in[b]], 0, sp.data_ptr(), mx.data_ptr(), am.data_ptr(), torch.cuda.current_stream())
        ref_am.append(am); ref_sp.append(sp)
    torch.cuda.synchronize()
    for adopt in (False, True):
        pipe = doa.music_pipeline(N, c["K"], c["ovl"], c["fb"], c["d"], M, P, max_batch=n)
        if adopt:
            pipe.set_lane_streams([torch.cuda.Stream() for _ in range(3)])
        am = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
        mx = [torch.empty((n, M), dtype=torch.float32, device="cuda") for _ in range(nb)]
        sp = [torch.empty((n, P), dtype=torch.float32, device="cuda") for _ in range(nb)]
        for b0, b1 in ((0, 1), (1, 4), (4, 6)):                      # calls of 1, 3 and 2 batches: the rotation carries over
            assert pipe.work_dev_batches(n, [[t.data_ptr() for t in d_in[b]] for b in range(b0, b1)], None,
                                         [sp[b].data_ptr() for b in range(b0, b1)], [mx[b].data_ptr() for b in range(b0, b1)],
                                         [am[b].data_ptr() for b in range(b0, b1)], doa.DETACHED) == (b1 - b0) * n
        pipe.synchronize()
        for b in range(nb):
            assert torch.equal(am[b], ref_am[b]) and torch.equal(sp[b], ref_sp[b]), (adopt, b)


def test_large_batch_scan_equals_small_batches():
    """At large batches the lean scan kernel is launched with 16 instead of 12 waves per CU and every wave loops over ~34 items
    (hand-placed record prefetch, music_scan_impl.hpp); one call over 140 000 snapshots must give the bits of the same
    snapshots processed 4096 at a time, ragged tail and an irregular row included."""
    N, K, P, M, d = 4, 16, 1024, 1, 0.5
    n = 140000 + 777                                                  # > 32 runs of 16 per wave at 16 waves per CU, ragged
    s, _ = doa.sim.make_batch_streams_torch(N, K, n, d, M, 15.0, seed=91, device="cuda")
    s[1][K * 100017 + 3] = float("nan")                              # one irregular item inside a run
    st = torch.cuda.current_stream()
    big = doa.music_pipeline(N, K, 0, 0, d, M, P, n)
    spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    big.work_dev(n, [t.data_ptr() for t in s], 0, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    small = doa.music_pipeline(N, K, 0, 0, d, M, P, 4096)
    spec2 = torch.empty((4096, P), dtype=torch.float32, device="cuda")
    mx2 = torch.empty((4096, M), dtype=torch.float32, device="cuda")
    am2 = torch.empty((4096, M), dtype=torch.float32, device="cuda")
    for i0 in list(range(0, n, 4096 * 7))[:5] + [96 * 1024, n - 4096 + 17 - 17]:     # a sample of chunks incl. the irregular item's and the tail
        i0 = min(i0, n - 4096)
        small.work_dev(4096, [t[i0 * K:].data_ptr() for t in s], 0, spec2.data_ptr(), mx2.data_ptr(), am2.data_ptr(), st)
        torch.cuda.synchronize()
        a, b = spec[i0:i0 + 4096], spec2
        same = (a == b) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), i0
        assert torch.equal(torch.nan_to_num(am[i0:i0 + 4096], nan=-1.0), torch.nan_to_num(am2, nan=-1.0)), i0
        assert torch.equal(torch.nan_to_num(mx[i0:i0 + 4096], nan=-1.0), torch.nan_to_num(mx2, nan=-1.0)), i0
    # and the stand-alone block (spectrum only) takes the same path at this size
    blk = doa.MUSIC_lin_array(d, M, N, P)
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    doa.autocorrelate(N, K, 0, 0).work_dev(n, [t.data_ptr() for t in s], cov.data_ptr(), st)
    spec3 = torch.empty((n, P), dtype=torch.float32, device="cuda")
    blk.work_dev(n, cov.data_ptr(), spec3.data_ptr(), st)
    torch.cuda.synchronize()
    same = (spec == spec3) | (torch.isnan(spec) & torch.isnan(spec3))
    assert bool(same.all())


@pytest.mark.parametrize("N,P,M,angles_only", [(4, 1024, 2, False), (3, 512, 2, False), (2, 256, 1, False), (4, 512, 3, False),
                                                (4, 256, 1, True), (4, 1024, 1, True), (4, 1024, 2, True)])
def test_large_batch_cooperative_scan_variants(N, P, M, angles_only):
    """From 16384 items on, the lean scan kernels run with 16 waves per CU and every wave loops over many items (the launch
    shape the row-store studies of rounds 3-4 were made on; the row-pair and workgroup-cooperative forms tried in round 4 were
    tested with this very test before they were dropped).  Every variant -- all three lean spectrum lengths, num_max_vals > 1
    (an LDS row per wave), the angles-only form -- must give the bits of the same items processed 4096 at a time, with a ragged
    tail and irregular rows."""
    K, d = 16, 0.5
    n = 16 * 4096 + 4096 + 531
    s, _ = doa.sim.make_batch_streams_torch(N, K, n, d, M, 15.0, seed=92, device="cuda")
    s[0][K * 40001 + 5] = float("nan")
    s[N - 1][K * (n - 3) + 1] = float("inf")
    st = torch.cuda.current_stream()
    big = doa.music_pipeline(N, K, 0, 0, d, M, P, n)
    M_out = M
    spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    mx = torch.empty((n, M_out), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M_out), dtype=torch.float32, device="cuda")
    big.work_dev(n, [t.data_ptr() for t in s], 0, 0 if angles_only else spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    small = doa.music_pipeline(N, K, 0, 0, d, M_out, P, 4096)
    spec2 = torch.empty((4096, P), dtype=torch.float32, device="cuda")
    mx2 = torch.empty((4096, M_out), dtype=torch.float32, device="cuda")
    am2 = torch.empty((4096, M_out), dtype=torch.float32, device="cuda")
    for i0 in (0, 36000, n - 4096):
        small.work_dev(4096, [t[i0 * K:].data_ptr() for t in s], 0, spec2.data_ptr(), mx2.data_ptr(), am2.data_ptr(), st)
        torch.cuda.synchronize()
        if not angles_only:
            a, b = spec[i0:i0 + 4096], spec2
            assert bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()), i0
        assert torch.equal(torch.nan_to_num(am[i0:i0 + 4096], nan=-1.0), torch.nan_to_num(am2, nan=-1.0)), i0
        assert torch.equal(torch.nan_to_num(mx[i0:i0 + 4096], nan=-1.0), torch.nan_to_num(mx2, nan=-1.0)), i0


@pytest.mark.parametrize("detached", [True, False])
def test_batches_entry_failure_leaves_nothing_running(detached):
    """An error return of doa_music_pipeline_work_dev_batches means nothing of the call is still running -- in the detached
    form too, where the caller would otherwise have to know that a call that FAILED must still be synchronised.  The batches
    launched before the failing one complete and are correct; the next call on the handle works."""
    N, K, P, d, M, n, nb = 4, 1024, 1024, 0.5, 1, 2048, 6
    s, th = doa.sim.make_batch_streams_torch(N, K, n * nb, d, M, 20.0, seed=21, device="cuda")
    ins = [[t[b * n * K:].data_ptr() for t in s] for b in range(nb)]
    mk = lambda shape: [torch.full(shape, -5.0, dtype=torch.float32, device="cuda") for _ in range(nb)]
    spec, mx, am = mk((n, P)), mk((n, M)), mk((n, M))
    pipe = doa.music_pipeline(N, K, 0, 0, d, M, P, max_batch=n)
    st = doa.DETACHED if detached else torch.cuda.current_stream()
    args = (n, ins, None, [t.data_ptr() for t in spec], [t.data_ptr() for t in mx], [t.data_ptr() for t in am], st)
    pipe.inject_failure(4)
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_batches(*args)
    assert ei.value.status == -3 and "injected failure in batch 4" in str(ei.value)
    assert pipe.lanes_idle()                                           # no synchronize call needed after a failed call
    torch.cuda.synchronize()
    for b in range(4):                                                 # what was launched before the failure is complete
        assert float(am[b].min()) > 0.0 and float((am[b][:, 0].cpu() - torch.from_numpy(th[b * n:(b + 1) * n, 0]).float()).abs().max()) <= 1.0
    assert float(am[4].max()) == -5.0 and float(am[5].max()) == -5.0   # the failing batch and the one behind it never ran
    assert pipe.work_dev_batches(*args) == n * nb                      # one-shot: disarmed
    pipe.synchronize()
    torch.cuda.synchronize()
    for b in range(nb):
        assert float((am[b][:, 0].cpu() - torch.from_numpy(th[b * n:(b + 1) * n, 0]).float()).abs().max()) <= 1.0
