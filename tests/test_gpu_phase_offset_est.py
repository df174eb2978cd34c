"""GPU tests of doa.twinrx_phase_offset_est against the numpy restatement of the reference's blocks (calibration_ref.py).

Streaming form: out_{p-1}[i] = atan2f(x_0[i]) - atan2f(x_p[i]), unwrapped.  Accuracy condition (stated with its derivation in
the feature's issue): |out - (angle64(x_0) - angle64(x_p))| <= 4 * 2^-21 rad -- each atan2f within 1.5 ulp of a value below 4
(ulp 2^-22), one subtraction rounded at a magnitude below 8 (half an ulp of 2^-21): 2 * 2^-21 in all, doubled for margin.
Fused form: maximum bit-identical to the maximum of the streaming output, mean within 1 float32 ulp of the float64 mean of the
streaming output, circular mean within 1e-6 rad of its float64 evaluation where |sum| >= 1e-3 sum |x_0||x_p|.
sc16: every output of both forms bit-identical to the fc32 path on float32(q) * float32(scale).

Non-finite samples: a NaN or an infinite component gives NaN for that sample's outputs and touches no other sample."""
import numpy as np
import pytest

import doa
import calibration_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 4 * 2.0 ** -21


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _streams(N, T, seed, special=True):
    """random samples of mixed magnitude; the first samples of every stream are the awkward ones"""
    rng = np.random.default_rng(seed)
    x = ((rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T))) * 10.0 ** rng.uniform(-3, 3, (N, T))).astype(np.complex64)
    if special:
        tiny = np.float32(1e-42)                                                  # a float32 denormal
        sp = np.array([1 + 0j, 0 + 1j, -1 + 0j, 0 - 1j, 0 + 0j, complex(tiny, tiny), complex(-tiny, 3 * tiny), complex(tiny, 0),
                       1e-20 + 1e-20j, -1e-20 + 2e-20j, 1e18 - 1e18j, -3e18 + 1e18j, complex(0.0, -0.0), complex(-1.0, -0.0),
                       1e-20 + 1e18j, 1e18 + 1e-20j], dtype=np.complex64)
        n = min(T, sp.size)
        for k in range(N):
            x[k, :n] = np.roll(sp, 3 * k)[:n]                                     # every pairing of stream 0 with the others differs
    return x


def _run_work(est, x, cuts):
    """feeds x [N, T] to est.work in calls cut at `cuts`; returns the concatenated outputs [N-1, produced]"""
    N, T = x.shape
    outs, edges = [], [0] + list(cuts) + [T]
    for a, b in zip(edges[:-1], edges[1:]):
        o = [np.full(b - a, 7.0, np.float32) for _ in range(N - 1)]
        got = est.work(b - a, [x[k, a:b] for k in range(N)], o)
        outs.append(np.stack([v[:got] for v in o]))
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("N,T,skip,cuts", [
    (2, 1001, 0, [333]),
    (4, 4099, 0, [1, 130, 131, 2049]),
    (4, 5003, 700, [1001, 3000]),              # skip smaller than the first call
    (8, 3001, 1500, [999, 1000, 2203]),        # skip larger than the first call (which produces nothing) and the second
    (16, 777, 77, [5, 400]),
])
def test_streaming_form_matches_numpy_and_does_not_depend_on_the_call_boundaries(N, T, skip, cuts):
    x = _streams(N, T, seed=N * 1000 + T)
    one = _run_work(doa.twinrx_phase_offset_est(N, skip), x, [])
    assert one.shape == (N - 1, T - skip)
    want64 = ref.phase_differences64(x, skip)
    err = np.abs(one.astype(np.float64) - want64)
    print(f"N={N} T={T} skip={skip}: max |out - float64| = {err.max():.3e} rad (bound {BOUND:.3e})")
    assert err.max() <= BOUND
    assert np.abs(one).max() < 2 * np.pi
    split = _run_work(doa.twinrx_phase_offset_est(N, skip), x, cuts)
    assert np.array_equal(_bits(split), _bits(one))
    # the restatement (correctly rounded float arctangents, one float subtraction) is within the same bound of it
    assert np.abs(one.astype(np.float64) - ref.twinrx_phase_offset_est(x, skip).astype(np.float64)).max() <= BOUND


def test_skip_is_paid_over_calls_and_reset_starts_over():
    N, skip = 3, 500
    x = _streams(N, 900, seed=3, special=False)
    est = doa.twinrx_phase_offset_est(N, skip)
    o = [np.empty(900, np.float32) for _ in range(N - 1)]
    assert est.work(200, [x[k, :200] for k in range(N)], o) == 0
    assert est.work(200, [x[k, 200:400] for k in range(N)], o) == 0
    assert est.work(200, [x[k, 400:600] for k in range(N)], o) == 100
    assert np.array_equal(_bits(np.stack(o)[:, :100]), _bits(_run_work(doa.twinrx_phase_offset_est(N, 0), x[:, 500:600], [])))
    assert est.work(300, [x[k, 600:] for k in range(N)], o) == 300
    est.reset()
    assert est.work(900, [x[k] for k in range(N)], o) == 400
    assert est.work(0, [x[k] for k in range(N)], o) == 0


def test_atan2_of_zero_is_zero():
    x = np.array([[0 + 0j, 1 + 0j, 0 + 0j, 0 + 1j], [0 + 0j, 0 + 0j, -1 + 0j, 0 - 1j]], dtype=np.complex64)
    out = _run_work(doa.twinrx_phase_offset_est(2, 0), x, [])[0]
    assert out[0] == 0.0 and out[1] == 0.0                      # atan2f(0, 0) = 0
    assert np.abs(out[2:].astype(np.float64) - np.array([-np.pi, np.pi])).max() <= BOUND


def test_a_nan_sample_gives_nan_there_and_touches_no_other():
    N, T = 4, 1030
    x = _streams(N, T, seed=9, special=False)
    clean = _run_work(doa.twinrx_phase_offset_est(N, 0), x, [])
    y = x.copy()
    y[2, 100] = complex(np.nan, 1.0)          # stream 2 -> output 1 at 100
    y[0, 200] = complex(1.0, np.nan)          # stream 0 -> every output at 200
    y[3, 300] = complex(np.inf, 1.0)          # stream 3 -> output 2 at 300
    y[1, 400] = complex(-2.0, -np.inf)        # stream 1 -> output 0 at 400
    y[0, 500] = complex(np.inf, np.inf)       # stream 0 -> every output at 500
    got = _run_work(doa.twinrx_phase_offset_est(N, 0), y, [])
    touched = np.zeros_like(got, dtype=bool)
    touched[1, 100] = touched[:, 200] = touched[2, 300] = touched[0, 400] = touched[:, 500] = True
    assert np.all(np.isnan(got[touched])) and not np.any(np.isnan(got[~touched]))
    assert np.array_equal(_bits(got[~touched]), _bits(clean[~touched]))
    # the fused form over the same samples: the maximum and the mean of an output that holds a NaN are NaN (numpy.amax, numpy.mean)
    mean, mx, circ = doa.twinrx_phase_offset_est(N, 0).estimate(T, [y[k] for k in range(N)], T)
    assert np.all(np.isnan(mx)) and np.all(np.isnan(mean))
    ok = y[:, :90]
    mean, mx, circ = doa.twinrx_phase_offset_est(N, 0).estimate(90, [ok[k] for k in range(N)], 90)
    assert not np.any(np.isnan(mx)) and not np.any(np.isnan(mean)) and not np.any(np.isnan(circ))


def _tone_plus_noise(N, T, seed, snr_db=10.0, phi=None):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-3.1, 3.1, N - 1) if phi is None else phi
    return ref.pilot_capture(N, T, phi, snr_db=snr_db, seed=seed, freq=0.0137)


@pytest.mark.parametrize("N,samples,skip,extra", [(2, 1, 0, 0), (2, 4097, 3, 10), (4, 10001, 123, 0), (4, 64 * 1024 + 5, 0, 7),
                                                  (8, 9000, 8192, 1), (16, 4096 * 3 + 1, 50, 2)])
def test_fused_form_against_the_streaming_form(N, samples, skip, extra):
    T = skip + samples + extra
    x = _tone_plus_noise(N, T, seed=N + samples)
    stream_out = _run_work(doa.twinrx_phase_offset_est(N, skip), x, [])[:, :samples]
    est = doa.twinrx_phase_offset_est(N, skip)
    mean, mx, circ = est.estimate(T, [x[k] for k in range(N)], samples)
    # maximum: bit for bit the maximum of the floats the streaming form writes
    assert np.array_equal(_bits(mx), _bits(stream_out.max(axis=1)))
    # mean: within 1 float32 ulp of the float64 mean of the streaming output
    mean64 = stream_out.astype(np.float64).mean(axis=1)
    print(f"N={N} samples={samples}: |mean - mean64| / ulp = {(np.abs(mean - mean64) / ref.ulp32(mean64)).max():.3f}")
    assert np.all(np.abs(mean.astype(np.float64) - mean64) <= ref.ulp32(mean64))
    # circular mean: within 1e-6 rad of the float64 evaluation, which is well conditioned for these inputs
    circ64, cond = ref.circular_mean64(x, skip, samples)
    assert np.all(cond >= 1e-3), cond
    d = np.abs(np.angle(np.exp(1j * (circ.astype(np.float64) - circ64))))
    print(f"N={N} samples={samples}: |circ - circ64| = {d.max():.3e} rad, conditioning {cond.min():.3f}")
    assert d.max() <= 1e-6
    assert np.all(np.abs(circ) <= np.float32(np.pi))
    # run to run
    est2 = doa.twinrx_phase_offset_est(N, skip)
    again = est2.estimate(T, [x[k] for k in range(N)], samples)
    for a, b in zip((mean, mx, circ), again):
        assert np.array_equal(_bits(a), _bits(b))


def test_fused_form_null_outputs_one_at_a_time_and_too_few_samples():
    N, samples, skip = 4, 5000, 100
    x = _tone_plus_noise(N, skip + samples, seed=1)
    ins = [x[k] for k in range(N)]
    full = doa.twinrx_phase_offset_est(N, skip).estimate(skip + samples, ins, samples)
    for drop in range(3):
        want = [i != drop for i in range(3)]
        got = doa.twinrx_phase_offset_est(N, skip).estimate(skip + samples, ins, samples, *want)
        assert got[drop] is None
        for i in range(3):
            if i != drop:
                assert np.array_equal(_bits(got[i]), _bits(full[i]))
    est = doa.twinrx_phase_offset_est(N, skip)
    with pytest.raises(doa.DoaError, match="fewer than samples"):
        est.estimate(skip + samples - 1, [a[:-1] for a in ins], samples)
    # the refused call took nothing from the skip
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(est.estimate(skip + samples, ins, samples), full))
    with pytest.raises(doa.DoaError):
        est.estimate(10, [a[:10] for a in ins], 0)


def test_device_entries_equal_host_entries_bit_for_bit_over_several_staging_chunks():
    """N = 4 fc32: the host entry stages 2^20 samples per copy, so 2.5 * 2^20 + 13 samples take three copies; the device
    entry sees them in one piece, once on 16-byte aligned streams (16-byte loads) and once on streams that start one
    sample further (one-sample loads)."""
    import torch
    N, skip = 4, 4097
    samples = 5 * 2 ** 19 + 13
    T = skip + samples + 1
    rng = np.random.default_rng(4)
    t = np.arange(T, dtype=np.float32)
    tone = np.exp(2j * np.pi * (0.0137 * t.astype(np.float64) % 1.0)).astype(np.complex64)
    x = np.empty((N, T), np.complex64)
    for k in range(N):
        noise = (rng.standard_normal(2 * T, dtype=np.float32) * np.float32(0.2)).view(np.complex64)
        x[k] = tone * np.complex64(np.exp(-0.9j * k)) + noise
    host = doa.twinrx_phase_offset_est(N, skip).estimate(T, [x[k] for k in range(N)], samples)
    res = torch.empty((3, N - 1), dtype=torch.float32, device="cuda")
    routes = set()
    for shift in (0, 1):
        dev = doa.sim.stream_slab_torch([torch.from_numpy(np.concatenate([np.zeros(shift, np.complex64), x[k]])).cuda() for k in range(N)])
        ptrs = [d.data_ptr() + 8 * shift for d in dev]
        routes.add(all((p + 8 * skip) % 16 == 0 for p in ptrs))
        est = doa.twinrx_phase_offset_est(N, skip)
        res.fill_(-9.0)
        est.estimate_dev(T, ptrs, samples, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), torch.cuda.current_stream())
        torch.cuda.synchronize()
        got = res.cpu().numpy()
        for i in range(3):
            assert np.array_equal(_bits(got[i]), _bits(host[i])), (shift, i)
        # NULL pointers on the device entry, one at a time
        for drop in range(3):
            res.fill_(-9.0)
            est.reset()
            p3 = [0 if i == drop else res[i].data_ptr() for i in range(3)]
            est.estimate_dev(T, ptrs, samples, *p3, stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
            g2 = res.cpu().numpy()
            assert np.all(g2[drop] == -9.0)
            assert all(np.array_equal(_bits(g2[i]), _bits(host[i])) for i in range(3) if i != drop)
    assert routes == {True, False}
    # the streaming device entry against the host one, on the same streams
    n = 100001
    outs = torch.empty((N - 1, n), dtype=torch.float32, device="cuda")
    est = doa.twinrx_phase_offset_est(N, skip)
    assert est.work_dev(n, ptrs, [outs[p].data_ptr() for p in range(N - 1)], torch.cuda.current_stream()) == n - skip
    torch.cuda.synchronize()
    want = _run_work(doa.twinrx_phase_offset_est(N, skip), x[:, :n], [])
    assert np.array_equal(_bits(outs.cpu().numpy()[:, :n - skip]), _bits(want))


@pytest.mark.parametrize("scale", [1.0 / 32768, 3.0517578e-5 * 1.37])
@pytest.mark.parametrize("N,T,skip", [(2, 5001, 0), (4, 20011, 1001), (16, 4099, 2)])
def test_sc16_is_bit_identical_to_fc32_on_the_widened_samples(N, T, skip, scale):
    rng = np.random.default_rng(N + T)
    q = rng.integers(-32768, 32768, size=(N, T, 2), dtype=np.int16)
    q[:, :4] = [[0, 0], [32767, -32768], [-32768, 0], [0, 1]]
    x = doa.sim.from_sc16(q, scale)
    assert np.array_equal(x.real, q[..., 0].astype(np.float32) * np.float32(scale))
    samples = T - skip - 3
    f_est = doa.twinrx_phase_offset_est(N, skip)
    f_stream = _run_work(f_est, x, [T // 3])
    f_fused = doa.twinrx_phase_offset_est(N, skip).estimate(T, [x[k] for k in range(N)], samples)
    s_est = doa.twinrx_phase_offset_est(N, skip)
    s_est.set_input_format("sc16", scale)
    outs, done = [], 0
    for a, b in ((0, T // 3), (T // 3, T)):
        o = [np.empty(b - a, np.float32) for _ in range(N - 1)]
        got = s_est.work(b - a, [q[k, a:b] for k in range(N)], o)
        outs.append(np.stack([v[:got] for v in o]))
    assert np.array_equal(_bits(np.concatenate(outs, axis=1)), _bits(f_stream))
    s_est.reset()
    s_fused = s_est.estimate(T, [q[k] for k in range(N)], samples)
    for a, b in zip(s_fused, f_fused):
        assert np.array_equal(_bits(a), _bits(b))
    with pytest.raises(doa.DoaError):
        s_est.set_input_format("fc32", 0.5)
    with pytest.raises(doa.DoaError):
        s_est.set_input_format("sc16", 0.0)
