"""GPU tests of music_pipeline's grid mode (set_steering_grid): the three circular scenarios of peaks2d_ref.py on their 72 x 18
grid, K = 512, 15 snapshots, MUSIC and Capon -- every entry against the chain autocorrelate -> MUSIC_array | capon_array ->
find_local_max_2d on the device, bit for bit; every source within one cell; a failed Capon item contained; the limits."""
import functools

import numpy as np
import pytest
import torch

import doa
import peaks2d_ref as p2

pytestmark = pytest.mark.gpu

NP_, DELTA = 15, 1e-3                # snapshots per case (3 batches of 5); the loading of the existing Capon array tests
N_AZ, N_EL, K, P = p2.N_AZ, p2.N_EL, p2.K, p2.N_AZ * p2.N_EL
ESTIMATORS = ("music", "capon")
KEYS = ("cov", "spec", "mx", "am")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the cached host arrays are read-only


def _case(name):
    N, radius, sources = p2.CIRCULAR[name]
    return N, len(sources), sources


@functools.lru_cache(maxsize=None)
def _table(name):
    N, radius, _ = p2.CIRCULAR[name]
    t = doa.planar_steering_grid(p2.circular_positions(N, radius), N_AZ, N_EL)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _host_streams(name):
    x = p2.streams(name, NP_)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _dev_streams(name):
    return tuple(doa.sim.stream_slab_torch([_dev(a) for a in _host_streams(name)]))


class _Out:
    def __init__(self, N, M, n, spec=True, am_width=None):
        self.cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
        self.spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda") if spec else None
        self.mx = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
        self.am = torch.full((n, 2 * M if am_width is None else am_width), -7.0, dtype=torch.float32, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in vars(self).items()}


def _pipe(name, est, grid=True, cls=None, **kw):
    N, M, _ = _case(name)
    p = (cls or doa.music_pipeline)(N, K, 0, 0, 0.5, M, P, max_batch=NP_, **kw)
    if est == "capon":
        p.set_estimator("capon", DELTA)
    if grid:
        p.set_steering_grid(_table(name), N_AZ, N_EL)
    return p


def _work_dev(pipe, name, spec=True, streams=None, am_width=None):
    N, M, _ = _case(name)
    o = _Out(N, M, NP_, spec, am_width)
    ptrs = [t.data_ptr() for t in (streams or _dev_streams(name))]
    assert pipe.work_dev(NP_, ptrs, o.cov.data_ptr(), o.spec.data_ptr() if spec else 0, o.mx.data_ptr(), o.am.data_ptr(),
                         torch.cuda.current_stream()) == NP_
    return o.host()


@functools.lru_cache(maxsize=None)
def _grid_run(name, est):
    return _work_dev(_pipe(name, est), name)


def _chain(name, est, cov_items=None):
    """autocorrelate -> MUSIC_array | capon_array -> find_local_max_2d on the device: cov, spec, mx, az, el (and the status)."""
    N, M, _ = _case(name)
    st = torch.cuda.current_stream()
    cov = torch.empty((NP_, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((NP_, P), dtype=torch.float32, device="cuda")
    mx, az, el = [torch.empty((NP_, M), dtype=torch.float32, device="cuda") for _ in range(3)]
    status = torch.zeros((NP_,), dtype=torch.int32, device="cuda")
    if cov_items is None:
        doa.autocorrelate(N, K, 0, 0).work_dev(NP_, [t.data_ptr() for t in _dev_streams(name)], cov.data_ptr(), st)
    else:
        cov.copy_(cov_items)
    if est == "music":
        doa.MUSIC_array(M, _table(name)).work_dev(NP_, cov.data_ptr(), spec.data_ptr(), st)
    else:
        doa.capon_array(_table(name), DELTA).work_dev(NP_, cov.data_ptr(), spec.data_ptr(), status.data_ptr(), st)
    doa.find_local_max_2d(M, N_AZ, N_EL, 0.0, 360.0, 0.0, 90.0, True).work_dev(NP_, spec.data_ptr(), mx.data_ptr(), az.data_ptr(),
                                                                            el.data_ptr(), st)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(cov=cov, spec=spec, mx=mx, az=az, el=el, status=status).items()}


@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("name", sorted(p2.CIRCULAR))
def test_grid_mode_equals_the_chain_of_blocks(name, est):
    N, M, sources = _case(name)
    got, want = _grid_run(name, est), _chain(name, est)
    for key in ("cov", "spec", "mx"):
        assert _same(got[key], want[key]), (name, est, key)
    assert got["am"].shape == (NP_, 2 * M)
    assert _same(np.ascontiguousarray(got["am"][:, :M]), want["az"]), (name, est, "azimuths")
    assert _same(np.ascontiguousarray(got["am"][:, M:]), want["el"]), (name, est, "elevations")
    for d in range(NP_):
        assert got["mx"][d, 0] == 0.0 and p2.sources_found(got["am"][d, :M], got["am"][d, M:], sources), (name, est, d, got["am"][d])


@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("name", sorted(p2.CIRCULAR))
def test_grid_mode_other_entries(name, est):
    N, M, _ = _case(name)
    want = _grid_run(name, est)
    pipe = _pipe(name, est)
    # angles only
    lean = _work_dev(pipe, name, spec=False)
    assert all(_same(lean[k], want[k]) for k in ("cov", "mx", "am")), (name, est, "angles only")
    # the host entry: argmax 2 M wide, and its shape is checked
    x = _host_streams(name)
    h = {"mx": np.empty((NP_, M), np.float32), "am": np.empty((NP_, 2 * M), np.float32),
         "cov": np.empty((NP_, N * N), np.complex64), "spec": np.empty((NP_, P), np.float32)}
    assert pipe.work(NP_, [x[k] for k in range(N)], h["mx"], h["am"], cov_out=h["cov"], spectrum_out=h["spec"]) == NP_
    for key in KEYS:
        assert _same(h[key], want[key]), (name, est, "host", key)
    with pytest.raises(ValueError):
        pipe.work(NP_, [x[k] for k in range(N)], h["mx"], np.empty((NP_, M), np.float32))
    # three batches of five, on the caller's stream alone and over two lanes
    nb, n = 3, NP_ // 3
    streams = _dev_streams(name)
    ins = [[t.data_ptr() + b * n * K * 8 for t in streams] for b in range(nb)]
    for lanes in (1, 2):
        pipe.set_lanes(lanes)
        o = _Out(N, M, NP_)
        rows = lambda t, per: [t.data_ptr() + b * n * per * t.element_size() for b in range(nb)]      # noqa: E731
        assert pipe.work_dev_batches(n, ins, rows(o.cov, N * N), rows(o.spec, P), rows(o.mx, M), rows(o.am, 2 * M),
                                     torch.cuda.current_stream()) == NP_
        got = o.host()
        for key in KEYS:
            assert _same(got[key], want[key]), (name, est, "batches", lanes, key)


@pytest.mark.parametrize("name", sorted(p2.CIRCULAR))
def test_the_sc16_handle_equals_the_fc32_handle_on_the_widened_streams(name):
    scale = 2.0 ** -15
    x = _host_streams(name)
    q = doa.sim.to_sc16(x / max(np.abs(x.real).max(), np.abs(x.imag).max()) * (0.25 * 32767 * scale), scale)      # 1/4 of full scale
    wide = doa.sim.stream_slab_torch([_dev(a) for a in doa.sim.from_sc16(q, scale)])
    narrow = doa.sim.stream_slab_torch([_dev(a) for a in q])
    want = _work_dev(_pipe(name, "music"), name, streams=wide)
    got = _work_dev(_pipe(name, "music", cls=doa.music_pipeline_sc16, scale=scale), name, streams=narrow)
    for key in KEYS:
        assert _same(got[key], want[key]), (name, key)


def test_a_failed_capon_item_is_contained():
    name, bad = "uca8", 7
    N, M, _ = _case(name)
    clean = _grid_run(name, "capon")
    x = np.array(_host_streams(name))
    x[:, bad * K:(bad + 1) * K] = 0                    # a zero covariance item
    streams = doa.sim.stream_slab_torch([_dev(a) for a in x])
    got = _work_dev(_pipe(name, "capon"), name, streams=streams)
    assert not got["cov"][bad].any()
    assert np.isnan(got["spec"][bad]).all() and np.isnan(got["mx"][bad]).all() and np.isnan(got["am"][bad]).all()
    keep = np.arange(NP_) != bad
    for key in KEYS:
        assert _same(got[key][keep], clean[key][keep]), key
    # what the chain of blocks gives for the same items, status included
    want = _chain(name, "capon", cov_items=_dev(got["cov"]))
    status = np.zeros(NP_, np.int32); status[bad] = 1
    assert np.array_equal(want["status"], status)
    assert _same(got["spec"], want["spec"]) and _same(got["mx"], want["mx"])
    assert _same(np.ascontiguousarray(got["am"][:, :M]), want["az"]) and _same(np.ascontiguousarray(got["am"][:, M:]), want["el"])
    # angles only: the same peaks
    lean = _work_dev(_pipe(name, "capon"), name, spec=False, streams=streams)
    assert _same(lean["mx"], got["mx"]) and _same(lean["am"], got["am"])


def test_limits_and_state():
    name = "uca5"
    N, M, _ = _case(name)
    table = _table(name)
    pipe = _pipe(name, "music")
    want = _grid_run(name, "music")
    o = _Out(N, M, NP_)
    cnt = torch.zeros((NP_,), dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in _dev_streams(name)]

    def still_works():
        got = _work_dev(pipe, name)
        for key in KEYS:
            assert _same(got[key], want[key]), key

    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_auto(NP_, ptrs, o.mx.data_ptr(), o.am.data_ptr(), cnt.data_ptr())
    assert ei.value.status == -4
    still_works()
    with pytest.raises(doa.DoaError) as ei:
        pipe.set_spatial_smoothing(4, True)
    assert ei.value.status == -4 and pipe.subarray_size == 0
    still_works()
    pipe.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        _work_dev(pipe, name)
    assert ei.value.status == -4
    pipe.set_internal_precision(64)
    still_works()
    # a grid that does not match pspectrum_len, bad limits and a NaN in the table leave the grid that was set
    bad = np.array(table); bad[7, 1] = np.nan
    for tab, na, ne, kw in ((table, N_AZ, N_EL - 1, {}), (table, N_AZ + 1, N_EL, {}), (table, N_AZ, N_EL, dict(az_min=10.0, az_max=10.0)),
                            (table, N_AZ, N_EL, dict(az_min=20.0, az_max=10.0)), (bad, N_AZ, N_EL, {})):
        with pytest.raises(doa.DoaError) as ei:
            pipe.set_steering_grid(tab, na, ne, **kw)
        assert ei.value.status == -1 and pipe.steering_grid == (N_AZ, N_EL), (na, ne, kw)
    still_works()
    # a plain table after a grid: a fresh table handle's bits, argmax M wide again
    flat = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=NP_)
    flat.set_steering_table(table, 0.0, 360.0)
    want_flat = _work_dev(flat, name, am_width=M)
    pipe.set_steering_table(table, 0.0, 360.0)
    assert pipe.steering_grid is None
    got = _work_dev(pipe, name, am_width=M)
    for key in KEYS:
        assert _same(got[key], want_flat[key]), ("table after grid", key)
    # the grid again, then no table at all: the uniform linear array of a fresh handle
    pipe.set_steering_grid(table, N_AZ, N_EL)
    still_works()
    pipe.set_steering_table(None)
    fresh = _work_dev(_pipe(name, "music", grid=False), name, am_width=M)
    back = _work_dev(pipe, name, am_width=M)
    for key in KEYS:
        assert _same(back[key], fresh[key]), ("cleared", key)
    # a grid while smoothing is on
    smoothed = _pipe(name, "music", grid=False)
    smoothed.set_spatial_smoothing(4, True)
    with pytest.raises(doa.DoaError) as ei:
        smoothed.set_steering_grid(table, N_AZ, N_EL)
    assert ei.value.status == -4 and smoothed.steering_grid is None and smoothed.steering_table is None
    smoothed.set_spatial_smoothing(0)
    back = _work_dev(smoothed, name, am_width=M)
    for key in KEYS:
        assert _same(back[key], fresh[key]), ("after the refused grid", key)
