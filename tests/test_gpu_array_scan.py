"""GPU tests of the steering-table estimators: doa.MUSIC_array and doa.capon_array against the numpy statement
(tests/array_ref.py) to the project's bounds for the double path (tests/test_gpu_music.py, tests/test_gpu_capon.py), a table
with gains, the cross-check against the ULA blocks, Capon's failure containment and scale invariance, batch boundaries, and
music_pipeline.set_steering_table against the chain of blocks, bit for bit.

The comparisons print their figures as fractions of the bounds before they assert; run with -s to see them
(profiles/array_scan_test_figures.txt holds one such run)."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import array_ref as ref
import capon_ref
from test_gpu_capon import BAD_AT, _bad_items, _spoil_unread_parts, _wishart

pytestmark = pytest.mark.gpu

N_BLOCK = 67                       # a partial workgroup of the scan (8 and 4 items) and a partial wave of every stage in front
ESTIMATORS = ("music", "capon")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _items(N):
    """67 covariance items of the scenario for N, unread parts spoiled; read-only."""
    R = _spoil_unread_parts(ref.covariance(ref.NAME_OF_N[N], N_BLOCK), N)
    R.setflags(write=False)
    return R


def _sources(N):
    return ref.SCENARIOS[ref.NAME_OF_N[N]][1]


@functools.lru_cache(maxsize=None)
def _table(N, P):
    t = ref.planar_table(ref.SCENARIOS[ref.NAME_OF_N[N]][0], P)
    t.setflags(write=False)
    return t


def _make(est, table, M, delta):
    return doa.MUSIC_array(M, table) if est == "music" else doa.capon_array(table, delta)


def _reference(est, R, table, M, delta):
    """(spectrum, Q, X, status) of the numpy statement."""
    if est == "music":
        s, q, X = ref.music(R, table, M)
        return s, q, X, np.zeros(R.shape[0], np.int32)
    return ref.capon(R, table, delta)


def _block_dev(est, table, M, delta, R):
    """(spectrum [n, P], status [n]) of work_dev; MUSIC has no status output (zeros)."""
    n, P = R.shape[0], table.shape[0]
    dR = _dev(R)
    spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    st = torch.zeros((n,), dtype=torch.int32, device="cuda")
    blk = _make(est, table, M, delta)
    if est == "music":
        assert blk.work_dev(n, dR.data_ptr(), spec.data_ptr(), torch.cuda.current_stream()) == n
    else:
        st.fill_(-7)
        assert blk.work_dev(n, dR.data_ptr(), spec.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    assert blk.nout_items_total() == n
    return spec.cpu().numpy(), st.cpu().numpy()


def _check_against_the_definition(label, est, R, table, M, delta):
    """Bounds (a), (b), (d) of the double path; prints each figure as a fraction of its bound."""
    n, (P, N) = R.shape[0], table.shape
    s_ref, q_ref, X_ref, st_ref = _reference(est, R, table, M, delta)
    assert np.all(st_ref == 0)
    spec, st = _block_dev(est, table, M, delta, R)
    X, q = _make(est, table, M, delta).debug(R)
    assert np.all(st == 0)
    e_x = e_q = e_s = 0.0
    for i in range(n):
        Xi = X[i].reshape(N, N, order="F")
        bound_x = 1e-7 if est == "music" else 3e-7 * np.abs(X_ref[i]).max()
        e_x = max(e_x, float(np.abs(Xi - X_ref[i]).max() / bound_x))
        e_q = max(e_q, float((np.abs(q[i] - q_ref[i]) / (3e-7 * np.abs(q_ref[i]) + 2e-13 * q_ref[i].max())).max()))
        e_s = max(e_s, float((np.abs(spec[i] - s_ref[i]) / (2e-5 + 2e-6 * np.abs(s_ref[i]))).max()))
    print("%s %s N=%d P=%d delta=%g: matrix %.3g, null spectrum %.3g, dB row %.3g of the bounds" % (label, est, N, P, delta, e_x, e_q, e_s))
    assert e_x <= 1.0 and e_q <= 1.0 and e_s <= 1.0
    assert np.all(spec.max(axis=1) == 0.0)
    assert np.array_equal(np.argmax(spec, axis=1), np.argmax(s_ref, axis=1))


# ---- 1: the blocks against the definition -----------------------------------------------------------------------------
BLOCK_CASES = [(3, 720), (4, 720), (5, 720), (8, 720), (11, 720), (16, 720), (4, 1024), (16, 4096), (5, 181), (8, 63), (8, 65),
               (4, 1)]
EST_CASES = [("music", 0.0), ("capon", 0.0), ("capon", 1e-2)]


@pytest.mark.parametrize("est,delta", EST_CASES)
@pytest.mark.parametrize("N,P", BLOCK_CASES)
def test_blocks_match_the_definition(N, P, est, delta):
    R = _items(N)
    if est == "capon":
        cond = capon_ref.condition_numbers(R, N, delta).max()
        assert cond <= 1e5, cond                    # what the double-path bounds below rest on
    _check_against_the_definition("scenario", est, R, _table(N, P), len(_sources(N)), delta)


# rows beyond the 4-items-per-workgroup form: one item per workgroup (4096 < P <= 16384), and the form that keeps no row in LDS
@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("P", [4097, 16384, 16385])
def test_long_rows_match_the_definition(P, est):
    N = 4
    _check_against_the_definition("long row", est, _items(N)[:9], _table(N, P), len(_sources(N)), 0.0)


# ---- 2: a table with gains --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
def test_table_with_gains(est):
    """Rows that are not of unit modulus: the |a_n|^2 terms of the bilinear form."""
    N, P = 8, 720
    rng = np.random.default_rng(11)
    g = rng.uniform(0.5, 2.0, N) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, N))
    table = _table(N, P) * g[None, :]
    assert np.abs(np.abs(table) - 1.0).max() > 0.4
    _check_against_the_definition("gains", est, _items(N), table, len(_sources(N)), 0.0)


# ---- 3: the ULA cross-check -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("row", [0, 2, 3])
def test_ula_table_agrees_with_the_ula_blocks(row, est):
    """With the ULA's own steering table the general blocks and the ULA blocks are within the dB bound of the same oracle,
    hence within twice the bound of each other, and they pick the same peaks."""
    N, thetas, snr_db, K, delta, d = capon_ref.TABLE[row]
    M, P = len(thetas), capon_ref.P
    R = capon_ref.row_covariance(row)
    n = R.shape[0]
    table = np.ascontiguousarray(oracle.music_steering(d, N, P, "f64").T)
    got, st = _block_dev(est, table, M, delta, R)
    assert np.all(st == 0)
    lin = doa.MUSIC_lin_array(d, M, N, P) if est == "music" else doa.capon_lin_array(d, N, P, delta)
    want = np.empty((n, P), np.float32)
    assert lin.work(n, [R], [want]) == n
    e = float((np.abs(got.astype(np.float64) - want) / (2.0 * (2e-5 + 2e-6 * np.abs(want.astype(np.float64))))).max())
    print("ULA cross-check %s row %d (N=%d): largest dB difference %.3g of twice the bound" % (est, row, N, e))
    assert e <= 1.0
    _, loc_a = oracle.find_local_max(got, M, P, 0.0, 180.0)
    _, loc_b = oracle.find_local_max(want, M, P, 0.0, 180.0)
    assert np.array_equal(loc_a, loc_b)


# ---- 4: Capon's failures are contained --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 8, 16])
def test_capon_failures_are_contained(N):
    P = 256
    table = _table(N, P)
    R = np.array(_items(N))
    clean, st_clean = _block_dev("capon", table, 0, 0.0, R)
    assert np.all(st_clean == 0)
    for pos, item in zip(BAD_AT, _bad_items(N, R[2])):
        R[pos] = item
    spec, st = _block_dev("capon", table, 0, 0.0, R)
    want = np.zeros(N_BLOCK, np.int32); want[list(BAD_AT)] = 1
    assert np.array_equal(st, want), st
    nan_rows = np.isnan(spec).all(axis=1)
    assert np.array_equal(nan_rows, want == 1) and not np.isnan(spec[want == 0]).any()
    assert _same(spec[want == 0], clean[want == 0])
    blk = doa.capon_array(table, 0.0)
    h_spec, h_st = np.empty((N_BLOCK, P), np.float32), np.empty(N_BLOCK, np.int32)
    assert blk.work(N_BLOCK, [R], [h_spec, h_st]) == N_BLOCK
    assert np.array_equal(h_st, want) and _same(h_spec, spec)


# ---- 5: scale invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, 1e-2])
@pytest.mark.parametrize("N", [4, 8, 16])
def test_capon_scale_invariance(N, delta):
    R, table = _items(N), _table(N, 256)
    base, st = _block_dev("capon", table, 0, delta, R)
    assert np.all(st == 0)
    for factor in (2.0 ** 40, 2.0 ** -40):
        scaled = (R * np.float32(factor)).astype(np.complex64)          # exact in float
        got, st = _block_dev("capon", table, 0, delta, scaled)
        assert np.all(st == 0) and _same(got, base), (N, delta, factor)


# ---- 6: batch boundaries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("N", [4, 16])
def test_batch_boundaries(N, est):
    P, sizes, M, delta = 256, (1, 63, 64, 65, 4097), 2, 1e-3
    table = _table(N, P)
    R = _wishart(N, max(sizes), 40 + N)
    full, st = _block_dev(est, table, M, delta, R)
    assert np.all(st == 0)
    blk = _make(est, table, M, delta)
    for n in sizes[:-1]:
        got, st = _block_dev(est, table, M, delta, R[:n])
        assert np.all(st == 0) and _same(got, full[:n]), (N, n)
        h = np.full((n, P), -7.0, np.float32)
        assert blk.work(n, [R[:n]], [h]) == n
        assert _same(h, full[:n]), (N, n, "host")
    h = np.full((max(sizes), P), -7.0, np.float32)
    assert blk.work(max(sizes), [R], [h]) == max(sizes) and _same(h, full)
    untouched = np.full((2, P), -7.0, np.float32)
    assert blk.work(0, [R], [untouched]) == 0 and np.all(untouched == -7.0)
    if est == "music":
        assert blk.work_dev(0, 0, 0, torch.cuda.current_stream()) == 0
    else:
        assert blk.work_dev(0, 0, 0, None, torch.cuda.current_stream()) == 0


def test_precision_32_is_unsupported():
    table = _table(4, 256)
    R = _items(4)[:1]
    out = np.empty((1, 256), np.float32)
    doa.set_internal_precision(32)
    try:
        blocks = [doa.MUSIC_array(1, table), doa.capon_array(table, 0.0)]
    finally:
        doa.set_internal_precision(64)
    for blk in blocks:
        with pytest.raises(doa.DoaError) as ei:
            blk.work(1, [R], [out])
        assert ei.value.status == -4
    blk = doa.MUSIC_array(1, table)
    blk.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        blk.work(1, [R], [out])
    assert ei.value.status == -4
    blk.set_internal_precision(64)
    assert blk.work(1, [R], [out]) == 1 and out.max() == 0.0


# ---- 7: the pipeline --------------------------------------------------------------------------------------------------
NP_, DELTA = 15, 1e-3               # snapshots per pipeline case (3 batches of 5), the loading of the Capon pipeline tests
# scenario -> (peaks, P)
PIPE_CASES = {"uca5": (2, 720), "uca8": (3, 720), "uca16": (3, 4096)}


def _case(name):
    pos, src, snr_db, K = ref.SCENARIOS[name]
    M, P = PIPE_CASES[name]
    return pos.shape[0], K, M, P, src


@functools.lru_cache(maxsize=None)
def _pipe_table(name):
    t = ref.planar_table(ref.SCENARIOS[name][0], PIPE_CASES[name][1])
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _dev_streams(name):
    return tuple(doa.sim.stream_slab_torch([_dev(a) for a in ref.streams(name, NP_)]))


class _Out:
    def __init__(self, N, M, P, n, spec=True):
        self.cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
        self.spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda") if spec else None
        self.mx = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
        self.am = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in vars(self).items()}


def _pipe(name, est, table=True):
    N, K, M, P, src = _case(name)
    p = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=NP_)
    if est == "capon":
        p.set_estimator("capon", DELTA)
    if table:
        p.set_steering_table(_pipe_table(name), 0.0, 360.0)
    return p


def _work_dev(pipe, name, spec=True):
    N, K, M, P, src = _case(name)
    o = _Out(N, M, P, NP_, spec)
    ptrs = [t.data_ptr() for t in _dev_streams(name)]
    assert pipe.work_dev(NP_, ptrs, o.cov.data_ptr(), o.spec.data_ptr() if spec else 0, o.mx.data_ptr(), o.am.data_ptr(),
                         torch.cuda.current_stream()) == NP_
    return o.host()


@functools.lru_cache(maxsize=None)
def _table_run(name, est):
    return _work_dev(_pipe(name, est), name)


@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("name", sorted(PIPE_CASES))
def test_pipeline_equals_the_chain_of_blocks(name, est):
    N, K, M, P, src = _case(name)
    got = _table_run(name, est)
    st = torch.cuda.current_stream()
    cov = torch.empty((NP_, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((NP_, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((NP_, M), dtype=torch.float32, device="cuda")
    am = torch.empty((NP_, M), dtype=torch.float32, device="cuda")
    doa.autocorrelate(N, K, 0, 0).work_dev(NP_, [t.data_ptr() for t in _dev_streams(name)], cov.data_ptr(), st)
    if est == "music":
        doa.MUSIC_array(M, _pipe_table(name)).work_dev(NP_, cov.data_ptr(), spec.data_ptr(), st)
    else:
        doa.capon_array(_pipe_table(name), DELTA).work_dev(NP_, cov.data_ptr(), spec.data_ptr(), None, st)
    doa.find_local_max(M, P, 0.0, 360.0).work_dev(NP_, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    torch.cuda.synchronize()
    for key, want in (("cov", cov), ("spec", spec), ("mx", mx), ("am", am)):
        assert _same(got[key], want.cpu().numpy()), (name, est, key)
    err = ref.angle_error(got["am"], src)
    print(name, est, "pipeline with a table: max angle error %.3f deg (cap %.3f)" % (err, ref.angle_cap(P)))
    assert err <= ref.angle_cap(P)


@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("name", sorted(PIPE_CASES))
def test_pipeline_other_entries(name, est):
    N, K, M, P, src = _case(name)
    want = _table_run(name, est)
    pipe = _pipe(name, est)
    # angles only
    lean = _work_dev(pipe, name, spec=False)
    assert _same(lean["mx"], want["mx"]) and _same(lean["am"], want["am"]) and _same(lean["cov"], want["cov"])
    # host entry
    x = ref.streams(name, NP_)
    h = {"mx": np.empty((NP_, M), np.float32), "am": np.empty((NP_, M), np.float32),
         "cov": np.empty((NP_, N * N), np.complex64), "spec": np.empty((NP_, P), np.float32)}
    assert pipe.work(NP_, [x[k] for k in range(N)], h["mx"], h["am"], cov_out=h["cov"], spectrum_out=h["spec"]) == NP_
    for key in ("cov", "spec", "mx", "am"):
        assert _same(h[key], want[key]), (name, est, "host", key)
    # three batches of five, on the caller's stream alone and over two lanes
    nb, n = 3, NP_ // 3
    streams = _dev_streams(name)
    ins = [[t.data_ptr() + b * n * K * 8 for t in streams] for b in range(nb)]
    for lanes in (1, 2):
        pipe.set_lanes(lanes)
        o = _Out(N, M, P, NP_)
        rows = lambda t, per: [t.data_ptr() + b * n * per * t.element_size() for b in range(nb)]
        assert pipe.work_dev_batches(n, ins, rows(o.cov, N * N), rows(o.spec, P), rows(o.mx, M), rows(o.am, M),
                                     torch.cuda.current_stream()) == NP_
        got = o.host()
        for key in ("cov", "spec", "mx", "am"):
            assert _same(got[key], want[key]), (name, est, "batches", lanes, key)


@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("name", sorted(PIPE_CASES))
def test_pipeline_clearing_the_table_restores_the_ula(name, est):
    fresh = _work_dev(_pipe(name, est, table=False), name)
    pipe = _pipe(name, est)
    with_table = _work_dev(pipe, name)
    assert not _same(with_table["spec"], fresh["spec"])
    pipe.set_steering_table(None)
    back = _work_dev(pipe, name)
    for key in ("cov", "spec", "mx", "am"):
        assert _same(back[key], fresh[key]), (name, est, key)


def test_pipeline_limits():
    name = "uca5"
    N, K, M, P, src = _case(name)
    table = _pipe_table(name)
    pipe = _pipe(name, "music")
    want = _table_run(name, "music")
    o = _Out(N, M, P, NP_)
    cnt = torch.zeros((NP_,), dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in _dev_streams(name)]

    def still_works():
        got = _work_dev(pipe, name)
        for key in ("cov", "spec", "mx", "am"):
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
    # bad tables and axes leave the table that is set
    bad = np.array(table); bad[7, 1] = np.nan
    for tab, lo, hi in ((bad, 0.0, 360.0), (table, 10.0, 10.0), (table, 0.0, float("nan"))):
        with pytest.raises(doa.DoaError) as ei:
            pipe.set_steering_table(tab, lo, hi)
        assert ei.value.status == -1
    with pytest.raises(ValueError):
        pipe.set_steering_table(table[:, :N - 1])
    with pytest.raises(ValueError):
        pipe.set_steering_table(table[:P - 1])
    still_works()
    # a table while smoothing is on
    smoothed = _pipe(name, "music", table=False)
    fresh = _work_dev(smoothed, name)
    smoothed.set_spatial_smoothing(4, True)
    with pytest.raises(doa.DoaError) as ei:
        smoothed.set_steering_table(table)
    assert ei.value.status == -4 and smoothed.steering_table is None
    smoothed.set_spatial_smoothing(0)
    back = _work_dev(smoothed, name)
    for key in ("cov", "spec", "mx", "am"):
        assert _same(back[key], fresh[key]), key
