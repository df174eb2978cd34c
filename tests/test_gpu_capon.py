"""GPU tests of the Capon estimator: the block doa.capon_lin_array against the numpy statement (tests/capon_ref.py) to the
project's bounds for the double path (tests/test_gpu_music.py), its failure containment, scale invariance and batch
boundaries, and music_pipeline.set_estimator("capon") against the chain of blocks, bit for bit.

The comparisons print their figures as fractions of the bounds before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import capon_ref as ref
import spatial_smooth_ref as ssref

pytestmark = pytest.mark.gpu

# the table row that generates the items of each array size
ROW_OF_N = {4: 0, 8: 2, 16: 3, 3: 5, 2: 6, 5: 7, 11: 8}
N_BLOCK = 67                       # a partial wave for every group width (64, 8 and 4 items per wave)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _spoil_unread_parts(R, N):
    """Strict lower triangle NaN, imaginary part of the diagonal 7.0: neither may be read."""
    R = np.array(R).reshape(-1, N, N)                       # [item][col][row]
    for col in range(N):
        R[:, col, col + 1:] = np.nan + 1j * np.nan
        R[:, col, col] = R[:, col, col].real + 7.0j
    return R.reshape(-1, N * N)


@functools.lru_cache(maxsize=None)
def _items(N):
    """67 covariance items of the table's generator for N, unread parts spoiled; read-only."""
    n_, thetas, snr_db, K, delta, d = ref.TABLE[ROW_OF_N[N]]
    R = _spoil_unread_parts(ref.covariance(N, thetas, snr_db, K, d, N_BLOCK), N)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _reference(N, delta, P):
    d = ref.TABLE[ROW_OF_N[N]][5]
    return ref.capon(_items(N), d, N, P, delta)


def _block_dev(N, P, delta, R, d=None):
    """(spectrum [n, P], status [n]) of work_dev."""
    d = ref.TABLE[ROW_OF_N[N]][5] if d is None else d
    n = R.shape[0]
    dR = _dev(R)
    spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    blk = doa.capon_lin_array(d, N, P, delta)
    assert blk.work_dev(n, dR.data_ptr(), spec.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    assert blk.nout_items_total() == n
    return spec.cpu().numpy(), st.cpu().numpy()


# ---- 1: the block against the definition ------------------------------------------------------------------------------
BLOCK_CASES = [(N, 256) for N in (2, 3, 4, 5, 8, 11, 16)] + [(4, 1024), (16, 4096)]


@pytest.mark.parametrize("delta", [0.0, 1e-2])
@pytest.mark.parametrize("N,P", BLOCK_CASES)
def test_block_matches_the_definition(N, P, delta):
    R = _items(N)
    d = ref.TABLE[ROW_OF_N[N]][5]
    cond = ref.condition_numbers(R, N, delta).max()
    assert cond <= 1e5, cond                        # what the double-path bounds below rest on
    s_ref, q_ref, W_ref, st_ref = _reference(N, delta, P)
    assert np.all(st_ref == 0)
    spec, st = _block_dev(N, P, delta, R)
    W, q = doa.capon_lin_array(d, N, P, delta).debug(R)
    assert np.all(st == 0)
    e_w = e_q = e_s = 0.0
    for i in range(N_BLOCK):
        Wi = W[i].reshape(N, N, order="F")
        e_w = max(e_w, float(np.abs(Wi - W_ref[i]).max() / (3e-7 * np.abs(W_ref[i]).max())))
        e_q = max(e_q, float((np.abs(q[i] - q_ref[i]) / (3e-7 * np.abs(q_ref[i]) + 2e-13 * q_ref[i].max())).max()))
        e_s = max(e_s, float((np.abs(spec[i] - s_ref[i]) / (2e-5 + 2e-6 * np.abs(s_ref[i]))).max()))
    print("N=%d P=%d delta=%g cond %.3g: inverse %.3g, null spectrum %.3g, dB row %.3g of the bounds" % (N, P, delta, cond, e_w, e_q, e_s))
    assert e_w <= 1.0 and e_q <= 1.0 and e_s <= 1.0
    assert np.all(spec.max(axis=1) == 0.0)
    assert np.array_equal(np.argmax(spec, axis=1), np.argmax(s_ref, axis=1))


# ---- 2: failures are contained ----------------------------------------------------------------------------------------
BAD_AT = (1, 9, 30, 63, 65)         # each shares its wave (N = 4) or its wave's other lane groups (N = 8, 16) with good items


def _bad_items(N, good):
    ones = np.ones(N * N, np.complex64)
    zero = np.zeros(N * N, np.complex64)
    minus_eye = -np.eye(N, dtype=np.complex64).reshape(-1)
    one_nan = np.array(good); one_nan[0 + (N - 1) * N] = np.nan           # upper triangle: row 0, last column
    one_inf = np.array(good); one_inf[1 + 1 * N] = np.inf                 # on the diagonal
    return [ones, zero, minus_eye, one_nan, one_inf]


@pytest.mark.parametrize("N", [4, 8, 16])
def test_failures_are_contained(N):
    P = 256
    R = np.array(_items(N))
    clean, st_clean = _block_dev(N, P, 0.0, R)
    assert np.all(st_clean == 0)
    for pos, item in zip(BAD_AT, _bad_items(N, R[2])):
        R[pos] = item
    spec, st = _block_dev(N, P, 0.0, R)
    want = np.zeros(N_BLOCK, np.int32); want[list(BAD_AT)] = 1
    assert np.array_equal(st, want), st
    nan_rows = np.isnan(spec).all(axis=1)
    assert np.array_equal(nan_rows, want == 1) and not np.isnan(spec[want == 0]).any()
    assert _same(spec[want == 0], clean[want == 0])
    # the host entry reports the same status
    blk = doa.capon_lin_array(ref.TABLE[ROW_OF_N[N]][5], N, P, 0.0)
    h_spec, h_st = np.empty((N_BLOCK, P), np.float32), np.empty(N_BLOCK, np.int32)
    assert blk.work(N_BLOCK, [R], [h_spec, h_st]) == N_BLOCK
    assert np.array_equal(h_st, want) and _same(h_spec, spec)
    # with loading the all-ones item is regular
    spec5, st5 = _block_dev(N, P, 0.5, R)
    assert st5[BAD_AT[0]] == 0 and np.all(np.isfinite(spec5[BAD_AT[0]])) and spec5[BAD_AT[0]].max() == 0.0


# ---- 3: scale invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, 1e-2])
@pytest.mark.parametrize("N", [4, 8, 16])
def test_scale_invariance(N, delta):
    R = _items(N)
    base, st = _block_dev(N, 256, delta, R)
    assert np.all(st == 0)
    for factor in (2.0 ** 40, 2.0 ** -40):
        scaled = (R * np.float32(factor)).astype(np.complex64)          # exact in float
        got, st = _block_dev(N, 256, delta, scaled)
        assert np.all(st == 0) and _same(got, base), (N, delta, factor)


# ---- 4: batch boundaries ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wishart(N, n, seed):
    """n well-conditioned random covariance items X X^H / 4N (X: N x 4N complex normal), unread parts spoiled."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, N, 4 * N)) + 1j * rng.standard_normal((n, N, 4 * N))
    H = X @ X.conj().transpose(0, 2, 1) / (4 * N)                         # [item][row][col]
    R = _spoil_unread_parts(H.transpose(0, 2, 1).reshape(n, N * N).astype(np.complex64), N)
    R.setflags(write=False)
    return R


@pytest.mark.parametrize("N", [4, 16])
def test_batch_boundaries(N):
    P, sizes = 256, (1, 63, 64, 65, 4097)
    R = _wishart(N, max(sizes), 40 + N)
    full, st = _block_dev(N, P, 1e-3, R, d=0.5)
    assert np.all(st == 0)
    blk = doa.capon_lin_array(0.5, N, P, 1e-3)
    for n in sizes[:-1]:
        got, st = _block_dev(N, P, 1e-3, R[:n], d=0.5)
        assert np.all(st == 0) and _same(got, full[:n]), (N, n)
        h = np.full((n, P), -7.0, np.float32)
        assert blk.work(n, [R[:n]], [h]) == n
        assert _same(h, full[:n]), (N, n, "host")
    h = np.full((max(sizes), P), -7.0, np.float32)
    assert blk.work(max(sizes), [R], [h]) == max(sizes) and _same(h, full)
    untouched = np.full((2, P), -7.0, np.float32)
    assert blk.work(0, [R], [untouched]) == 0 and np.all(untouched == -7.0)
    assert blk.work_dev(0, 0, 0, None, torch.cuda.current_stream()) == 0


# ---- 5-8: the pipeline ----------------------------------------------------------------------------------------------------
NP_, DELTA = 15, 1e-3               # snapshots per pipeline case (3 batches of 5), the loading of the pipeline tests
# (table row, P, peaks)
PIPE_CASES = {"n4": (0, 1024, 2), "n8": (2, 256, 3), "n16": (3, 4096, 3)}


def _case(name):
    row, P, M = PIPE_CASES[name]
    N, thetas, snr_db, K, delta, d = ref.TABLE[row]
    return N, K, d, P, M, thetas, snr_db


@functools.lru_cache(maxsize=None)
def _host_streams(name):
    N, K, d, P, M, thetas, snr_db = _case(name)
    return ref.streams(N, thetas, snr_db, K, d, NP_)


@functools.lru_cache(maxsize=None)
def _dev_streams(name):
    return tuple(doa.sim.stream_slab_torch([_dev(a) for a in _host_streams(name)]))


class _Out:
    def __init__(self, N, M, P, n, spec=True):
        self.cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
        self.spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda") if spec else None
        self.mx = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
        self.am = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in vars(self).items()}


def _pipe(name, capon=True, cls=doa.music_pipeline):
    N, K, d, P, M, thetas, snr_db = _case(name)
    p = cls(N, K, 0, 0, d, M, P, max_batch=NP_)
    if capon:
        p.set_estimator("capon", DELTA)
    return p


def _work_dev(pipe, name, spec=True, ptrs=None):
    N, K, d, P, M, thetas, snr_db = _case(name)
    o = _Out(N, M, P, NP_, spec)
    ptrs = [t.data_ptr() for t in _dev_streams(name)] if ptrs is None else ptrs
    assert pipe.work_dev(NP_, ptrs, o.cov.data_ptr(), o.spec.data_ptr() if spec else 0, o.mx.data_ptr(), o.am.data_ptr(),
                         torch.cuda.current_stream()) == NP_
    return o.host()


@functools.lru_cache(maxsize=None)
def _capon_run(name):
    return _work_dev(_pipe(name), name)


@pytest.mark.parametrize("name", sorted(PIPE_CASES))
def test_pipeline_equals_the_chain_of_blocks(name):
    N, K, d, P, M, thetas, snr_db = _case(name)
    got = _capon_run(name)
    st = torch.cuda.current_stream()
    cov = torch.empty((NP_, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((NP_, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((NP_, M), dtype=torch.float32, device="cuda")
    am = torch.empty((NP_, M), dtype=torch.float32, device="cuda")
    doa.autocorrelate(N, K, 0, 0).work_dev(NP_, [t.data_ptr() for t in _dev_streams(name)], cov.data_ptr(), st)
    doa.capon_lin_array(d, N, P, DELTA).work_dev(NP_, cov.data_ptr(), spec.data_ptr(), None, st)
    doa.find_local_max(M, P, 0.0, 180.0).work_dev(NP_, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    torch.cuda.synchronize()
    for key, want in (("cov", cov), ("spec", spec), ("mx", mx), ("am", am)):
        assert _same(got[key], want.cpu().numpy()), (name, key)
    err = ref.angle_error(got["am"], thetas)
    print(name, "Capon pipeline: max angle error %.3f deg" % err)
    assert err <= 0.6 + 180.0 / P


@pytest.mark.parametrize("name", sorted(PIPE_CASES))
def test_pipeline_other_entries(name):
    N, K, d, P, M, thetas, snr_db = _case(name)
    want = _capon_run(name)
    pipe = _pipe(name)
    # angles only
    lean = _work_dev(pipe, name, spec=False)
    assert _same(lean["mx"], want["mx"]) and _same(lean["am"], want["am"]) and _same(lean["cov"], want["cov"])
    # host entry
    x = _host_streams(name)
    h = {"mx": np.empty((NP_, M), np.float32), "am": np.empty((NP_, M), np.float32),
         "cov": np.empty((NP_, N * N), np.complex64), "spec": np.empty((NP_, P), np.float32)}
    assert pipe.work(NP_, [x[k] for k in range(N)], h["mx"], h["am"], cov_out=h["cov"], spectrum_out=h["spec"]) == NP_
    for key in ("cov", "spec", "mx", "am"):
        assert _same(h[key], want[key]), (name, "host", key)
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
            assert _same(got[key], want[key]), (name, "batches", lanes, key)


def test_pipeline_sc16_equals_fc32():
    name = "n4"
    q = doa.sim.to_sc16(0.25 * _host_streams(name))
    x = doa.sim.from_sc16(q)
    keep16 = [_dev(t) for t in q]
    a = _work_dev(_pipe(name, cls=doa.music_pipeline_sc16), name, ptrs=[t.data_ptr() for t in keep16])
    keep = [_dev(t) for t in x]
    b = _work_dev(_pipe(name), name, ptrs=[t.data_ptr() for t in keep])
    for key in ("cov", "spec", "mx", "am"):
        assert _same(a[key], b[key]), key
    assert np.all(np.isfinite(a["spec"]))


def test_pipeline_zero_snapshot_is_contained():
    name = "n4"
    N, K, d, P, M, thetas, snr_db = _case(name)
    want = _capon_run(name)
    x = np.array(_host_streams(name))
    x[:, 7 * K:8 * K] = 0
    keep = [_dev(t) for t in x]
    pipe = _pipe(name)
    got = _work_dev(pipe, name, ptrs=[t.data_ptr() for t in keep])
    others = [i for i in range(NP_) if i != 7]
    assert np.isnan(got["spec"][7]).all() and np.isnan(got["mx"][7]).all() and np.isnan(got["am"][7]).all()
    assert np.all(got["cov"][7] == 0)
    for key in ("cov", "spec", "mx", "am"):
        assert _same(got[key][others], want[key][others]), key
    lean = _work_dev(pipe, name, spec=False, ptrs=[t.data_ptr() for t in keep])
    assert _same(lean["mx"], got["mx"]) and _same(lean["am"], got["am"])


def test_pipeline_limits():
    name = "n4"
    N, K, d, P, M, thetas, snr_db = _case(name)
    pipe = _pipe(name)
    o = _Out(N, M, P, NP_)
    cnt = torch.zeros((NP_,), dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in _dev_streams(name)]
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_auto(NP_, ptrs, o.mx.data_ptr(), o.am.data_ptr(), cnt.data_ptr())
    assert ei.value.status == -4
    pipe.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        _work_dev(pipe, name)
    assert ei.value.status == -4
    pipe.set_internal_precision(64)
    got = _work_dev(pipe, name)
    assert _same(got["spec"], _capon_run(name)["spec"])
    for bad in (("capon", -1.0), ("capon", float("nan"))):
        with pytest.raises(doa.DoaError) as ei:
            pipe.set_estimator(*bad)
        assert ei.value.status == -1
    with pytest.raises(ValueError):
        pipe.set_estimator("esprit")
    doa.set_internal_precision(32)
    try:
        blk = doa.capon_lin_array(d, N, P, 0.0)
    finally:
        doa.set_internal_precision(64)
    with pytest.raises(doa.DoaError) as ei:
        blk.work(1, [_items(4)[:1]], [np.empty((1, P), np.float32)])
    assert ei.value.status == -4


@pytest.mark.parametrize("name", sorted(PIPE_CASES))
def test_pipeline_switching_back_restores_music(name):
    fresh = _work_dev(_pipe(name, capon=False), name)
    pipe = _pipe(name)
    capon = _work_dev(pipe, name)
    assert not _same(capon["spec"], fresh["spec"])
    pipe.set_estimator("music")
    back = _work_dev(pipe, name)
    for key in ("cov", "spec", "mx", "am"):
        assert _same(back[key], fresh[key]), (name, key)


# ---- 9: with spatial smoothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "A"])
def test_capon_with_spatial_smoothing(name):
    """Coherent sources (tests/spatial_smooth_ref.py): with smoothing on, the Capon pipeline's peak locations are those of the
    reference on the smoothed items to within one grid step.  Unsmoothed, the same handle misses a direction by more than
    5 degrees on at least one snapshot -- asserted for scenario B only: on the CPU the unsmoothed REFERENCE's largest angle
    error over the 24 snapshots is 11.99 degrees in B but 1.56 degrees in A (eight antennas at 20 dB still separate the two
    coherent paths well enough for Capon), so A has no such gap to assert; its figures are printed."""
    N, S, fb, th, rho = ssref.SCENARIOS[name]
    M, P, K, NS, D = len(th), ssref.P, ssref.K, ssref.N_SNAP, ssref.D
    streams = doa.sim.stream_slab_torch([_dev(a) for a in ssref.streams(name)])
    ptrs = [t.data_ptr() for t in streams]
    pipe = doa.music_pipeline(N, K, 0, 0, D, M, P, max_batch=NS)
    pipe.set_estimator("capon", 0.0)

    def run():
        o = _Out(N, M, P, NS)
        assert pipe.work_dev(NS, ptrs, o.cov.data_ptr(), o.spec.data_ptr(), o.mx.data_ptr(), o.am.data_ptr(),
                             torch.cuda.current_stream()) == NS
        return o.host()

    raw = run()
    pipe.set_spatial_smoothing(S, fb)
    got = run()
    s_ref, _, _, st = ref.capon(ssref.smoothed(name), D, S, P, 0.0)
    assert np.all(st == 0)
    _, loc = oracle.find_local_max(s_ref, M, P, 0.0, 180.0)
    step = 180.0 / P + 1e-4
    e = np.abs(np.sort(got["am"], axis=1) - np.sort(loc, axis=1)).max()
    s_raw, _, _, st_raw = ref.capon(ssref.covariance(name), D, N, P, 0.0)
    _, loc_raw = oracle.find_local_max(s_raw, M, P, 0.0, 180.0)
    per_item = np.abs(np.sort(raw["am"].astype(np.float64), axis=1) - np.sort(np.asarray(th))[None, :]).max(axis=1)
    print(name, "smoothed Capon: peak locations within %.3g deg of the reference's; angle error smoothed %.3f, unsmoothed "
          "device %.3f, unsmoothed reference %.3f deg" % (e, ssref.angle_error(got["am"], th), per_item.max(),
                                                           ssref.angle_error(loc_raw, th)))
    assert e <= step
    if name == "B":
        assert ssref.angle_error(loc_raw, th) > 5.0 and per_item.max() > 5.0
