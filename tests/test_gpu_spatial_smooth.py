"""GPU tests of spatial smoothing: the block doa.spatial_smooth against the numpy statement (tests/spatial_smooth_ref.py)
BIT FOR BIT -- the definition has no product feeding an addition, so a kernel that follows its order has no freedom --, and
music_pipeline.set_spatial_smoothing against the chain of blocks, on the coherent scenarios of the same file.

The pipeline tests print their figures (distance to the chain of blocks and to the fp64 oracle as fractions of the bounds,
angle errors) before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import spatial_smooth_ref as ref

pytestmark = pytest.mark.gpu

K, D, P, NS = ref.K, ref.D, ref.P, ref.N_SNAP
STEP = 180.0 / P + 1e-4            # one grid step of the arg-max axis


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _random_items(N, n, seed):
    """Seeded complex normal entries, NOT Hermitian, strict lower triangle NaN; read-only."""
    rng = np.random.default_rng(seed)
    R = (rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))).astype(np.complex64)     # [item][col][row]
    for col in range(N):
        R[:, col, col + 1:] = np.nan + 1j * np.nan
    R = R.reshape(n, N * N)
    R.setflags(write=False)
    return R


def _block_dev(N, S, fb, R):
    n = R.shape[0]
    dR = _dev(R)
    out = torch.full((n, S * S), -7.0, dtype=torch.complex64, device="cuda")
    blk = doa.spatial_smooth(N, S, fb)
    assert blk.work_dev(n, dR.data_ptr(), out.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1-5: the block --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 11, 16])
def test_block_equals_the_statement_bit_for_bit(N):
    R = _random_items(N, 67, N)
    for S in range(2, N + 1):
        for fb in (0, 1):
            got = _block_dev(N, S, fb, R)
            assert np.all(np.isfinite(got.view(np.float32))), (N, S, fb)        # the lower triangle is never read
            assert _same(got, ref.smooth(R, N, S, fb)), (N, S, fb)


@pytest.mark.parametrize("N,S", [(4, 3), (16, 12)])
def test_tile_and_grid_boundaries(N, S):
    """64 items of N = 4 (4 of N = 16) make one workgroup's tile; 4097 items leave the last tile partial."""
    sizes = (1, 63, 64, 65, 4097)
    R = _random_items(N, max(sizes), 100 + N)
    want = ref.smooth(R, N, S, 1)
    for n in sizes:
        assert _same(_block_dev(N, S, 1, R[:n]), want[:n]), (N, S, n)


def test_more_tiles_than_the_grid_holds():
    """70 001 items of N = 4 are 1094 tiles, past the grid cap of four workgroups per compute unit: the grid-stride rounds."""
    R = _random_items(4, 70001, 7)
    assert _same(_block_dev(4, 3, 1, R), ref.smooth(R, 4, 3, 1))


def test_eight_byte_path_equals_the_aligned_one():
    N, S, n = 3, 2, 67
    R = _random_items(N, n, 5)
    aligned = _block_dev(N, S, 1, R)
    buf_in = torch.zeros(n * N * N + 1, dtype=torch.complex64, device="cuda")
    buf_out = torch.full((n * S * S + 1,), -7.0, dtype=torch.complex64, device="cuda")
    assert buf_in.data_ptr() % 256 == 0 and buf_out.data_ptr() % 256 == 0
    buf_in[1:] = _dev(R).reshape(-1)
    blk = doa.spatial_smooth(N, S, 1)
    assert blk.work_dev(n, buf_in.data_ptr() + 8, buf_out.data_ptr() + 8, torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    got = buf_out.cpu().numpy()
    assert got[0] == np.complex64(-7.0)
    assert _same(got[1:].reshape(n, S * S), aligned) and _same(aligned, ref.smooth(R, N, S, 1))


@pytest.mark.parametrize("N,S,fb,row,col", [(8, 6, 1, 1, 3), (5, 3, 0, 2, 2), (4, 3, 1, 0, 2)])
def test_nan_isolation(N, S, fb, row, col):
    R = np.array(_random_items(N, 9, 11))
    clean = _block_dev(N, S, fb, R)
    R[4, row + col * N] = np.nan + 1j * np.nan                   # one upper-triangle entry of one item
    got = _block_dev(N, S, fb, R)
    want = ref.smooth(R, N, S, fb)
    nan_got = np.isnan(got.real) | np.isnan(got.imag)
    nan_want = np.isnan(want.real) | np.isnan(want.imag)
    assert np.array_equal(np.isnan(got.real), np.isnan(want.real)) and np.array_equal(np.isnan(got.imag), np.isnan(want.imag))
    assert nan_want[4].any() and not nan_want[[0, 1, 2, 3, 5, 6, 7, 8]].any()
    assert (not nan_want[4].all()) or S * S <= 4                 # (only the sums that touch the entry)
    keep = ~nan_got
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    others = [0, 1, 2, 3, 5, 6, 7, 8]
    assert _same(got[others], clean[others])


@pytest.mark.parametrize("N,S,fb", [(4, 3, 1), (8, 6, 0), (16, 12, 1)])
def test_host_entry_equals_device_entry(N, S, fb):
    R = _random_items(N, 67, 13)
    dev = _block_dev(N, S, fb, R)
    blk = doa.spatial_smooth(N, S, fb)
    out = np.full((67, S * S), -7.0, np.complex64)
    assert blk.work(67, [R], [out]) == 67
    assert _same(out, dev)
    untouched = np.full((2, S * S), -7.0, np.complex64)
    assert blk.work(0, [R], [untouched]) == 0 and np.all(untouched == -7.0)
    assert blk.work_dev(0, 0, 0, torch.cuda.current_stream()) == 0


# ---- 6-10: the pipeline ------------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, N, M, n, spec=True):
        self.cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
        self.spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda") if spec else None
        self.mx = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
        self.am = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in vars(self).items()}


@functools.lru_cache(maxsize=None)
def _dev_streams(name):
    x = ref.streams(name)
    return tuple(doa.sim.stream_slab_torch([_dev(a) for a in x]))


def _pipe(name, smoothed=True, max_batch=NS):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    p = doa.music_pipeline(N, K, 0, 0, D, len(th), P, max_batch=max_batch)
    if smoothed:
        p.set_spatial_smoothing(S, fb)
    return p


def _work_dev(pipe, name, spec=True):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    o = _Out(N, len(th), NS, spec)
    ptrs = [t.data_ptr() for t in _dev_streams(name)]
    assert pipe.work_dev(NS, ptrs, o.cov.data_ptr(), o.spec.data_ptr() if spec else 0, o.mx.data_ptr(), o.am.data_ptr(),
                         torch.cuda.current_stream()) == NS
    return o.host()


@functools.lru_cache(maxsize=None)
def _smoothed_run(name):
    """work_dev of a smoothed handle on the scenario, computed once."""
    return _work_dev(_pipe(name), name)


@functools.lru_cache(maxsize=None)
def _plain_run(name):
    return _work_dev(_pipe(name, smoothed=False), name)


@pytest.mark.parametrize("name", sorted(ref.SCENARIOS))
def test_pipeline_identities(name):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    want, plain = _smoothed_run(name), _plain_run(name)
    assert _same(want["cov"], plain["cov"])                         # K1 exactly as the unsmoothed handle runs it
    assert not _same(want["am"], plain["am"])
    pipe = _pipe(name)
    x = ref.streams(name)
    # host entry (the staged form: 24 items are scheduler-sized)
    h = {"mx": np.empty((NS, M), np.float32), "am": np.empty((NS, M), np.float32),
         "cov": np.empty((NS, N * N), np.complex64), "spec": np.empty((NS, P), np.float32)}
    assert pipe.work(NS, [x[k] for k in range(N)], h["mx"], h["am"], cov_out=h["cov"], spectrum_out=h["spec"]) == NS
    for key in ("cov", "spec", "mx", "am"):
        assert _same(h[key], want[key]), (name, "host", key)
    # angles only
    lean = _work_dev(pipe, name, spec=False)
    assert _same(lean["mx"], want["mx"]) and _same(lean["am"], want["am"]) and _same(lean["cov"], want["cov"])
    # three batches of eight, on the caller's stream alone and over four lanes
    nb, n = 3, NS // 3
    streams = _dev_streams(name)
    ins = [[t.data_ptr() + b * n * K * 8 for t in streams] for b in range(nb)]
    for lanes in (1, 4):
        pipe.set_lanes(lanes)
        o = _Out(N, M, NS)
        rows = lambda t, per: [t.data_ptr() + b * n * per * t.element_size() for b in range(nb)]
        assert pipe.work_dev_batches(n, ins, rows(o.cov, N * N), rows(o.spec, P), rows(o.mx, M), rows(o.am, M),
                                     torch.cuda.current_stream()) == NS
        got = o.host()
        for key in ("cov", "spec", "mx", "am"):
            assert _same(got[key], want[key]), (name, "batches", lanes, key)
    # switched off again: a fresh unsmoothed handle's outputs
    pipe.set_spatial_smoothing(0, 0)
    off = _work_dev(pipe, name)
    for key in ("cov", "spec", "mx", "am"):
        assert _same(off[key], plain[key]), (name, "off", key)


def test_pipeline_host_entry_chunked_form():
    """Enough snapshots for several 32 MiB chunks on both copy lanes: each chunk's smoothed items live at its own offset."""
    N, S, fb, th, rho = ref.SCENARIOS["B"]
    M = len(th)
    n = 2 * ((32 << 20) // (K * N * 8)) + 37
    x = ref.coherent_streams(N, th, rho, n * K)
    pipe = doa.music_pipeline(N, K, 0, 0, D, M, P, max_batch=n)
    pipe.set_spatial_smoothing(S, fb)
    h_mx, h_am = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
    assert pipe.work(n, [x[k] for k in range(N)], h_mx, h_am) == n
    streams = [_dev(x[k]) for k in range(N)]
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    pipe.work_dev(n, [s.data_ptr() for s in streams], 0, 0, mx.data_ptr(), am.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert _same(h_mx, mx.cpu().numpy()) and _same(h_am, am.cpu().numpy())
    assert ref.angle_error(h_am, th) <= 1.0


@pytest.mark.parametrize("name", sorted(ref.SCENARIOS))
def test_pipeline_equals_the_chain_of_blocks(name):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    got = _smoothed_run(name)
    st = torch.cuda.current_stream()
    dR = _dev(got["cov"])
    dRs = torch.empty((NS, S * S), dtype=torch.complex64, device="cuda")
    spec = torch.empty((NS, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((NS, M), dtype=torch.float32, device="cuda")
    am = torch.empty((NS, M), dtype=torch.float32, device="cuda")
    doa.spatial_smooth(N, S, fb).work_dev(NS, dR.data_ptr(), dRs.data_ptr(), st)
    doa.MUSIC_lin_array(D, M, S, P).work_dev(NS, dRs.data_ptr(), spec.data_ptr(), st)
    doa.find_local_max(M, P, 0.0, 180.0).work_dev(NS, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    torch.cuda.synchronize()
    Rs, spec, mx, am = dRs.cpu().numpy(), spec.cpu().numpy(), mx.cpu().numpy(), am.cpu().numpy()
    assert _same(Rs, ref.smooth(got["cov"], N, S, fb))
    e_spec = np.abs(got["spec"] - spec) / (2e-6 + 5e-7 * np.abs(spec))
    e_mx = np.abs(got["mx"] - mx) / (2e-6 + 5e-7 * np.abs(mx))
    e_am = np.abs(got["am"] - am).max()
    s64 = oracle.music_lin_array(Rs, D, M, S, P, "f64")
    e_64 = np.abs(got["spec"] - s64) / (2e-5 + 2e-6 * np.abs(s64))
    print(name, "vs chain: spectrum %.3g, maxima %.3g of the bound (max |diff| %.3g dB), arg-max diff %.3g deg; vs fp64 oracle "
          "%.3g of the bound" % (e_spec.max(), e_mx.max(), np.abs(got["spec"] - spec).max(), e_am, e_64.max()))
    assert e_spec.max() <= 1.0 and e_mx.max() <= 1.0
    assert e_am <= STEP
    assert e_64.max() <= 1.0


def _auto(pipe, name, method, S_eig):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    o = _Out(N, M, NS)
    cnt = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
    eig = torch.full((NS, S_eig), -7.0, dtype=torch.float32, device="cuda")
    ptrs = [t.data_ptr() for t in _dev_streams(name)]
    assert pipe.work_dev_auto(NS, ptrs, o.mx.data_ptr(), o.am.data_ptr(), cnt.data_ptr(), method, o.cov.data_ptr(),
                              o.spec.data_ptr(), eig.data_ptr(), torch.cuda.current_stream()) == NS
    got = o.host()
    got["cnt"], got["eig"] = cnt.cpu().numpy(), eig.cpu().numpy()
    return got


@pytest.mark.parametrize("method", ["mdl", "aic"])
@pytest.mark.parametrize("name", ref.TABLE)
def test_auto_on_a_smoothed_handle_equals_the_chain(name, method):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    got = _auto(_pipe(name), name, method, S)
    assert _same(got["cov"], _plain_run(name)["cov"])
    st = torch.cuda.current_stream()
    dR = _dev(got["cov"])
    dRs = torch.empty((NS, S * S), dtype=torch.complex64, device="cuda")
    cnt = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
    eig = torch.full((NS, S), -7.0, dtype=torch.float32, device="cuda")
    spec = torch.full((NS, P), -7.0, dtype=torch.float32, device="cuda")
    mx = torch.full((NS, M), -7.0, dtype=torch.float32, device="cuda")
    am = torch.full((NS, M), -7.0, dtype=torch.float32, device="cuda")
    doa.spatial_smooth(N, S, fb).work_dev(NS, dR.data_ptr(), dRs.data_ptr(), st)
    doa.source_count(S, K, method, M).work_dev(NS, dRs.data_ptr(), cnt.data_ptr(), eig.data_ptr(), st)
    doa.MUSIC_lin_array(D, 1, S, P).work_dev_counts(NS, dRs.data_ptr(), cnt.data_ptr(), spec.data_ptr(), st)
    doa.find_local_max(M, P, 0.0, 180.0).work_dev_counts(NS, spec.data_ptr(), cnt.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    torch.cuda.synchronize()
    for key, want in (("cnt", cnt), ("eig", eig), ("spec", spec), ("mx", mx), ("am", am)):
        assert _same(got[key], want.cpu().numpy()), (name, method, key)


@pytest.mark.parametrize("name", ref.TABLE)
def test_end_to_end_coherent_sources(name):
    """The reason for the feature: with smoothing the pipeline finds the coherent sources and their number; without, neither."""
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    got = _smoothed_run(name)
    err = ref.angle_error(got["am"], th)
    auto = _auto(_pipe(name), name, "mdl", S)
    raw = _auto(_pipe(name, smoothed=False), name, "mdl", N)
    print(name, "smoothed pipeline: max angle error %.3f deg; MDL counts smoothed %s, unsmoothed %s"
          % (err, np.unique(auto["cnt"]), np.unique(raw["cnt"])))
    assert err <= 1.0
    assert np.all(auto["cnt"] == M), auto["cnt"]
    assert ref.angle_error(auto["am"], th) <= 1.0
    assert np.all(raw["cnt"] == 1), raw["cnt"]
    assert ref.angle_error(_plain_run(name)["am"], th) > 10.0       # the fixed-count handle misses a direction, too
    if name in ("A", "B"):
        x = ref.streams(name)
        R = np.empty((NS, N * N), np.complex64)
        doa.autocorrelate(N, K, 0, 0).general_work(NS, [x[k] for k in range(N)], [R])
        Rs = np.empty((NS, S * S), np.complex64)
        doa.spatial_smooth(N, S, fb).work(NS, [R], [Rs])
        ang = np.empty((NS, 2), np.float32)
        doa.rootMUSIC_linear_array(0.5, 2, S).work(NS, [Rs], [ang])
        e_root = ref.angle_error(ang, th)
        print(name, "Root-MUSIC on smoothed items: max angle error %.3f deg" % e_root)
        assert e_root <= 1.0


def test_rejections_leave_the_handle_as_it_was():
    name = "A"
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    for smoothed in (False, True):
        pipe = _pipe(name, smoothed)
        want = _smoothed_run(name) if smoothed else _plain_run(name)
        for bad in ((1, 1), (N + 1, 1), (M, 1), (S, 2)):
            with pytest.raises(doa.DoaError) as ei:
                pipe.set_spatial_smoothing(*bad)
            assert ei.value.status == -1, bad
            got = _work_dev(pipe, name)
            for key in ("cov", "spec", "mx", "am"):
                assert _same(got[key], want[key]), (smoothed, bad, key)


@pytest.mark.parametrize("name", ["A", "B"])
def test_precision_32_smoothed_handle(name):
    """The smoothing arithmetic is the definition at either precision; eigen stage and scan in float stay within the
    precision-32 bounds of test_gpu_music.py: where the null spectrum is at least 1e-2 of its maximum (the dB row at most
    20 dB above its minimum) each of the two spectra is within 4e-4 / 2e-5 dB of the fp64 evaluation up to a common
    constant, so their difference spreads by at most 2 (4e-4 + 2e-5) dB; arg-maxima within one grid step.

    Which items.  The same file bounds the float null spectrum by |Q_32 - Q_f64| <= 4 max|Q_oracle32 - Q_f64| + 1e-6 max Q
    at every angle.  A forward-backward smoothed item is persymmetric, so with one noise vector (B: S = 3, M = 2) the
    zeros of Q lie ON the unit circle, and on the grid Q comes as low as 3.8e-9 of its maximum (B, item 14, fp64, bin
    626: below 2^-24): there the bound lets Q_32 be zero or negative, the reference's own float evaluation IS negative
    (-1.9e-8 of the maximum, a non-finite row), and the dB row and its peaks are not defined at precision 32.  The dB and
    arg-max comparisons therefore run on the items whose fp64 minimum of Q exceeds that bound, i.e. where the bound keeps
    Q_32 positive -- a rule from the fp64 and fp32 oracles alone (8 of B's 24 items and 20 of A's on the oracle's own
    covariances); every row, the others included, still has its maximum at exactly 0 dB."""
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    pipe = _pipe(name)
    pipe.set_internal_precision(32)
    got, want = _work_dev(pipe, name), _smoothed_run(name)
    assert _same(got["cov"], want["cov"])
    assert np.all(got["spec"].max(axis=1) == 0.0)
    Rs = ref.smooth(want["cov"], N, S, fb)
    _, q64, _ = oracle.music_lin_array(Rs, D, M, S, P, "f64", return_parts=True)
    _, q32, _ = oracle.music_lin_array(Rs, D, M, S, P, "f32", return_parts=True)
    bound = 4 * np.abs(q32 - q64).max(axis=1) + 1e-6 * q64.max(axis=1)
    items = np.flatnonzero(q64.min(axis=1) > bound)
    print(name, "items whose nulls precision 32 resolves:", items.size, "of", NS)
    assert items.size >= NS // 6                    # (not vacuous; 8 and 20 items on the CPU's covariances)
    spread = 0.0
    for i in items:
        assert np.all(np.isfinite(got["spec"][i])), (name, i)
        g2 = want["spec"][i] <= want["spec"][i].min() + 20.0
        dg = (got["spec"][i].astype(np.float64) - want["spec"][i])[g2]
        spread = max(spread, float(dg.max() - dg.min()))
    e_am = np.abs(got["am"][items] - want["am"][items]).max()
    print(name, "precision 32 against 64: spread %.3g dB (bound %.3g), arg-max diff %.3g deg" % (spread, 2 * (4e-4 + 2e-5), e_am))
    assert spread <= 2 * (4e-4 + 2e-5)
    assert e_am <= STEP
