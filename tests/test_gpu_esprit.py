"""GPU tests of the ESPRIT estimator: the block doa.esprit_linear_array against the numpy statement (tests/esprit_ref.py) to
the project's Root-MUSIC parity bound, its failure containment, scale invariance, batch independence and counts entries,
and root_pipeline.set_estimator("esprit") against the chain of blocks, bit for bit.

The figures these tests print on an MI355X are kept in profiles/esprit_test_figures.txt: over all 29 cases and 67 items
each the device's angles are the reference's floats (worst |device - reference| 0 degrees, bound 1e-3), every status 0; on
the coherent scenario smoothed ESPRIT is within 0.013 degrees of smoothed Root-MUSIC (bound 0.5).

The comparisons print their figures as fractions of the bound before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import esprit_ref as ref
import spatial_smooth_ref as ssref
from doa import _lib

pytestmark = pytest.mark.gpu

BOUND_DEG = 1e-3                   # the project's Root-MUSIC parity bound (tests/test_gpu_root_music.py)
N_BLOCK = ref.N_ITEMS              # 67: a partial wave for every group width
WIDTH_CASES = [(4, 2), (8, 3), (16, 3)]      # one shape per group width (4, 8, 16 lanes per item), the last two iterating


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only arrays)


def _spoil_unread_parts(R, N):
    """Strict lower triangle NaN, imaginary part of the diagonal 7.0: neither may be read."""
    R = np.array(R).reshape(-1, N, N)                       # [item][col][row]
    for col in range(N):
        R[:, col, col + 1:] = np.nan + 1j * np.nan
        R[:, col, col] = R[:, col, col].real + 7.0j
    return R.reshape(-1, N * N)


@functools.lru_cache(maxsize=None)
def _items(N, M, snr):
    R = _spoil_unread_parts(ref.case_covariance(N, M, snr), N)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _reference(N, M, snr):
    return ref.esprit(_items(N, M, snr), ref.D, M, N)


def _block_dev(N, M, R, counts=None, d=ref.D):
    """(angles [n, M], status [n]) of work_dev / work_dev_counts."""
    n = R.shape[0]
    dR = _dev(R)
    ang = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    blk = doa.esprit_linear_array(d, M, N)
    s = torch.cuda.current_stream()
    if counts is None:
        assert blk.work_dev(n, dR.data_ptr(), ang.data_ptr(), st.data_ptr(), s) == n
    else:
        dc = _dev(np.asarray(counts, np.int32))
        assert blk.work_dev_counts(n, dR.data_ptr(), dc.data_ptr(), ang.data_ptr(), st.data_ptr(), s) == n
    torch.cuda.synchronize()
    return ang.cpu().numpy(), st.cpu().numpy()


# ---- 1: the block against the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,snr", ref.CASES)
def test_block_matches_the_definition(N, M, snr):
    R = _items(N, M, snr)
    a_ref, st_ref, gamma, gap = _reference(N, M, snr)
    # what the bound rests on, for every item: the definition itself is well posed
    assert not np.isnan(a_ref).any() and np.all(st_ref == 0)
    assert gamma.min() >= 1e-4 and gap.min() >= 1e-4, (gamma.min(), gap.min())
    ang, st = _block_dev(N, M, R)
    with np.errstate(invalid="ignore"):
        err = np.abs(ang.astype(np.float64) - a_ref.astype(np.float64))
    worst = float(np.nanmax(err)) if not np.isnan(err).all() else float("nan")
    print("N=%d M=%d %g dB: gamma >= %.3g, gap >= %.3g, worst |device - reference| %.3g deg = %.3g of the bound, status max %d"
          % (N, M, snr, gamma.min(), gap.min(), worst, worst / BOUND_DEG, st.max()))
    assert np.all(st == 0), st
    assert not np.isnan(ang).any()
    assert np.all(err <= BOUND_DEG)
    assert np.all(np.diff(ang, axis=1) >= 0)
    # the host entry: the same bits, with and without the status output
    blk = doa.esprit_linear_array(ref.D, M, N)
    h_ang, h_st = np.empty((N_BLOCK, M), np.float32), np.empty(N_BLOCK, np.int32)
    assert blk.work(N_BLOCK, [R], [h_ang, h_st]) == N_BLOCK
    assert _same(h_ang, ang) and np.array_equal(h_st, st)
    h2 = np.empty((N_BLOCK, M), np.float32)
    assert blk.work(N_BLOCK, [R], [h2]) == N_BLOCK and _same(h2, ang)


# ---- 2: failures are contained ----------------------------------------------------------------------------------------
BAD_AT = (1, 9, 30, 63)             # each shares its wave with good items, at every group width


@pytest.mark.parametrize("N,M", WIDTH_CASES)
def test_failures_are_contained(N, M):
    R = np.array(_items(N, M, 20.0))
    clean, st_clean = _block_dev(N, M, R)
    assert np.all(st_clean == 0)
    for pos, item in zip(BAD_AT, ref.failure_items(N, R[2])):      # singular (gamma = 0), zero, NaN, Inf
        R[pos] = item
    ang, st = _block_dev(N, M, R)
    want = np.zeros(N_BLOCK, np.int32); want[list(BAD_AT)] = 1
    assert np.array_equal(st, want), st
    nan_rows = np.isnan(ang).all(axis=1)
    assert np.array_equal(nan_rows, want == 1) and not np.isnan(ang[want == 0]).any()
    assert _same(ang[want == 0], clean[want == 0])
    _, st_ref = ref.esprit(R, ref.D, M, N)[:2]
    assert np.array_equal(st_ref, want)


# ---- 3: scale invariance, batch independence -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", WIDTH_CASES)
def test_power_of_two_scaling_gives_the_same_bits(N, M):
    R = _items(N, M, 20.0)
    base, st = _block_dev(N, M, R)
    for k in (10, -20):
        scaled = (R * np.float32(2.0 ** k)).astype(np.complex64)
        ang, st_k = _block_dev(N, M, scaled)
        assert _same(ang, base) and np.array_equal(st_k, st), k


@pytest.mark.parametrize("N,M", WIDTH_CASES)
def test_an_item_alone_gives_the_bits_it_has_in_the_batch(N, M):
    R = _items(N, M, 5.0)
    base, _ = _block_dev(N, M, R)
    for k in (0, 17, N_BLOCK - 1):
        one, st = _block_dev(N, M, R[k:k + 1])
        assert st[0] == 0 and _same(one[0], base[k]), k


# ---- 4: the counts entries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,W,snr", [(8, 3, 20.0), (4, 3, 5.0)])
def test_counts_entry_equals_the_fixed_blocks(N, W, snr):
    R = _items(N, W, snr)
    values = list(range(-1, N + 1))                        # -1, 0 .. N-1, N
    counts = np.array([values[i % len(values)] for i in range(N_BLOCK)], np.int32)
    ang, st = _block_dev(N, W, R, counts)
    top = min(W, N - 1)
    fixed = {m: _block_dev(N, m, R) for m in range(1, top + 1)}
    for i, m in enumerate(counts):
        if m < 0 or m > top:
            assert st[i] == 2 and np.isnan(ang[i]).all(), (i, m)
        elif m == 0:
            assert st[i] == 0 and np.isnan(ang[i]).all(), (i, m)
        else:
            a_m, st_m = fixed[m]
            assert st[i] == st_m[i] == 0 and _same(ang[i, :m], a_m[i]) and np.isnan(ang[i, m:]).all(), (i, m)
    assert st[counts == -1].tolist() == [2] * int((counts == -1).sum()) and np.all(st[counts == N] == 2)
    a_ref, st_ref = ref.esprit_counts(R, counts, ref.D, W, N)
    assert np.array_equal(st, st_ref) and np.array_equal(np.isnan(ang), np.isnan(a_ref))
    # the host entry
    blk = doa.esprit_linear_array(ref.D, W, N)
    h_ang, h_st = np.empty((N_BLOCK, W), np.float32), np.empty(N_BLOCK, np.int32)
    assert blk.work_counts(N_BLOCK, [R], counts, [h_ang, h_st]) == N_BLOCK
    assert _same(h_ang, ang) and np.array_equal(h_st, st)


# ---- 5: root_pipeline.set_estimator("esprit") ----------------------------------------------------------------------------
K_PIPE, N_BATCHES, N_PER = 256, 3, 23
N_PIPE = N_BATCHES * N_PER
# name: (N, M, thetas, subarray size (0 = no smoothing), forward-backward)
PIPE_SHAPES = {
    "n4": (4, 2, (30.0, 123.0), 0, 0),
    "n8": (8, 3, (60.0, 75.0, 120.0), 0, 0),
    "n8_smoothed": (8, 3, (60.0, 75.0, 120.0), 5, 1),
    "n16": (16, 3, (40.0, 75.0, 120.0), 0, 0),                     # 16 lanes per item
    "n16_smoothed": (16, 3, (40.0, 75.0, 120.0), 9, 1),            # subarrays of 9: 16 lanes per item after smoothing
}


@functools.lru_cache(maxsize=None)
def _pipe_streams(shape):
    N, M, th, S, fb = PIPE_SHAPES[shape]
    x = doa.sim.make_streams(N, N_PIPE * K_PIPE, list(th), ref.D, snr_db=20.0, seed=ref.SEED)
    x.setflags(write=False)
    return x


def _pipe(shape, estimator="esprit"):
    N, M, th, S, fb = PIPE_SHAPES[shape]
    pipe = doa.root_pipeline(N, K_PIPE, 0, 0, ref.D, M, max_batch=N_PIPE)
    if S:
        pipe.set_spatial_smoothing(S, fb)
    if estimator is not None:
        pipe.set_estimator(estimator)
    return pipe


def _pipe_work_dev(pipe, ptrs, N, M, n=N_PIPE):
    cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
    ang = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert pipe.work_dev(n, ptrs, cov.data_ptr(), ang.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return cov.cpu().numpy(), ang.cpu().numpy(), st.cpu().numpy()


def _hand_chain(shape, ptrs, method=None, n=N_PIPE):
    """autocorrelate -> [spatial_smooth ->] [source_count ->] esprit_linear_array[_counts]: block handles, one stream."""
    N, M, th, S, fb = PIPE_SHAPES[shape]
    s = torch.cuda.current_stream()
    cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
    assert doa.autocorrelate(N, K_PIPE, 0, 0).work_dev(n, ptrs, cov.data_ptr(), s) == n
    items, E = cov, N
    if S:
        items, E = torch.full((n, S * S), -7.0, dtype=torch.complex64, device="cuda"), S
        assert doa.spatial_smooth(N, S, bool(fb)).work_dev(n, cov.data_ptr(), items.data_ptr(), s) == n
    ang = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cnt = None
    blk = doa.esprit_linear_array(ref.D, M, E)
    if method is None:
        assert blk.work_dev(n, items.data_ptr(), ang.data_ptr(), st.data_ptr(), s) == n
    else:
        cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        eig = torch.full((n, E), -7.0, dtype=torch.float32, device="cuda")
        doa.source_count(E, K_PIPE, method, M).work_dev(n, items.data_ptr(), cnt.data_ptr(), eig.data_ptr(), s)
        assert blk.work_dev_counts(n, items.data_ptr(), cnt.data_ptr(), ang.data_ptr(), st.data_ptr(), s) == n
    torch.cuda.synchronize()
    if cnt is None:
        return cov.cpu().numpy(), ang.cpu().numpy(), st.cpu().numpy(), None
    return cov.cpu().numpy(), ang.cpu().numpy(), st.cpu().numpy(), (cnt.cpu().numpy(), eig.cpu().numpy())


@pytest.mark.parametrize("shape", sorted(PIPE_SHAPES))
def test_pipeline_equals_the_chain_of_blocks(shape):
    N, M, th, S, fb = PIPE_SHAPES[shape]
    x = _pipe_streams(shape)
    dev = doa.sim.stream_slab_torch([_dev(a) for a in x])
    ptrs = [t.data_ptr() for t in dev]
    want_cov, want_ang, want_st, _ = _hand_chain(shape, ptrs)
    assert np.all(want_st == 0) and not np.isnan(want_ang).any()
    assert np.abs(want_ang - np.array(th)[None, :]).max() <= 3.0
    fresh_root = _pipe_work_dev(_pipe(shape, None), ptrs, N, M)          # a Root-MUSIC handle that never changed mode

    pipe = _pipe(shape)
    cov, ang, st = _pipe_work_dev(pipe, ptrs, N, M)
    assert _same(cov, want_cov) and _same(ang, want_ang) and np.array_equal(st, want_st)
    assert _same(cov, fresh_root[0])                                    # K1 does not depend on the mode

    # work_dev_batches: three batches, one chain of launches each
    b_cov = [torch.full((N_PER, N * N), -7.0, dtype=torch.complex64, device="cuda") for _ in range(N_BATCHES)]
    b_ang = [torch.full((N_PER, M), -7.0, dtype=torch.float32, device="cuda") for _ in range(N_BATCHES)]
    b_st = [torch.full((N_PER,), -7, dtype=torch.int32, device="cuda") for _ in range(N_BATCHES)]
    b_ptrs = [[t.data_ptr() + b * N_PER * K_PIPE * 8 for t in dev] for b in range(N_BATCHES)]
    assert pipe.work_dev_batches(N_PER, b_ptrs, [t.data_ptr() for t in b_cov], [t.data_ptr() for t in b_ang],
                                 [t.data_ptr() for t in b_st], torch.cuda.current_stream()) == N_PIPE
    pipe.synchronize()
    torch.cuda.synchronize()
    assert _same(torch.cat(b_cov).cpu().numpy(), want_cov)
    assert _same(torch.cat(b_ang).cpu().numpy(), want_ang) and np.array_equal(torch.cat(b_st).cpu().numpy(), want_st)

    # the host entry
    h_ang, h_cov = np.empty((N_PIPE, M), np.float32), np.empty((N_PIPE, N * N), np.complex64)
    assert pipe.work(N_PIPE, [np.array(a) for a in x], h_ang, h_cov) == N_PIPE
    assert _same(h_ang, want_ang) and _same(h_cov, want_cov)

    # work_dev_auto (MDL): counts from the same eigen launch, the counted kernel
    a_cov, a_ang, a_st, (a_cnt, a_eig) = _hand_chain(shape, ptrs, "mdl")
    cnt = torch.full((N_PIPE,), -7, dtype=torch.int32, device="cuda")
    ang_t = torch.full((N_PIPE, M), -7.0, dtype=torch.float32, device="cuda")
    st_t = torch.full((N_PIPE,), -7, dtype=torch.int32, device="cuda")
    cov_t = torch.full((N_PIPE, N * N), -7.0, dtype=torch.complex64, device="cuda")
    E = S if S else N
    eig_t = torch.full((N_PIPE, E), -7.0, dtype=torch.float32, device="cuda")
    assert pipe.work_dev_auto(N_PIPE, ptrs, ang_t.data_ptr(), cnt.data_ptr(), "mdl", cov_t.data_ptr(), eig_t.data_ptr(),
                              st_t.data_ptr(), torch.cuda.current_stream()) == N_PIPE
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), a_cnt) and a_cnt.min() >= 0 and a_cnt.max() <= M
    assert _same(cov_t.cpu().numpy(), a_cov) and _same(ang_t.cpu().numpy(), a_ang) and np.array_equal(st_t.cpu().numpy(), a_st)
    eig = eig_t.cpu().numpy()
    assert np.all(np.isfinite(eig)) and np.all(np.diff(eig, axis=1) >= 0)
    if E > 4:
        assert _same(eig, a_eig)                                        # the same eigen launch as source_count's
    else:
        # E <= 4: the record comes from the 4-lane Jacobi form, source_count runs one lane per item; both round a double
        # that agrees to ~1e-15 of the largest eigenvalue to float, so they differ by at most one float ulp (2^-23 relative)
        rel = float((np.abs(eig - a_eig) / np.abs(a_eig)).max())
        print("%s: eigenvalues of the auto launch vs source_count: %.3g relative (bound 2^-23 = 1.2e-7), %s"
              % (shape, rel, "bit-identical" if _same(eig, a_eig) else "not bit-identical"))
        assert rel <= 2.0 ** -23

    # back to Root-MUSIC: the bits of a handle that never left it
    pipe.set_estimator("root_music")
    back = _pipe_work_dev(pipe, ptrs, N, M)
    for a, b in zip(back, fresh_root):
        assert _same(a, b)


def test_host_entry_reports_an_unsolvable_item():
    """An all-zero snapshot: status 1 on the device entry, DOA_ERR_NUMERIC from work, the other items valid."""
    shape = "n4"
    N, M, th, S, fb = PIPE_SHAPES[shape]
    x = np.array(_pipe_streams(shape))
    x[:, 5 * K_PIPE:6 * K_PIPE] = 0
    pipe = _pipe(shape)
    h_ang = np.full((N_PIPE, M), -7.0, np.float32)
    with pytest.raises(doa.DoaError) as ei:
        pipe.work(N_PIPE, list(x), h_ang)
    assert ei.value.status == -5 and "item 5" in str(ei.value)
    assert np.isnan(h_ang[5]).all() and not np.isnan(np.delete(h_ang, 5, axis=0)).any()


def test_smoothed_esprit_resolves_coherent_sources():
    """Scenario A of tests/spatial_smooth_ref.py (two fully coherent paths): smoothed ESPRIT finds both directions, each
    within 0.5 degrees of the smoothed Root-MUSIC chain's answer."""
    N, S, fb, th, rho = ssref.SCENARIOS["A"]
    M, n = len(th), ssref.N_SNAP
    dev = doa.sim.stream_slab_torch([_dev(a) for a in ssref.streams("A")])
    ptrs = [t.data_ptr() for t in dev]
    out = {}
    for est in ("root_music", "esprit"):
        pipe = doa.root_pipeline(N, ssref.K, 0, 0, ssref.D, M, max_batch=n)
        pipe.set_spatial_smoothing(S, fb)
        pipe.set_estimator(est)
        _, out[est], st = _pipe_work_dev(pipe, ptrs, N, M, n)
        assert not st.any()
    diff = float(np.abs(out["esprit"].astype(np.float64) - out["root_music"]).max())
    err = ssref.angle_error(out["esprit"], th)
    print("coherent scenario A: smoothed ESPRIT vs smoothed Root-MUSIC %.3f deg (bound 0.5), vs the truth %.3f deg" % (diff, err))
    assert not np.isnan(out["esprit"]).any()
    assert diff <= 0.5


# ---- 6: rejections ------------------------------------------------------------------------------------------------------------
def test_precision_32_is_unsupported():
    R = _items(4, 2, 20.0)
    dR = _dev(R)
    ang = torch.zeros((N_BLOCK, 2), dtype=torch.float32, device="cuda")
    doa.set_internal_precision(32)
    try:
        blk = doa.esprit_linear_array(ref.D, 2, 4)
    finally:
        doa.set_internal_precision(64)
    with pytest.raises(doa.DoaError) as ei:
        blk.work_dev(N_BLOCK, dR.data_ptr(), ang.data_ptr())
    assert ei.value.status == -4
    with pytest.raises(doa.DoaError) as ei:
        blk.work(N_BLOCK, [R], [np.empty((N_BLOCK, 2), np.float32)])
    assert ei.value.status == -4
    shape = "n4"
    dev = doa.sim.stream_slab_torch([_dev(a) for a in _pipe_streams(shape)])
    pipe = _pipe(shape)
    pipe.set_internal_precision(32)
    ang_p = torch.zeros((N_PIPE, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev(N_PIPE, [t.data_ptr() for t in dev], None, ang_p.data_ptr())
    assert ei.value.status == -4


def test_bad_estimator_leaves_the_handle_as_it_was():
    shape = "n4"
    N, M, th, S, fb = PIPE_SHAPES[shape]
    dev = doa.sim.stream_slab_torch([_dev(a) for a in _pipe_streams(shape)])
    ptrs = [t.data_ptr() for t in dev]
    pipe = _pipe(shape)
    before = _pipe_work_dev(pipe, ptrs, N, M)
    for bad in (-1, 2, 7):
        assert _lib.lib.doa_root_pipeline_set_estimator(pipe._h, bad) == -1
        assert "set_estimator" in _lib.last_error()
    with pytest.raises(ValueError):
        pipe.set_estimator("music")
    assert pipe.estimator == "esprit"
    after = _pipe_work_dev(pipe, ptrs, N, M)
    for a, b in zip(before, after):
        assert _same(a, b)
