"""GPU tests of the IAA estimator: the block doa.iaa_lin_array against the numpy statement (tests/iaa_ref.py) to the
project's bounds for the double path (tests/test_gpu_music.py, tests/test_gpu_capon.py), on rank-one and coherent items,
its failure containment, scale invariance, batch boundaries and determinism, and the chain autocorrelate -> iaa_lin_array ->
find_local_max on the device.  tests/test_cpu_iaa.py asserts the condition numbers (at most 1e6) the bounds rest on.

Which case (N, P) of test 1 reaches which instantiation of the launcher (csrc/iaa.hip: one wave per item at every size; the
compile-time bound NT of the loops over the array size is what differs):
    iaa_wave_kernel<4>    N = 2, 3, 4    (2, 256) (3, 256) (4, 256) (4, 1024) (3, 37), tests 3, 4, 5, 6, 7
    iaa_wave_kernel<8>    N = 5 .. 8     (5, 256) (8, 256) (8, 1001), tests 2 (k1_n8), 3, 4
    iaa_wave_kernel<16>   N = 9 .. 16    (11, 256) (16, 256) (16, 4096), tests 2 (k1_n16, C), 3, 4, 5
(3, 37) is a grid shorter than a wave, (8, 1001) and (3, 37) end in a partial chunk of 64 directions.

The comparisons print their figures as fractions of the bounds before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import capon_ref
import iaa_ref as ref
import spatial_smooth_ref as ssref

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _block_dev(N, P, delta, iterations, R, d, blk=None):
    """(spectrum [n, P], power [n, P], status [n]) of work_dev."""
    n = R.shape[0]
    dR = _dev(R)
    spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    power = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    blk = doa.iaa_lin_array(d, N, P, delta, iterations) if blk is None else blk
    before = blk.nout_items_total()
    assert blk.work_dev(n, dR.data_ptr(), spec.data_ptr(), power.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    assert blk.nout_items_total() == before + n
    return spec.cpu().numpy(), power.cpu().numpy(), st.cpu().numpy()


def _db_excess(spec, s_ref):
    """|spec - s_ref| as a fraction of the dB bound 2e-5 + 2e-6 |s|, per cell; a -inf cell must be -inf on both sides."""
    inf = np.isneginf(s_ref)
    assert np.array_equal(np.isneginf(spec), inf)
    with np.errstate(invalid="ignore"):
        e = np.abs(spec - s_ref) / (2e-5 + 2e-6 * np.abs(s_ref))
    return np.where(inf, 0.0, e)


# ---- 1: the block against the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", ref.BLOCK_ITERATIONS)
@pytest.mark.parametrize("delta", ref.BLOCK_DELTAS)
@pytest.mark.parametrize("N,P", ref.BLOCK_CASES)
def test_block_matches_the_definition(N, P, delta, iterations):
    R, d = ref.block_items(N), ref.block_spacing(N)
    want = ref.block_reference(N, P, delta)
    assert np.all(want["status"] == 0)
    p_ref, lag_ref = want["p_all"][:, iterations - 1], want["lags_all"][:, iterations - 1]
    s_ref = np.array([ref.db_row(row) for row in p_ref])
    pow_ref = want["mu"][:, None] * p_ref
    spec, power, st = _block_dev(N, P, delta, iterations, R, d)
    p, lags = doa.iaa_lin_array(d, N, P, delta, iterations).debug(R)
    assert np.all(st == 0)
    e_p = float((np.abs(p - p_ref) / (3e-7 * np.abs(p_ref) + 2e-13 * p_ref.max(axis=1, keepdims=True))).max())
    e_l = float((np.abs(lags - lag_ref) / (3e-7 * np.abs(lag_ref[:, :1]))).max())
    e_s = float(_db_excess(spec, s_ref).max())
    ulp = np.spacing(np.abs(pow_ref).astype(np.float32)).astype(np.float64)
    e_w = float((np.abs(power - pow_ref) / (3e-7 * np.abs(pow_ref) + ulp)).max())
    print("N=%d P=%d delta=%g L=%d cond %.3g: p %.3g, lags %.3g, dB row %.3g, power port %.3g of the bounds"
          % (N, P, delta, iterations, want["cond"].max(), e_p, e_l, e_s, e_w))
    assert e_p <= 1.0 and e_l <= 1.0 and e_s <= 1.0 and e_w <= 1.0
    assert np.all(spec.max(axis=1) == 0.0)
    assert np.array_equal(np.argmax(spec, axis=1), np.argmax(s_ref, axis=1))


# ---- 2: rank-one and coherent items -----------------------------------------------------------------------------------
def _hard_set(name):
    if name == "C":
        N, th, _ = ref.coherent_truth("C")
        return ssref.covariance("C"), N, ssref.D, ssref.P, len(th)
    N, th, snr_db, d = ref.K1_SETS[name]
    return ref.k1_covariance(name), N, d, ref.K1_P, len(th)


@pytest.mark.parametrize("name", ["k1_n8", "k1_n16", "C"])
def test_rank_one_and_coherent_items(name):
    R, N, d, P, M = _hard_set(name)
    want = ref.iaa(R, d, N, P, 0.0, ref.DEFAULT_ITERATIONS)
    assert np.all(want["status"] == 0)
    spec, power, st = _block_dev(N, P, 0.0, ref.DEFAULT_ITERATIONS, R, d)
    assert np.all(st == 0) and np.all(spec.max(axis=1) == 0.0)
    s_ref = want["spectrum"]
    keep = s_ref >= -80.0
    left_out = 1.0 - keep.mean(axis=1)
    with np.errstate(invalid="ignore"):
        e = np.where(keep, np.abs(spec - s_ref) / (2e-5 + 2e-6 * np.abs(s_ref)), 0.0)
    _, loc = oracle.find_local_max(spec, M, P, 0.0, 180.0)
    _, loc_ref = ref.peaks(s_ref, M, P)
    e_loc = float(np.abs(np.sort(loc, axis=1) - np.sort(loc_ref, axis=1)).max())
    print("%s: cond %.3g, dB row %.3g of the bound on the cells at -80 dB or more (%.2f %% of a row left out at most), peaks "
          "within %.3g deg of the reference's" % (name, want["cond"].max(), e.max(), 100 * left_out.max(), e_loc))
    assert left_out.max() <= 0.005
    assert e.max() <= 1.0
    assert e_loc <= 180.0 / P + 1e-4


# ---- 3: failures are contained ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 8, 16])
def test_failures_are_contained(N):
    """At the largest iteration count, where the all-ones item (a noise-free rank-one covariance) has failed a pivot at every
    array size (tests/test_cpu_iaa.py: test_failure_items)."""
    P, L, d = 256, ref.MAX_ITERATIONS, ref.block_spacing(N)
    R = np.array(ref.block_items(N))
    clean, clean_pow, st_clean = _block_dev(N, P, 0.0, L, R, d)
    assert np.all(st_clean == 0)
    for pos, item in zip(ref.BAD_AT, ref.bad_items(N, R[2])):
        R[pos] = item
    spec, power, st = _block_dev(N, P, 0.0, L, R, d)
    want = np.zeros(ref.N_BLOCK, np.int32); want[list(ref.BAD_AT)] = 1
    assert np.array_equal(st, want), st
    for rows in (spec, power):
        assert np.array_equal(np.isnan(rows).all(axis=1), want == 1) and not np.isnan(rows[want == 0]).any()
    assert _same(spec[want == 0], clean[want == 0]) and _same(power[want == 0], clean_pow[want == 0])
    # the host entry agrees
    blk = doa.iaa_lin_array(d, N, P, 0.0, L)
    h_spec, h_pow, h_st = np.empty((ref.N_BLOCK, P), np.float32), np.empty((ref.N_BLOCK, P), np.float32), np.empty(ref.N_BLOCK, np.int32)
    assert blk.work(ref.N_BLOCK, [R], [h_spec, h_pow, h_st]) == ref.N_BLOCK
    assert np.array_equal(h_st, want) and _same(h_spec, spec) and _same(h_pow, power)
    p, lags = blk.debug(R)
    assert np.array_equal(np.isnan(p).all(axis=1), want == 1) and np.array_equal(np.isnan(lags).all(axis=1), want == 1)


# ---- 4: scale invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, 1e-2])
@pytest.mark.parametrize("N", [4, 8, 16])
def test_scale_invariance(N, delta):
    R, d = ref.block_items(N), ref.block_spacing(N)
    base, base_pow, st = _block_dev(N, 256, delta, ref.DEFAULT_ITERATIONS, R, d)
    assert np.all(st == 0)
    for factor in (2.0 ** 40, 2.0 ** -40):
        scaled = (R * np.float32(factor)).astype(np.complex64)          # exact in float
        got, got_pow, st = _block_dev(N, 256, delta, ref.DEFAULT_ITERATIONS, scaled, d)
        assert np.all(st == 0) and _same(got, base), (N, delta, factor)
        assert _same(got_pow, base_pow * np.float32(factor)), (N, delta, factor)


# ---- 5: batch boundaries and determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 16])
def test_batch_boundaries_and_determinism(N):
    P, L, sizes = 256, ref.DEFAULT_ITERATIONS, (1, 63, 64, 65, 4097)
    R = ref.wishart(N, max(sizes), 40 + N)
    blk = doa.iaa_lin_array(0.5, N, P, 1e-3, L)
    full, full_pow, st = _block_dev(N, P, 1e-3, L, R, 0.5, blk)
    assert np.all(st == 0)
    again, again_pow, st = _block_dev(N, P, 1e-3, L, R, 0.5, blk)
    assert np.all(st == 0) and _same(again, full) and _same(again_pow, full_pow)
    for n in sizes[:-1]:
        got, got_pow, st = _block_dev(N, P, 1e-3, L, R[:n], 0.5, blk)
        assert np.all(st == 0) and _same(got, full[:n]) and _same(got_pow, full_pow[:n]), (N, n)
        h, hp = np.full((n, P), -7.0, np.float32), np.full((n, P), -7.0, np.float32)
        assert blk.work(n, [R[:n]], [h, hp]) == n
        assert _same(h, full[:n]) and _same(hp, full_pow[:n]), (N, n, "host")
    h = np.full((max(sizes), P), -7.0, np.float32)
    assert blk.work(max(sizes), [R], [h]) == max(sizes) and _same(h, full)          # NULL power and status ports
    hs = np.full(5, -7, np.int32)
    assert blk.work(5, [R[:5]], [h[:5], None, hs]) == 5 and np.all(hs == 0) and _same(h[:5], full[:5])
    # n = 0 touches nothing
    untouched = np.full((2, P), -7.0, np.float32)
    total = blk.nout_items_total()
    assert blk.work(0, [R], [untouched, untouched]) == 0 and np.all(untouched == -7.0)
    assert blk.work_dev(0, 0, 0, None, None, torch.cuda.current_stream()) == 0
    assert blk.nout_items_total() == total
    # NULL optional ports on the device entry
    dR = _dev(R[:65])
    spec = torch.full((65, P), -7.0, dtype=torch.float32, device="cuda")
    assert blk.work_dev(65, dR.data_ptr(), spec.data_ptr(), None, None, torch.cuda.current_stream()) == 65
    torch.cuda.synchronize()
    assert _same(spec.cpu().numpy(), full[:65])


# ---- 6: the chain on the device -------------------------------------------------------------------------------------------
def test_chain_on_the_device():
    """autocorrelate -> iaa_lin_array -> find_local_max on the coherent scenario B at the full aperture (no smoothing), where
    capon_lin_array on the same covariance misses a direction by more than 5 degrees."""
    N, th, pw = ref.coherent_truth("B")
    M, P, K, NS, D = len(th), ssref.P, ssref.K, ssref.N_SNAP, ssref.D
    st = torch.cuda.current_stream()
    streams = doa.sim.stream_slab_torch([_dev(a) for a in ssref.streams("B")])
    cov = torch.empty((NS, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((NS, P), dtype=torch.float32, device="cuda")
    power = torch.empty((NS, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((NS, M), dtype=torch.float32, device="cuda")
    am = torch.empty((NS, M), dtype=torch.float32, device="cuda")
    peaks = doa.find_local_max(M, P, 0.0, 180.0)
    assert doa.autocorrelate(N, K, 0, 0).work_dev(NS, [t.data_ptr() for t in streams], cov.data_ptr(), st) == NS
    assert doa.iaa_lin_array(D, N, P).work_dev(NS, cov.data_ptr(), spec.data_ptr(), power.data_ptr(), None, st) == NS
    assert peaks.work_dev(NS, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st) == NS
    torch.cuda.synchronize()
    loc = am.cpu().numpy()
    err = ref.angle_error(loc, th)
    pk = ref.power_at_peaks(power.cpu().numpy(), loc, P)
    truth = np.asarray(pw)[np.argsort(th)]
    spec_c = torch.empty((NS, P), dtype=torch.float32, device="cuda")
    assert doa.capon_lin_array(D, N, P, 0.0).work_dev(NS, cov.data_ptr(), spec_c.data_ptr(), None, st) == NS
    assert peaks.work_dev(NS, spec_c.data_ptr(), mx.data_ptr(), am.data_ptr(), st) == NS
    torch.cuda.synchronize()
    err_c = ref.angle_error(am.cpu().numpy(), th)
    print("scenario B unsmoothed: IAA %.3f deg, Capon %.3f deg; powers at the peaks %s .. %s (true %s)"
          % (err, err_c, pk.min(axis=0), pk.max(axis=0), truth))
    assert err <= 0.6 + 180.0 / P
    assert err_c > 5.0
    assert np.abs(pk / truth[None, :] - 1.0).max() <= 0.10


# ---- 7: precision 32 is refused -------------------------------------------------------------------------------------------
def test_precision_32_is_refused():
    doa.set_internal_precision(32)
    try:
        blk = doa.iaa_lin_array(0.5, 4, 64)
    finally:
        doa.set_internal_precision(64)
    R = ref.block_items(4)[:1]
    with pytest.raises(doa.DoaError) as ei:
        blk.work(1, [R], [np.empty((1, 64), np.float32)])
    assert ei.value.status == -4
    dR = _dev(R)
    spec = torch.full((1, 64), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:
        blk.work_dev(1, dR.data_ptr(), spec.data_ptr(), None, None, torch.cuda.current_stream())
    assert ei.value.status == -4
    torch.cuda.synchronize()
    assert np.all(spec.cpu().numpy() == -7.0)
    with pytest.raises(doa.DoaError) as ei:
        blk.debug(R)
    assert ei.value.status == -4
