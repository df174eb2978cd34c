"""GPU tests of MUSIC_lin_array with a source count per item (work_counts / work_dev_counts) on the shared covariance cases
(tests/source_count_cases.py).  Every item is compared with oracle.music_lin_array(R[i:i+1], d, M_i, N, P, "f64") under bounds
(d) and (e) of tests/test_gpu_music.py for noisy data, unchanged: the maximum is exactly 0 dB,
|dB - dB_f64| <= 2e-5 + 2e-6 |dB|, and the arg-max bin is equal."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import source_count_cases as cases
import source_count_ref as ref

pytestmark = pytest.mark.gpu

# name -> pspectrum_len (256 for N <= 4, 1000 for N = 5, 2048 for N = 12; and the full group and block forms, N = 8 and 16, at
# 1024 -- the lean scan on plain records -- and 4096 -- the long-spectrum scan)
SHAPES = {"n4_two_fb": 256, "n4_one": 256, "n3_two": 256, "n2_one_s0": 256, "n5_two_s0": 1000, "n5_two_s1": 1000,
          "n12_four_s0": 2048, "n8_three": 1024, "n16_three_fb": 4096}


@functools.lru_cache(maxsize=None)
def _oracle_row(name, i, M):
    N, d = cases.CASES[name][0], cases.CASES[name][2]
    s = oracle.music_lin_array(cases.covariance(name)[i:i + 1], d, M, N, SHAPES[name], "f64")[0]
    s.setflags(write=False)
    return s


def _check_rows(name, spec, counts, what):
    """bounds (d) and (e) per item; count 0: the row is all 0.0; an invalid count: NaN."""
    N = cases.CASES[name][0]
    worst = 0.0
    for i, M in enumerate(counts):
        if M == 0:
            assert np.all(spec[i] == 0.0), (name, what, i)
            continue
        if M < 0 or M >= N:
            assert np.all(np.isnan(spec[i])), (name, what, i, M)
            continue
        s64 = _oracle_row(name, i, int(M))
        assert spec[i].max() == 0.0, (name, what, i, M)
        fin = np.isfinite(s64)
        diff = np.abs(spec[i].astype(np.float64) - s64)[fin]
        bound = 2e-5 + 2e-6 * np.abs(s64[fin])
        worst = max(worst, float((diff / bound).max()))
        assert np.all(diff <= bound), (name, what, i, int(M), float(diff.max()), float((diff / bound).max()))
        assert int(np.argmax(spec[i])) == int(np.argmax(s64)), (name, what, i, int(M))
    print(name, what, "worst |dB - dB_f64| / bound = %.3g" % worst)


def _work(name, counts):
    N, d = cases.CASES[name][0], cases.CASES[name][2]
    R = cases.covariance(name)
    n = R.shape[0]
    blk = doa.MUSIC_lin_array(d, 1, N, SHAPES[name])
    spec = np.full((n, SHAPES[name]), -7.0, np.float32)
    assert blk.work_counts(n, [R], np.asarray(counts, np.int32), [spec]) == n
    assert blk.nout_items_total() == n
    return spec


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_counts_from_the_reference_estimator(name):
    counts = cases.reference(name, ref.MDL)[0]
    _check_rows(name, _work(name, counts), counts, "estimated")


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_forced_counts_cover_every_value_inside_one_wave(name):
    N, n = cases.CASES[name][0], cases.CASES[name][7]
    counts = np.arange(n, dtype=np.int32) % N                          # 0 .. N-1
    _check_rows(name, _work(name, counts), counts, "forced")


@pytest.mark.parametrize("name", ["n4_two_fb", "n3_two", "n5_two_s0", "n12_four_s0", "n8_three", "n16_three_fb"])
def test_invalid_counts_give_nan_rows_and_leave_neighbours_intact(name):
    N, n = cases.CASES[name][0], cases.CASES[name][7]
    good = np.arange(n, dtype=np.int32) % N
    counts = good.copy()
    bad = [1, 6, 12, 13, 15]
    counts[bad] = [-1, N, 99, -2 ** 31, 2 ** 31 - 1]
    a, b = _work(name, good), _work(name, counts)
    for i in bad:
        assert np.all(np.isnan(b[i])), (name, i)
    keep = np.ones(n, bool)
    keep[bad] = False
    assert np.array_equal(a[keep], b[keep])
    zero = np.flatnonzero(good == 0)
    assert len(zero) and np.all(a[zero] == 0.0)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_uniform_counts_agree_with_work(name):
    """Not bit-equal: work may take the subspace-iteration route, the counted entry always runs the Jacobi."""
    N, d, n = cases.CASES[name][0], cases.CASES[name][2], cases.CASES[name][7]
    M = len(cases.CASES[name][1])
    R = cases.covariance(name)
    blk = doa.MUSIC_lin_array(d, M, N, SHAPES[name])
    want = np.empty((n, SHAPES[name]), np.float32)
    blk.work(n, [R], [want])
    got = np.empty_like(want)
    blk.work_counts(n, [R], np.full(n, M, np.int32), [got])
    assert np.all(got.max(axis=1) == 0.0)
    diff = np.abs(got.astype(np.float64) - want)
    assert np.all(diff <= 2e-5 + 2e-6 * np.abs(want)), (name, float(diff.max()))
    assert np.array_equal(np.argmax(got, axis=1), np.argmax(want, axis=1))


def test_device_entry_equals_host_entry():
    name = "n5_two_s1"
    N, d, n = cases.CASES[name][0], cases.CASES[name][2], cases.CASES[name][7]
    counts = np.arange(n, dtype=np.int32) % N
    host = _work(name, counts)
    blk = doa.MUSIC_lin_array(d, 1, N, SHAPES[name])
    dR = torch.from_numpy(cases.covariance(name).copy()).cuda()
    dc = torch.from_numpy(counts).cuda()
    out = torch.full((n, SHAPES[name]), -7.0, dtype=torch.float32, device="cuda")
    assert blk.work_dev_counts(n, dR.data_ptr(), dc.data_ptr(), out.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host, equal_nan=True)


def test_rejections():
    name = "n4_one"
    R = cases.covariance(name)
    blk = doa.MUSIC_lin_array(0.5, 1, 4, 256)
    spec = np.empty((4, 256), np.float32)
    blk.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        blk.work_counts(4, [R], np.ones(4, np.int32), [spec])
    assert ei.value.status == -4                                        # DOA_ERR_UNSUPPORTED
    blk.set_internal_precision(64)
    assert blk.work_counts(4, [R], np.ones(4, np.int32), [spec]) == 4
    dR = torch.from_numpy(R.copy()).cuda()
    out = torch.empty((4, 256), dtype=torch.float32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:
        blk.work_dev_counts(4, dR.data_ptr(), None, out.data_ptr())
    assert ei.value.status == -1                                        # NULL counts
