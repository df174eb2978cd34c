"""The used-bin rule of a snapshot of bins (csrc/bin_plan.hpp: bin_weight_used), once for both kernels that apply it: a bin
counts when 0 < w < +inf, and the item of any other bin is not read.

N = 4, F = 16, all 16 bins, 7 snapshots.  In snapshot k bin 5 has the k-th weight of WEIGHTS, every other weight is 1, and
bin 5's item has a NaN in its upper triangle.  wideband_music (null_mean, P = 64) and focus_covariance (identity table) must
give the status words of their numpy statements: 0 where the weight is not usable (the NaN is never read), 3 where it is.  The
rows and items of status 0 are compared at the parity bounds of tests/test_gpu_wideband_music.py and
tests/test_gpu_focus_covariance.py, through those modules' own helpers.

The call-size limit, the other rule both work_dev entries share, is compared with the text recorded in
tests/golden/bin_plan_refusals.json (tests/test_cpu_bin_plan_refusals.py)."""
import functools

import numpy as np
import pytest

import doa
import focus_ref as fr
import test_cpu_bin_plan_refusals as refusals
import test_gpu_focus_covariance as tf
import test_gpu_wideband_music as tw
import wideband_ref as wb

gpu = pytest.mark.gpu                   # the references' own test needs no device

N, M, F, NB, P, SNAPSHOTS, BIN = 4, 2, 16, 16, 64, 7, 5
FLT_MIN, FLT_MAX = np.float32(1.17549435e-38), np.float32(3.4028235e38)
WEIGHTS = np.array([0.0, -0.0, -1.0, np.inf, np.nan, FLT_MIN, FLT_MAX], np.float32)
STATUS = [0, 0, 0, 0, 0, 3, 3]


@functools.lru_cache(maxsize=None)
def _case():
    """(items [7, 16, 16] complex64, weights [7, 16] float32), read-only."""
    items = wb.parity_items((N, M, F, 0, NB, P, SNAPSHOTS)).copy()
    items[:, BIN, 0 + 1 * N] = np.nan                           # element (0, 1): the upper triangle
    w = np.ones((SNAPSHOTS, NB), np.float32)
    w[:, BIN] = WEIGHTS
    items.setflags(write=False)
    w.setflags(write=False)
    return items, w


@functools.lru_cache(maxsize=None)
def _references():
    items, w = _case()
    eye = np.broadcast_to(np.eye(N, dtype=np.complex128), (NB, N, N))
    return wb.wideband_music(items, wb.D, M, N, P, F, 0, NB, wb.RHO, "null_mean", weights=w), fr.focus_covariance(items, eye, w)


def test_the_references_state_the_rule():
    """On the CPU first: both numpy statements give 0 0 0 0 0 3 3."""
    (_, _, st_wb, _), (_, st_fc) = _references()
    assert FLT_MIN == np.finfo(np.float32).tiny and FLT_MAX == np.finfo(np.float32).max
    assert st_wb.tolist() == STATUS and st_fc.tolist() == STATUS


@gpu
def test_wideband_music_uses_a_bin_by_the_rule():
    items, w = _case()
    (dB_ref, q_ref, st_ref, Qb), _ = _references()
    ok = st_ref == 0
    spec, q, st = tw._run(doa.wideband_music(wb.D, M, N, P, F, 0, NB, wb.RHO, "null_mean"), items, w)
    print("wideband_music status", st.tolist())
    assert st.tolist() == STATUS
    assert np.isnan(spec[~ok]).all() and np.isnan(q[~ok]).all()
    assert np.isnan(Qb[ok][:, BIN]).all()                      # the references skipped bin 5 there
    Qu = np.delete(Qb[ok], BIN, axis=1)                         # the used bins
    cond = (Qu.min(axis=2) / Qu.max(axis=2)).min()
    assert cond >= 1e-6, cond                                   # the inputs the bounds are stated for
    frac_q = (np.abs(q[ok] - q_ref[ok]) / tw._q_bound("null_mean", q_ref[ok], Qb[ok], np.ones((ok.sum(), NB)))).max()
    frac_db = (np.abs(spec[ok] - dB_ref[ok]) / (2e-5 + 2e-6 * np.abs(dB_ref[ok]))).max()     # the dB bound of tw's docstring
    print(f"wideband_music: q at {frac_q:.3f} of its bound, dB at {frac_db:.3f} of its bound")
    assert frac_q <= 1.0 and frac_db <= 1.0
    assert np.all(spec[ok].max(axis=1) == 0.0) and np.array_equal(spec[ok].argmax(axis=1), dB_ref[ok].argmax(axis=1))


@gpu
def test_focus_covariance_uses_a_bin_by_the_rule():
    items, w = _case()
    _, (ref, st_ref) = _references()
    ok = st_ref == 0
    eye = np.broadcast_to(np.eye(N, dtype=np.complex128), (NB, N, N)).copy()
    got, st = tf._run(doa.focus_covariance(N, NB, eye), items, w)
    print("focus_covariance status", st.tolist())
    assert st.tolist() == STATUS
    assert np.isnan(got[~ok].real).all() and np.isnan(got[~ok].imag).all()
    # the bound is stated with the weights of the used bins: bin 5 is none of them in the rows of status 0
    used_w, used_items = np.array(w[ok], np.float64), items[ok].copy()
    used_w[:, BIN], used_items[:, BIN] = 0.0, 0.0
    frac = tf._fraction(got[ok], ref[ok], used_items, N, used_w)
    print(f"focus_covariance: at {frac:.3f} of the bound")
    assert frac <= 1.0
    tf._assert_exactly_hermitian(got[ok], N)


@gpu
def test_the_call_size_limit_is_worded_as_recorded():
    fx = refusals.load_fixture()["call_size"]
    assert sorted(fx) == sorted(e for e, _ in refusals.CALL_SIZE)
    for entry, n in refusals.CALL_SIZE:
        assert list(refusals.call_size_case(entry, n)) == fx[entry], entry
