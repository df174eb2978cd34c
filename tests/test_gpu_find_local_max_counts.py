"""GPU tests of find_local_max with a peak count per item (work_counts / work_dev_counts): the first m_i slots of both ports
are BIT-EQUAL to oracle.find_local_max(row, m_i, ...) -- fill rule and the m_i == 1 global arg-max rule included --, the rest
of the num_max_vals-wide items is NaN, and m_i outside 0..num_max_vals gives all NaN.  Vector lengths cover every route of
the launch: the register kernel (CH = 1, 2, 4), blocked<16>, blocked<64>, the streaming kernel (unaligned short vectors) and
the serial kernel (L > 4096)."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle

pytestmark = pytest.mark.gpu

N_ITEMS = 37
LENGTHS = [20, 64, 256, 512, 1000, 1024, 2048, 4100]
WIDTHS = [1, 2, 5, 16]


@functools.lru_cache(maxsize=None)
def _rows(L):
    """[37, L] float32: the reference's two analytic QA signals (python/qa_find_local_max.py) cut to length, quantised noise
    (flats, plateau peaks, ties), smooth noise, and a few degenerate rows."""
    t = 2 * np.pi * np.linspace(0, 1, 4100)
    y1 = np.sin(3.14 * t) + 0.5 * np.cos(6.09 * t) + 0.1 * np.sin(10.11 * t + 1 / 6) + 0.1 * np.sin(15.3 * t + 1 / 3)
    y2 = np.sin(0.25 * 3.14 * t) + 5 * np.sin(6.09 * t) + 0.6 * np.cos(1.11 * t + 1 / 6) + 2 * np.sin(5.3 * t + 1 / 3)
    rng = np.random.default_rng(1000 + L)
    rows = [np.abs(y1)[:L], np.abs(y2)[:L], np.abs(y1)[-L:], np.abs(y2)[-L:], np.zeros(L), np.arange(L, dtype=np.float64)]
    while len(rows) < N_ITEMS:
        k = len(rows) % 3
        if k == 0:
            rows.append(np.round(rng.standard_normal(L) * 1.5))
        elif k == 1:
            rows.append(rng.integers(0, 3, size=L).astype(np.float64))
        else:
            rows.append(np.convolve(rng.standard_normal(L + 8), np.ones(9) / 9.0, mode="valid"))
    v = np.stack(rows).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _reference(L, m):
    """oracle.find_local_max of every row with num_max_vals = m (computed once per (L, m), read-only)."""
    r0, r1 = oracle.find_local_max(_rows(L), m, L, 0.0, 180.0)
    r0.setflags(write=False)
    r1.setflags(write=False)
    return r0, r1


def _expected(L, W, counts):
    e0 = np.full((N_ITEMS, W), np.nan, np.float32)
    e1 = np.full((N_ITEMS, W), np.nan, np.float32)
    for i, m in enumerate(counts):
        if 1 <= m <= W:
            r0, r1 = _reference(L, int(m))
            e0[i, :m] = r0[i]
            e1[i, :m] = r1[i]
    return e0, e1


def _same(a, b):
    return np.array_equal(a.view(np.uint32) & 0x7FC00000 == 0x7FC00000, b.view(np.uint32) & 0x7FC00000 == 0x7FC00000) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def _run_dev(L, W, counts, offset):
    """work_dev_counts on a device tensor that starts `offset` floats into its allocation."""
    blk = doa.find_local_max(W, L, 0.0, 180.0)
    buf = torch.zeros(N_ITEMS * L + offset, dtype=torch.float32, device="cuda")
    buf[offset:] = torch.from_numpy(_rows(L).reshape(-1)).cuda()
    dc = torch.from_numpy(np.asarray(counts, np.int32)).cuda()
    o0 = torch.full((N_ITEMS, W), -7.0, dtype=torch.float32, device="cuda")
    o1 = torch.full((N_ITEMS, W), -7.0, dtype=torch.float32, device="cuda")
    assert blk.work_dev_counts(N_ITEMS, buf.data_ptr() + 4 * offset, dc.data_ptr(), o0.data_ptr(), o1.data_ptr(),
                               torch.cuda.current_stream()) == N_ITEMS
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("L", LENGTHS)
def test_counts_cycle_over_every_value(L, W, offset):
    counts = np.arange(N_ITEMS, dtype=np.int32) % (W + 1)            # 0 .. num_max_vals
    got0, got1 = _run_dev(L, W, counts, offset)
    e0, e1 = _expected(L, W, counts)
    assert _same(got0, e0), (L, W, offset, got0[:4], e0[:4])
    assert _same(got1, e1), (L, W, offset, got1[:4], e1[:4])


@pytest.mark.parametrize("L,W", [(20, 2), (256, 1), (256, 5), (1000, 16), (2048, 5), (4100, 2)])
def test_out_of_range_counts_give_nan(L, W):
    counts = np.full(N_ITEMS, W, np.int32)
    bad = {2: -1, 5: W + 1, 11: 99, 20: -2 ** 31, 36: 2 ** 31 - 1}
    for i, m in bad.items():
        counts[i] = m
    got0, got1 = _run_dev(L, W, counts, 0)
    e0, e1 = _expected(L, W, counts)
    for i in bad:
        assert np.all(np.isnan(got0[i])) and np.all(np.isnan(got1[i])), (L, W, i)
    assert _same(got0, e0) and _same(got1, e1)
    # with every count equal to num_max_vals the counted entry is the block itself
    blk = doa.find_local_max(W, L, 0.0, 180.0)
    p0, p1 = np.empty((N_ITEMS, W), np.float32), np.empty((N_ITEMS, W), np.float32)
    blk.work(N_ITEMS, [_rows(L)], [p0, p1])
    keep = [i for i in range(N_ITEMS) if i not in bad]
    assert np.array_equal(got0[keep].view(np.uint32), p0[keep].view(np.uint32))
    assert np.array_equal(got1[keep].view(np.uint32), p1[keep].view(np.uint32))


@pytest.mark.parametrize("L,W", [(64, 2), (1024, 5), (4100, 16)])
def test_host_entry(L, W):
    counts = (np.arange(N_ITEMS, dtype=np.int32) * 3) % (W + 1)
    blk = doa.find_local_max(W, L, 0.0, 180.0)
    o0, o1 = np.full((N_ITEMS, W), -7.0, np.float32), np.full((N_ITEMS, W), -7.0, np.float32)
    assert blk.work_counts(N_ITEMS, [_rows(L)], counts, [o0, o1]) == N_ITEMS
    e0, e1 = _expected(L, W, counts)
    assert _same(o0, e0) and _same(o1, e1)
    d0, d1 = _run_dev(L, W, counts, 0)
    assert np.array_equal(o0.view(np.uint32), d0.view(np.uint32)) and np.array_equal(o1.view(np.uint32), d1.view(np.uint32))


def test_missing_counts_are_rejected():
    blk = doa.find_local_max(2, 64, 0.0, 180.0)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:
        blk.work_dev_counts(1, buf.data_ptr(), None, out.data_ptr(), out.data_ptr() + 8)
    assert ei.value.status == -1
