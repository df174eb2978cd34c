"""GPU tests of doa.wideband_music against the numpy statement (tests/wideband_ref.py): parity to the project's bounds for the
double path (tests/test_gpu_music.py (b) and (d), propagated to first order through the combine rule), the cross-check with
MUSIC_lin_array, what must be the same bit for bit, the counts entries and the status port, and the chain
channel_covariance -> wideband_music -> find_local_max on the three scenarios.

With mx_j = max_p Q_ij and the weights w_j of the used bins:
    null_mean   |q - q_ref| <= 3e-7 q_ref + 2e-13 sum_j w_j mx_j / sum_j w_j
    power_sum   |q - q_ref| <= 3e-7 q_ref + q_ref^2 sum_j w_j 2e-13 mx_j / Q_ij^2 / sum_j w_j
    dB row      |dB - dB_ref| <= 2e-5 + 2e-6 |dB_ref|, the maximum exactly 0 dB at the same direction
on inputs with min_p Q_ij >= 1e-6 mx_j in every bin (asserted on the reference).
The comparisons print their figures as fractions of the bounds before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import wideband_ref as wb

pytestmark = pytest.mark.gpu

BIG = (4, 2, 64, 0, 64, 1024, 9)          # the parity shape the bit-for-bit and counts tests run on
assert BIG in wb.PARITY_SHAPES


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _items(shape):
    R = wb.parity_items(shape)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _reference(shape, combine):
    N, M, F, first, nb, P, n = shape
    return wb.wideband_music(_items(shape), wb.D, M, N, P, F, first, nb, wb.RHO, combine)


def _block(shape, combine="null_mean", rho=wb.RHO, first=None, nb=None):
    N, M, F, first0, nb0, P, _n = shape
    return doa.wideband_music(wb.D, M, N, P, F, first0 if first is None else first, nb0 if nb is None else nb, rho, combine)


def _run(blk, items, weights=None, counts=None):
    """work_dev / work_dev_counts on [n, nb, N*N] items: (spectrum [n, P], q [n, P], status [n])."""
    items = np.asarray(items)
    n, P = items.shape[0], blk.pspectrum_len
    cov = _dev(items.astype(np.complex64).reshape(n * blk.num_bins, -1))
    spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    q = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    w = None if weights is None else _dev(np.asarray(weights, np.float32).reshape(n, blk.num_bins))
    wp = None if w is None else w.data_ptr()
    if counts is None:
        assert blk.work_dev(n, cov.data_ptr(), spec.data_ptr(), wp, q.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    else:
        c = _dev(np.asarray(counts, np.int32).reshape(n, blk.num_bins))
        assert blk.work_dev_counts(n, cov.data_ptr(), c.data_ptr(), spec.data_ptr(), wp, q.data_ptr(), st.data_ptr(),
                                   torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return spec.cpu().numpy(), q.cpu().numpy(), st.cpu().numpy()


def _q_bound(combine, q_ref, Qb, w=None):
    """The bound on |q - q_ref| of the module docstring; Qb [n, nb, P] with NaN rows for the bins not used."""
    used = np.isfinite(Qb[:, :, 0])
    w = np.where(used, 1.0 if w is None else w, 0.0)
    mx = np.where(used, np.nanmax(np.where(used[:, :, None], Qb, 0.0), axis=2), 0.0)
    wsum = w.sum(axis=1)
    if combine == "null_mean":
        return 3e-7 * q_ref + 2e-13 * ((w * mx).sum(axis=1) / wsum)[:, None]
    per_bin = np.where(used[:, :, None], (w * 2e-13 * mx)[:, :, None] / np.where(used[:, :, None], Qb, 1.0) ** 2, 0.0)
    return 3e-7 * q_ref + q_ref ** 2 * per_bin.sum(axis=1) / wsum[:, None]


@pytest.mark.parametrize("shape", wb.PARITY_SHAPES, ids=lambda s: "N{}_M{}_F{}_first{}_nb{}_P{}_n{}".format(*s))
def test_parity_with_the_definition(shape):
    N, M, F, first, nb, P, n = shape
    for combine in wb.COMBINE:
        dB_ref, q_ref, st_ref, Qb = _reference(shape, combine)
        assert not st_ref.any()
        cond = (np.nanmin(Qb, axis=2) / np.nanmax(Qb, axis=2)).min()
        assert cond >= 1e-6, cond                              # the inputs the bounds are stated for
        spec, q, st = _run(_block(shape, combine), _items(shape))
        assert not st.any()
        bound = _q_bound(combine, q_ref, Qb)
        frac_q = (np.abs(q - q_ref) / bound).max()
        frac_db = (np.abs(spec - dB_ref) / (2e-5 + 2e-6 * np.abs(dB_ref))).max()
        print(f"{shape} {combine}: min Q / max Q {cond:.1e}; q at {frac_q:.3f} of its bound, dB at {frac_db:.3f} of its bound")
        assert frac_q <= 1.0
        assert np.all(spec.max(axis=1) == 0.0) and np.array_equal(spec.argmax(axis=1), dB_ref.argmax(axis=1))
        assert frac_db <= 1.0


# ---- cross-check with MUSIC_lin_array ------------------------------------------------------------------------------------------
def test_one_bin_at_the_carrier_is_MUSIC_lin_array():
    """rho = 0, one bin: the row is within twice the dB bound of MUSIC_lin_array.work on the same items, with the same peaks."""
    N, M, F, first, nb, P, n = BIG
    items = _items(BIG)[:, 5:6]
    spec, _, st = _run(_block(BIG, rho=0.0, first=5, nb=1), items)
    want = np.empty((n, P), np.float32)
    doa.MUSIC_lin_array(wb.D, M, N, P).work(n, [items.reshape(n, N * N)], [want])
    assert not st.any()
    frac = (np.abs(spec.astype(np.float64) - want) / (2e-5 + 2e-6 * np.abs(want))).max()
    print(f"one bin against MUSIC_lin_array: dB at {frac:.3f} of the bound (twice allowed)")
    assert frac <= 2.0
    a, b = oracle.find_local_max(spec, M, P, 0.0, 180.0), oracle.find_local_max(want, M, P, 0.0, 180.0)
    assert np.array_equal(a[1], b[1])


def test_eight_bins_at_the_carrier_are_the_mean_of_MUSIC_lin_array_debug():
    """rho = 0, eight bins: the q port is within twice bound (b) of the mean over the bins of MUSIC_lin_array.debug's Q."""
    N, M, F, first, nb, P, n = BIG
    items = _items(BIG)[:, 8:16]
    _, q, st = _run(_block(BIG, rho=0.0, first=8, nb=8), items)
    _, Q = doa.MUSIC_lin_array(wb.D, M, N, P).debug(items.reshape(n * 8, N * N))
    Q = Q.astype(np.float64).reshape(n, 8, P)
    want = Q.mean(axis=1)
    bound = 3e-7 * want + 2e-13 * Q.max(axis=2).mean(axis=1)[:, None]
    frac = (np.abs(q - want) / bound).max()
    print(f"eight bins against the mean of MUSIC_lin_array.debug: q at {frac:.3f} of bound (b) (twice allowed)")
    assert not st.any() and frac <= 2.0


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", wb.COMBINE)
def test_a_snapshot_does_not_depend_on_the_call(combine):
    blk = _block(BIG, combine)
    items = _items(BIG)
    spec, q, st = _run(blk, items)
    for i in range(items.shape[0]):
        s1, q1, st1 = _run(blk, items[i:i + 1])
        assert _same(s1[0], spec[i]) and _same(q1[0], q[i]) and st1[0] == st[i] == 0, i


@pytest.mark.parametrize("combine", wb.COMBINE)
def test_a_selection_is_the_full_band_with_the_other_bins_switched_off(combine):
    """Eight bins against all F with weight 0 outside those eight and NaN items in the skipped bins."""
    N, M, F, first, nb, P, n = BIG
    items = _items(BIG)
    sel = slice(20, 28)
    spec8, q8, st8 = _run(_block(BIG, combine, first=20, nb=8), items[:, sel])
    spoiled = np.full(items.shape, np.nan + 1j * np.nan, np.complex64)
    spoiled[:, sel] = items[:, sel]
    w = np.zeros((n, F), np.float32)
    w[:, sel] = 1.0
    w[:, 0], w[:, 40], w[:, 41] = -1.0, np.inf, np.nan                   # every weight that is not usable skips its bin
    spec, q, st = _run(_block(BIG, combine), spoiled, weights=w)
    assert not st.any() and not st8.any()
    assert _same(spec, spec8) and _same(q, q8)


@pytest.mark.parametrize("combine", wb.COMBINE)
def test_weights(combine):
    """Weights scaled by 2^-3 change nothing; no weights are all ones; and weights weigh (against the reference)."""
    N, M, F, first, nb, P, n = BIG
    blk = _block(BIG, combine)
    items = _items(BIG)
    w = (0.25 + np.random.default_rng(5).random((n, nb))).astype(np.float32)
    a, b = _run(blk, items, weights=w), _run(blk, items, weights=w * np.float32(0.125))
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    c, d = _run(blk, items), _run(blk, items, weights=np.ones((n, nb), np.float32))
    assert _same(c[0], d[0]) and _same(c[1], d[1])
    _, q_ref, _, Qb = wb.wideband_music(items, wb.D, M, N, P, F, first, nb, wb.RHO, combine, weights=w)
    frac = (np.abs(a[1] - q_ref) / _q_bound(combine, q_ref, Qb, w.astype(np.float64))).max()
    print(f"weighted {combine}: q at {frac:.3f} of its bound")
    assert frac <= 1.0 and not _same(a[1], c[1])


def test_host_work_is_work_dev():
    N, M, F, first, nb, P, n = BIG
    blk = _block(BIG)
    items = _items(BIG)
    w = (0.25 + np.random.default_rng(6).random((n, nb))).astype(np.float32)
    spec_dev, _, st_dev = _run(blk, items, weights=w)
    spec, st = np.full((n, P), -7.0, np.float32), np.full(n, -7, np.int32)
    assert blk.work(n, [items.reshape(n * nb, N * N)], [spec, st], weights=w) == n
    assert _same(spec, spec_dev) and np.array_equal(st, st_dev)
    counts = np.full((n, nb), M, np.int32)
    spec_c = np.full((n, P), -7.0, np.float32)
    assert blk.work_counts(n, [items.reshape(n * nb, N * N)], counts, [spec_c], weights=w) == n
    assert _same(spec_c, _run(blk, items, weights=w, counts=counts)[0])
    assert blk.nout_items_total() == 4 * n


# ---- the counts entries and the status port ------------------------------------------------------------------------------------
def test_counts_entries():
    N, M, F, first, nb, P, n = BIG
    blk = _block(BIG)
    items = _items(BIG)
    uniform = np.full((n, nb), M, np.int32)
    clean = _run(blk, items, counts=uniform)
    again = _run(blk, items, counts=uniform.copy())                      # the same counts from a second buffer
    assert not clean[2].any() and _same(clean[0], again[0]) and _same(clean[1], again[1])
    # a count of 0 skips the bin: the same bits as weight 0
    off = np.zeros((n, nb), bool)
    off[1, ::3] = True
    off[4, 5:50] = True
    by_count = _run(blk, items, counts=np.where(off, 0, M))
    by_weight = _run(blk, items, counts=uniform, weights=np.where(off, 0.0, 1.0))
    assert not by_count[2].any() and _same(by_count[0], by_weight[0]) and _same(by_count[1], by_weight[1])
    assert not _same(by_count[0][1], clean[0][1])
    # a count per item is the item's own source count: against the reference
    mixed = np.where(np.arange(nb)[None, :] % 2 == 0, 1, 2) * np.ones((n, 1), int)
    got = _run(blk, items, counts=mixed)
    _, q_ref, _, Qb = wb.wideband_music(items, wb.D, M, N, P, F, first, nb, wb.RHO, "null_mean", counts=mixed)
    frac = (np.abs(got[1] - q_ref) / _q_bound("null_mean", q_ref, Qb)).max()
    print(f"mixed counts: q at {frac:.3f} of its bound")
    assert frac <= 1.0


@pytest.mark.parametrize("combine", wb.COMBINE)
def test_status_and_nan_rows_leave_the_neighbours_alone(combine):
    N, M, F, first, nb, P, n = BIG
    blk = _block(BIG, combine)
    items = _items(BIG)
    uniform = np.full((n, nb), M, np.int32)
    clean = _run(blk, items, counts=uniform)
    counts = uniform.copy()
    counts[1, :] = 0                       # no bin used: status 1
    counts[3, 7] = N                       # status 2
    counts[5, 60] = -1                     # status 2
    spoiled = items.copy()
    spoiled[7, 33] = np.nan                # a used bin's item: status 3
    spoiled[5, 2] = np.nan                 # ... and status 2 wins over 3
    w = np.ones((n, nb), np.float32)
    w[8, :] = 0.0                          # no bin used, by the weights: status 1
    counts[8, 3] = 99                      # (the count of a bin whose weight is not usable is not looked at)
    spec, q, st = _run(blk, spoiled, weights=w, counts=counts)
    want = np.array([0, 1, 0, 2, 0, 2, 0, 3, 1], np.int32)
    assert np.array_equal(st, want), st
    _, _, st_ref, _ = wb.wideband_music(spoiled, wb.D, M, N, P, F, first, nb, wb.RHO, combine, weights=w, counts=counts)
    assert np.array_equal(st_ref, want)
    for i in range(n):
        if want[i]:
            assert np.isnan(spec[i]).all() and np.isnan(q[i]).all(), i
        else:
            assert _same(spec[i], clean[0][i]) and _same(q[i], clean[1][i]), i
    # the entry without counts: status 3 and 1 the same way
    spec, q, st = _run(blk, spoiled, weights=w)
    assert np.array_equal(st, np.array([0, 0, 0, 0, 0, 3, 0, 3, 1], np.int32)), st
    assert np.isnan(spec[[5, 7, 8]]).all() and np.isfinite(spec[[0, 1, 2, 3, 4, 6]]).all()


# ---- end to end on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, combine", [("two", "null_mean"), ("four", "null_mean"), ("split", "power_sum")])
def test_the_chain_on_the_device_finds_the_sources(name, combine):
    """channel_covariance -> wideband_music -> find_local_max: the angles of the reference within one grid step, and within
    the 0.5 degree cap of the use case."""
    s = wb.SCENARIOS[name]
    N, M, K, F, n, P = s["N"], s["M"], s["K"], s["F"], s["n"], wb.P_USE
    num = len(s["thetas"])
    x, items_ref = wb.scenario_items(name)
    cov = np.empty((n * F, N * N), np.complex64)
    produced, _ = doa.channel_covariance(N, K, 0, F, "hann").general_work(n, [x[k] for k in range(N)], [cov])
    assert produced == n
    spec, st = np.empty((n, P), np.float32), np.empty(n, np.int32)
    assert doa.wideband_music(wb.D, M, N, P, F, rate_over_carrier=wb.RHO, combine=combine).work(n, [cov], [spec, st]) == n
    val, loc = np.empty((n, num), np.float32), np.empty((n, num), np.float32)
    assert doa.find_local_max(num, P, 0.0, 180.0).work(n, [spec], [val, loc]) == n
    found = np.sort(loc.astype(np.float64), axis=1)
    dB_ref, _, _, _ = wb.wideband_music(items_ref, wb.D, M, N, P, F, rho=wb.RHO, combine=combine)
    ref = wb.peaks(dB_ref, num)
    err = wb.worst_error(found, s["thetas"])
    print(f"{name} ({combine}): worst error {err:.2f} degrees; largest distance from the reference's angles "
          f"{np.abs(found - ref).max():.3f} degrees")
    assert not st.any()
    assert np.abs(found - ref).max() <= 180.0 / P + 1e-4
    assert err <= 0.5
