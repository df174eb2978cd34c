"""GPU tests of rootMUSIC_linear_array with a source count per item (work_counts / work_dev_counts / select_counts_debug) on
the shared covariance cases (tests/source_count_cases.py: N = 2, 3, 4, 5, 8, 9, 12, 16; 37 and 67 items leave the last wave
partial).  Every item with a count m >= 1 is compared with oracle.root_music(R[i:i+1], d, m, N, "f64") under the bar
tests/test_gpu_root_music.py holds the fixed block to against fp64: |angle - angle_f64| <= 1e-3 degrees.

That bar is meaningful for an item whose fp64 reference is DECIDED: a root within rounding of the unit circle, two interior
roots at (almost) the same distance competing for the last pick, or a picked root at the edge of the visible region would
make the reference's own answer a coin toss.  Decided = all three margins >= 1e-6:
  (1) the smallest |1 - |z|| over the 2N-2 roots,
  (2) the gap between the m-th and the (m+1)-th smallest interior distance,
  (3) |1 - |arg z / (2 pi d)|| of the m selected roots.
On these cases every item is decided (minima over all cases, forced counts: 2.8e-6, 3.3e-4, 9.0e-5; MDL counts: 1.2e-5, 0.23,
0.09), so the tests ASSERT that no item is undecided and skip none."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import source_count_cases as cases
import source_count_ref as ref

pytestmark = pytest.mark.gpu

NAMES = sorted(cases.CASES)
MARGIN = 1e-6
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _reference(name, i, m):
    """(fp64 angles [m], (margin 1, margin 2, margin 3)) of item i of the case with m sources."""
    N, d = cases.CASES[name][0], cases.CASES[name][2]
    R = cases.covariance(name)
    ang = oracle.root_music(R[i:i + 1], d, m, N, "f64")[0]
    z = oracle.root_music_roots(oracle.noise_projector(R[i], m, N, "f64"), "f64")
    dist = 1.0 - np.abs(z)
    inside = np.flatnonzero(dist > 0.0)
    order = inside[np.argsort(dist[inside], kind="stable")]
    ds = dist[order]
    gap = float(ds[m] - ds[m - 1]) if len(ds) > m else np.inf
    picked = z[order[:m]]
    edge = float(np.min(np.abs(1.0 - np.abs(np.angle(picked) / (2 * np.pi * float(np.float32(d))))))) if len(picked) else np.inf
    ang.setflags(write=False)
    return ang, (float(np.abs(dist).min()), gap, edge)


def _run(name, counts, W=None):
    """(angles [n, W], status [n]) of work_dev_counts on the case's covariances."""
    N, d = cases.CASES[name][0], cases.CASES[name][2]
    W = N - 1 if W is None else W
    R = cases.covariance(name)
    n = R.shape[0]
    blk = doa.rootMUSIC_linear_array(d, W, N)
    dR = torch.from_numpy(R.copy()).cuda()
    dc = torch.from_numpy(np.array(counts, dtype=np.int32)).cuda()          # (a writable copy)
    out = torch.full((n, W), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert blk.work_dev_counts(n, dR.data_ptr(), dc.data_ptr(), out.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _check(name, ang, status, counts, what):
    W = ang.shape[1]
    worst, margins = 0.0, [np.inf, np.inf, np.inf]
    undecided = []
    for i, m in enumerate(int(c) for c in counts):
        if m == 0:
            assert np.all(np.isnan(ang[i])) and status[i] == 0, (name, what, i, ang[i], status[i])
            continue
        want, mg = _reference(name, i, m)
        margins = [min(a, b) for a, b in zip(margins, mg)]
        if min(mg) < MARGIN:
            undecided.append((i, m, mg))
            continue
        got = ang[i, :m]
        assert status[i] == 0, (name, what, i, m, status[i])
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, what, i, m, got, want)
        ok = ~np.isnan(want)
        diff = np.abs(got[ok].astype(np.float64) - want[ok])
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
        assert np.all(diff <= 1e-3), (name, what, i, m, got, want)
        assert np.all(np.diff(got[ok]) >= 0.0), (name, what, i, m, got)               # ascending, NaN last
        assert np.all(np.isnan(ang[i, m:])), (name, what, i, m, ang[i])
    print(name, what, "worst |angle - angle_f64| = %.3g deg; smallest margins %.3g %.3g %.3g" % (worst, *margins))
    assert not undecided, (name, what, undecided)


@pytest.mark.parametrize("name", NAMES)
def test_forced_counts_cover_every_value_inside_one_wave(name):
    N, n = cases.CASES[name][0], cases.CASES[name][7]
    counts = np.arange(n, dtype=np.int32) % N                          # 0 .. N-1 = W
    ang, status = _run(name, counts)
    _check(name, ang, status, counts, "forced")


@pytest.mark.parametrize("name", NAMES)
def test_counts_from_the_reference_estimator(name):
    counts = cases.reference(name, ref.MDL)[0]
    assert counts.min() >= 0
    ang, status = _run(name, counts)
    _check(name, ang, status, counts, "estimated")


@pytest.mark.parametrize("name", ["n4_two_fb", "n3_two", "n5_two_s0", "n12_four_s0", "n8_three", "n16_three_fb"])
def test_invalid_counts_give_nan_rows_status_2_and_leave_neighbours_intact(name):
    N, n = cases.CASES[name][0], cases.CASES[name][7]
    good = np.arange(n, dtype=np.int32) % N
    counts = good.copy()
    bad = [1, 6, 12, 13, 15]
    counts[bad] = [-1, N, 99, INT_MIN, INT_MAX]
    (a, sa), (b, sb) = _run(name, good), _run(name, counts)
    for i in bad:
        assert np.all(np.isnan(b[i])) and sb[i] == 2, (name, i, b[i], sb[i])
    keep = np.ones(n, bool)
    keep[bad] = False
    assert _same(a[keep], b[keep]) and np.array_equal(sa[keep], sb[keep])
    assert not sa.any()


@pytest.mark.parametrize("name", NAMES)
def test_uniform_counts_agree_with_work(name):
    """Not bit-equal: work may take the subspace-iteration route, the counted entry always runs the Jacobi."""
    N, d, n = cases.CASES[name][0], cases.CASES[name][2], cases.CASES[name][7]
    M = len(cases.CASES[name][1])
    R = cases.covariance(name)
    blk = doa.rootMUSIC_linear_array(d, M, N)
    want = np.empty((n, M), np.float32)
    assert blk.work(n, [R], [want]) == n
    got = np.full((n, M), -7.0, np.float32)
    assert blk.work_counts(n, [R], np.full(n, M, np.int32), [got]) == n
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(got[ok].astype(np.float64) - want[ok]).max() <= 1e-3, (name, np.abs(got[ok] - want[ok]).max())


# ---- the selection stage on hand-made roots ---------------------------------------------------------------------------------
def _root_sets(N, d, rng):
    """Root lists [n, 2N-2] that drive the branches of the selection rule for every count 1..N-1."""
    D = 2 * N - 2
    ph = lambda k: np.exp(1j * rng.uniform(-2 * np.pi * d, 2 * np.pi * d, k))       # visible region: real angles
    on = np.array([1.0, -1.0, 1j, -1j])                                             # |z| == 1.0 exactly
    out = [rng.uniform(0.2, 0.98, D) * ph(D)]                                       # interior roots only
    for j in range(D + 1):                                                          # j interior roots (0 = none): padding, error
        out.append(rng.permutation(np.concatenate([rng.uniform(0.2, 0.98, j) * ph(j), rng.uniform(1.02, 3.0, D - j) * ph(D - j)])))
    for j in range(1, min(D, 4) + 1):                                               # roots exactly on the circle are not inside
        z = np.concatenate([on[:j], rng.uniform(0.3, 0.9, D - j) * ph(D - j)])
        out += [z, z[::-1].copy()]
    out.append(np.concatenate([on[:min(D, 4)], rng.uniform(1.1, 2.0, D - min(D, 4)) * ph(D - min(D, 4))]))   # on + outside: none
    for r in (0.5, 0.75):                                                           # equal distances: the first in order wins
        k = min(D, 4)
        z = np.concatenate([r * on[:k], rng.uniform(0.1, 0.3, D - k) * ph(D - k)])
        out += [z, np.roll(z, 1), z[::-1].copy()]
    return np.stack([np.asarray(z, np.complex128) for z in out])


@pytest.mark.parametrize("N,d", [(2, 0.5), (4, 0.44), (5, 0.3), (16, 0.5)])
def test_counted_selection_equals_the_fixed_selection_of_that_count(N, d):
    """An item with count m is bit-identical to the select_debug row of a num_targets = m handle on the same roots, and
    agrees with the oracle's restatement of the rule to the existing selection test's 2e-5."""
    W = N - 1
    sets = _root_sets(N, d, np.random.default_rng(77 + N))
    ns = len(sets)
    # every set with every count 0..W and three unusable ones, the counts interleaved so that neighbours in a wave differ
    cvals = list(range(W + 1)) + [-1, W + 1, INT_MAX]
    roots = np.repeat(sets, len(cvals), axis=0)
    counts = np.tile(np.array(cvals, np.int64), ns).astype(np.int32)
    ang, status = doa.rootMUSIC_linear_array(d, W, N).select_counts_debug(roots, counts)
    ang, status = ang.reshape(ns, len(cvals), W), status.reshape(ns, len(cvals))
    with np.errstate(invalid="ignore"):
        n_in = np.sum(1.0 - np.abs(sets) > 0.0, axis=1)
    assert (n_in == 0).sum() >= 2 and (n_in < W).any() and (n_in == 2 * N - 2).any()
    for m in range(1, W + 1):
        want, wst = doa.rootMUSIC_linear_array(d, m, N).select_debug(sets)
        assert _same(ang[:, m, :m], want), (N, m)
        assert np.array_equal(status[:, m], wst), (N, m)
        assert np.all(np.isnan(ang[:, m, m:]))
        assert np.array_equal(wst == 1, n_in == 0)
        for s in np.flatnonzero(n_in > 0):
            w64 = oracle.root_music_select(sets[s], d, m, "f64")
            w64 = np.concatenate([np.sort(w64[~np.isnan(w64)]), w64[np.isnan(w64)]])
            got = ang[s, m, :m]
            assert np.array_equal(np.isnan(got), np.isnan(w64)), (N, m, s)
            ok = ~np.isnan(w64)
            assert np.all(np.abs(got[ok] - w64[ok]) <= 2e-5), (N, m, s, got, w64)
            if n_in[s] < m:
                assert np.sum(got == 90.0) >= m - n_in[s]
    assert np.all(np.isnan(ang[:, 0])) and not status[:, 0].any()                   # count 0
    assert np.all(np.isnan(ang[:, W + 1:])) and np.all(status[:, W + 1:] == 2)      # no usable count


# ---- further checks ---------------------------------------------------------------------------------------------------------
def test_device_entry_equals_host_entry():
    name = "n5_two_s1"
    N, d, n = cases.CASES[name][0], cases.CASES[name][2], cases.CASES[name][7]
    counts = np.arange(n, dtype=np.int32) % N
    counts[[3, 9]] = [-1, 77]                                          # status 2 is not an error of the host entry
    dev, status = _run(name, counts)
    host = np.full((n, N - 1), -7.0, np.float32)
    assert doa.rootMUSIC_linear_array(d, N - 1, N).work_counts(n, [cases.covariance(name)], counts, [host]) == n
    assert _same(host, dev)
    assert np.array_equal(np.flatnonzero(status), [3, 9])


def test_counts_above_a_narrow_handles_num_targets_are_status_2():
    name = "n8_three"
    N, n = cases.CASES[name][0], cases.CASES[name][7]
    W = 3
    counts = np.arange(n, dtype=np.int32) % N                          # 0..7: 4..7 exceed W
    full, _ = _run(name, counts)
    ang, status = _run(name, counts, W)
    over = counts > W
    assert over.any() and np.all(status[over] == 2) and np.all(np.isnan(ang[over]))
    assert not status[~over].any()
    assert _same(ang[~over], np.ascontiguousarray(full[~over][:, :W]))   # the same picks in a narrower item


def test_rejections():
    name = "n4_one"
    R = cases.covariance(name)
    blk = doa.rootMUSIC_linear_array(0.5, 2, 4)
    out = np.empty((4, 2), np.float32)
    blk.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        blk.work_counts(4, [R], np.ones(4, np.int32), [out])
    assert ei.value.status == -4                                        # DOA_ERR_UNSUPPORTED
    dR = torch.from_numpy(R.copy()).cuda()
    dc = torch.ones(4, dtype=torch.int32, device="cuda")
    dout = torch.empty((4, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:
        blk.work_dev_counts(4, dR.data_ptr(), dc.data_ptr(), dout.data_ptr())
    assert ei.value.status == -4
    blk.set_internal_precision(64)
    assert blk.work_counts(4, [R], np.ones(4, np.int32), [out]) == 4
    with pytest.raises(doa.DoaError) as ei:
        blk.work_dev_counts(4, dR.data_ptr(), None, dout.data_ptr())
    assert ei.value.status == -1                                        # NULL counts


def test_non_finite_item_is_status_1_and_spares_its_neighbours():
    name = "n5_two_s0"
    N, d, n = cases.CASES[name][0], cases.CASES[name][2], cases.CASES[name][7]
    counts = np.arange(n, dtype=np.int32) % N
    bad = 7                                                            # count 2: a valid count
    assert counts[bad] == 2
    R = cases.covariance(name).copy()
    R[bad, N] = complex(np.nan, 0.0)                                   # element (0, 1): in the upper triangle, which is read
    blk = doa.rootMUSIC_linear_array(d, N - 1, N)
    dR = torch.from_numpy(R).cuda()
    dc = torch.from_numpy(counts).cuda()
    out = torch.full((n, N - 1), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    blk.work_dev_counts(n, dR.data_ptr(), dc.data_ptr(), out.data_ptr(), st.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    ang, status = out.cpu().numpy(), st.cpu().numpy()
    clean, cst = _run(name, counts)
    assert status[bad] == 1 and np.all(np.isnan(ang[bad]))
    keep = np.arange(n) != bad
    assert _same(ang[keep], clean[keep]) and np.array_equal(status[keep], cst[keep])
    # and the host entry reports exactly this item
    host = np.empty((n, N - 1), np.float32)
    with pytest.raises(doa.DoaError) as ei:
        blk.work_counts(n, [R], counts, [host])
    assert ei.value.status == -5 and "item %d " % bad in str(ei.value)  # DOA_ERR_NUMERIC
    assert _same(host[keep], clean[keep])
