"""GPU tests of doa.focus_covariance against the numpy statement (tests/focus_ref.py): parity, the exact Hermitian structure,
what must be the same bit for bit, the status port, the chains channel_covariance -> focus_covariance -> MUSIC / Root-MUSIC /
ESPRIT / MDL on a source and its echo, and the refusals.

The parity bound, per real component c of an output item, with the weights w_j of the used bins:
    |c - c_ref| <= 2^-24 |c_ref| + 2^-40 N sum_j w_j max|R_ij| / sum_j w_j
one rounding to float32 plus the double accumulation of N-term products over the bins, with about ten times room.
The comparisons print their figures as fractions of the bound before they assert; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import focus_ref as fr
import source_count_ref as count_ref
import wideband_ref as wb

pytestmark = pytest.mark.gpu

DOA_ERR_UNSUPPORTED = -4
# N, M (of the generator), F, first_bin, nb, n
SHAPES = [(2, 1, 16, 0, 16, 3), (3, 2, 16, 14, 5, 3), (4, 2, 64, 0, 64, 9), (4, 1, 32, 7, 1, 3), (5, 2, 16, 0, 16, 3),
          (8, 4, 64, 60, 8, 3), (11, 3, 32, 0, 32, 2), (16, 3, 32, 0, 32, 2), (4, 2, 64, 0, 64, 1), (4, 2, 64, 0, 64, 130)]
BIG = SHAPES[2]                          # the shape the bit-for-bit and status tests run on
_ID = "N{}_M{}_F{}_first{}_nb{}_n{}".format


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # a copy: the cached inputs are read-only


@functools.lru_cache(maxsize=None)
def _items(shape):
    N, M, F, first, nb, n = shape
    R = wb.parity_items((N, M, F, first, nb, 0, n))
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _table(shape):
    """The fan of N angles at the shape's selection."""
    N, M, F, first, nb, n = shape
    T = doa.rss_focusing_matrices(wb.D, N, F, fr.fan(N), first, nb, wb.RHO)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def _weights(shape):
    N, M, F, first, nb, n = shape
    w = (0.25 + np.random.default_rng(5).random((n, nb))).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _block(shape):
    return doa.focus_covariance(shape[0], shape[4], _table(shape))


def _run(blk, items, weights=None, lead_items=0):
    """work_dev on [n, nb, N*N] items: (focused items [n, N*N] complex64, status [n]).  lead_items: the input starts that many
    items into its allocation."""
    items = np.asarray(items)
    n, NN = items.shape[0], blk.num_ant_ele ** 2
    flat = items.astype(np.complex64).reshape(n * blk.num_bins, NN)
    if lead_items:
        flat = np.concatenate([np.full((lead_items, NN), 9.0 + 9.0j, np.complex64), flat])
    cov = _dev(flat)
    out = torch.full((n, NN), -7.0, dtype=torch.complex64, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    w = None if weights is None else _dev(np.asarray(weights, np.float32).reshape(n, blk.num_bins))
    assert blk.work_dev(n, cov.data_ptr() + lead_items * NN * 8, out.data_ptr(), None if w is None else w.data_ptr(), st.data_ptr(),
                        torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _fraction(got, ref, items, N, weights=None):
    """The largest |c - c_ref| over the module docstring's bound, over the real components of [n, N*N] items."""
    items = np.asarray(items)
    n, nb = items.shape[:2]
    w = np.ones((n, nb)) if weights is None else np.asarray(weights, np.float64).reshape(n, nb)
    r, c = np.triu_indices(N)
    mx = np.abs(items[:, :, r + c * N]).max(axis=2)
    scale = 2.0 ** -40 * N * (w * mx).sum(axis=1) / w.sum(axis=1)
    worst = 0.0
    for part in (np.real, np.imag):
        bound = 2.0 ** -24 * np.abs(part(ref)) + scale[:, None]
        worst = max(worst, float((np.abs(part(got).astype(np.float64) - part(ref)) / bound).max()))
    return worst


def _assert_exactly_hermitian(out, N):
    A = out.reshape(-1, N, N)                                   # [i, col, row]
    d = np.arange(N)
    assert _same(A.imag[:, d, d], np.zeros((A.shape[0], N), np.float32))         # +0.0, not -0.0
    mirrored, negated = A.imag.transpose(0, 2, 1).copy(), -A.imag
    mirrored[:, d, d] = negated[:, d, d] = 0.0
    assert _same(A.real.transpose(0, 2, 1), A.real) and _same(mirrored, negated)


# ---- parity and structure --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: _ID(*s))
def test_parity_with_the_definition(shape):
    N = shape[0]
    for w in (None, _weights(shape)):
        ref, st_ref = fr.focus_covariance(_items(shape), _table(shape), w)
        got, st = _run(_block(shape), _items(shape), w)
        assert not st_ref.any() and not st.any()
        frac = _fraction(got, ref, _items(shape), N, w)
        print(f"{shape} {'weighted' if w is not None else 'plain'}: at {frac:.3f} of the bound")
        assert frac <= 1.0
        _assert_exactly_hermitian(got, N)


@pytest.mark.parametrize("shape", [SHAPES[1], BIG, SHAPES[6]], ids=lambda s: _ID(*s))
def test_identities_give_the_weighted_mean(shape):
    N, M, F, first, nb, n = shape
    items, w = _items(shape), _weights(shape)
    eye = np.broadcast_to(np.eye(N, dtype=np.complex128), (nb, N, N))
    got, st = _run(doa.focus_covariance(N, nb, eye), items, w)
    w64 = w.astype(np.float64)
    mean = np.array([sum(w64[i, j] * fr.hermitian(items[i, j], N) for j in range(nb)) / w64[i].sum() for i in range(n)])
    frac = _fraction(got, mean.transpose(0, 2, 1).reshape(n, N * N), items, N, w)
    print(f"{shape} identities: at {frac:.3f} of the bound")
    assert not st.any() and frac <= 1.0


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[1], SHAPES[7]], ids=lambda s: _ID(*s))
def test_one_bin_and_the_identity_is_the_item_completed(shape):
    N, n = shape[0], shape[5]
    items = _items(shape)[:, :1]
    got, st = _run(doa.focus_covariance(N, 1, np.eye(N, dtype=np.complex128)[None]), items)
    want = np.array([fr.hermitian(items[i, 0], N).T.reshape(N * N) for i in range(n)]).astype(np.complex64)
    assert not st.any() and _same(got.real, want.real) and _same(got.imag + np.float32(0.0), want.imag + np.float32(0.0))
    _assert_exactly_hermitian(got, N)


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
def test_a_snapshot_does_not_depend_on_the_call():
    blk, items, w = _block(BIG), _items(BIG), _weights(BIG)
    out, st = _run(blk, items, w)
    for i in range(items.shape[0]):
        o1, st1 = _run(blk, items[i:i + 1], w[i:i + 1])
        assert _same(o1[0], out[i]) and st1[0] == st[i] == 0, i
    many = SHAPES[9]                                           # more snapshots than one launch unit takes, whatever the mapping
    out_many, _ = _run(_block(many), _items(many))
    for i in (0, 63, 64, 129):
        assert _same(_run(_block(many), _items(many)[i:i + 1])[0][0], out_many[i]), i


def test_weights():
    """Weights scaled by 2^-3 change nothing; no weights are all ones; and weights weigh."""
    blk, items, w = _block(BIG), _items(BIG), _weights(BIG)
    a, b = _run(blk, items, w), _run(blk, items, w * np.float32(0.125))
    assert _same(a[0], b[0])
    c, d = _run(blk, items), _run(blk, items, np.ones(w.shape, np.float32))
    assert _same(c[0], d[0]) and not _same(a[0], c[0])


def test_host_work_is_work_dev():
    N, M, F, first, nb, n = BIG
    blk, items, w = doa.focus_covariance(N, nb, _table(BIG)), _items(BIG), _weights(BIG)
    out_dev, st_dev = _run(blk, items, w)
    out, st = np.full((n, N * N), -7.0, np.complex64), np.full(n, -7, np.int32)
    assert blk.work(n, [items.reshape(n * nb, N * N)], [out, st], weights=w) == n
    assert _same(out, out_dev) and np.array_equal(st, st_dev)
    out2 = np.full((n, N * N), -7.0, np.complex64)
    assert blk.work(n, [items.reshape(n * nb, N * N)], [out2]) == n             # no status port, no weights
    assert _same(out2, _run(blk, items)[0])
    assert blk.nout_items_total() == 4 * n
    ula = doa.focus_covariance.for_ula(wb.D, N, F, fr.fan(N), first, nb, wb.RHO)
    assert _same(_run(ula, items, w)[0], out_dev)


@pytest.mark.parametrize("shape", [SHAPES[1], BIG, SHAPES[4]], ids=lambda s: _ID(*s))
def test_an_input_one_item_into_its_allocation_gives_the_same_bits(shape):
    """One item further on, an odd-sized item's rounds start on the other 8 bytes of a 16-byte line."""
    blk, items, w = _block(shape), _items(shape), _weights(shape)
    a, b = _run(blk, items, w), _run(blk, items, w, lead_items=1)
    assert _same(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the status port ---------------------------------------------------------------------------------------------------------------
def test_status_and_nan_items_leave_the_neighbours_alone():
    N, M, F, first, nb, n = BIG
    blk, items = _block(BIG), _items(BIG)
    clean, st_clean = _run(blk, items)
    assert not st_clean.any()
    nan = np.complex64(np.nan + 1j * np.nan)
    spoiled, w = items.copy(), np.ones((n, nb), np.float32)
    w[1, :] = 0.0                                   # no bin used: status 1
    w[8, :] = [-1.0, np.inf, np.nan, 0.0] * (nb // 4)           # ... by every kind of weight that is not usable
    spoiled[8, 3] = nan
    spoiled[3, 7] = nan                             # a used bin's item: status 3
    spoiled[5, 60, 4] = np.inf                      # ... one element of its upper triangle, (0, 1)
    spoiled[7, 63, 0] = np.nan                      # ... the real part of a diagonal element in the last bin
    spoiled[2, 10], w[2, 10] = nan, 0.0             # NaN in skipped bins is harmless
    spoiled[2, 11], w[2, 11] = nan, -2.0
    spoiled[2, 12], w[2, 12] = nan, np.inf
    spoiled[2, 13], w[2, 13] = nan, np.nan
    spoiled[4, :, 1] = nan                          # element (1, 0): the lower triangle is not read
    spoiled.imag[4, :, 5] = np.nan                  # element (1, 1): nor the diagonal's imaginary part
    spoiled[6, 20, 11] = np.inf                     # element (3, 2) of a 4 x 4 item: the lower triangle again
    out, st = _run(blk, spoiled, w)
    want = np.array([0, 1, 0, 3, 0, 3, 0, 3, 1], np.int32)
    assert np.array_equal(st, want), st
    ref, st_ref = fr.focus_covariance(spoiled, _table(BIG), w)
    assert np.array_equal(st_ref, want)
    for i in range(n):
        if want[i]:
            assert np.isnan(out[i].real).all() and np.isnan(out[i].imag).all(), i
        elif i == 2:                                # four bins fewer: against the reference, and the same bits as weight 0 alone
            w0 = np.ones(nb, np.float32)
            w0[10:14] = 0.0
            assert _same(out[i], _run(blk, items[i:i + 1], w0[None])[0][0])
            assert _fraction(out[i:i + 1], ref[i:i + 1], items[i:i + 1], N, w0[None]) <= 1.0
        else:
            assert _same(out[i], clean[i]), i


# ---- the chains on the device ------------------------------------------------------------------------------------------------------
MDL_SNAPSHOTS = 16          # K / F: the blocks behind one bin's item


@pytest.mark.parametrize("name", ["echo4", "echo8"])
def test_the_chains_on_the_device_find_the_source_and_its_echo(name):
    """channel_covariance -> focus_covariance (the table of the reference's second pass) -> MUSIC_lin_array + find_local_max,
    rootMUSIC_linear_array, esprit_linear_array, source_count."""
    s = fr.SCENARIOS[name]
    N, K, n, F, P, M = s["N"], s["K"], s["n"], fr.F_USE, fr.P_USE, fr.M_USE
    x, items_ref = fr.scenario_items(name)
    _, angles, focused_ref, music_ref = fr.two_pass(name)
    cov = np.empty((n * F, N * N), np.complex64)
    produced, _ = doa.channel_covariance(N, K, 0, F, "hann").general_work(n, [x[k] for k in range(N)], [cov])
    assert produced == n
    foc, st = np.empty((n, N * N), np.complex64), np.empty(n, np.int32)
    assert doa.focus_covariance.for_ula(fr.D, N, F, angles, rate_over_carrier=fr.RHO).work(n, [cov], [foc, st]) == n
    assert not st.any()
    _assert_exactly_hermitian(foc, N)
    # MUSIC on the grid
    spec = np.empty((n, P), np.float32)
    assert doa.MUSIC_lin_array(fr.D, M, N, P).work(n, [foc], [spec]) == n
    val, loc = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
    assert doa.find_local_max(M, P, 0.0, 180.0).work(n, [spec], [val, loc]) == n
    found = np.sort(loc.astype(np.float64), axis=1)
    e_music = wb.worst_error(found, s["thetas"])
    print(f"{name}: MUSIC worst error {e_music:.2f} degrees, largest distance from the reference chain {np.abs(found - music_ref).max():.3f}")
    assert np.abs(found - music_ref).max() <= 180.0 / P + 1e-4
    assert e_music <= 0.5
    # the grid-free estimators; first what a float64 Root-MUSIC makes of the reference's focused items
    root64 = np.sort(oracle.root_music(focused_ref.astype(np.complex64), fr.D, M, N, "f64").astype(np.float64), axis=1)
    e_root64 = wb.worst_error(root64, s["thetas"])
    assert e_root64 <= 0.5, e_root64
    ang = np.empty((n, M), np.float32)
    assert doa.rootMUSIC_linear_array(fr.D, M, N).work(n, [foc], [ang]) == n
    e_root = wb.worst_error(np.sort(ang.astype(np.float64), axis=1), s["thetas"])
    ang_e, st_e = np.empty((n, M), np.float32), np.empty(n, np.int32)
    assert doa.esprit_linear_array(fr.D, M, N).work(n, [foc], [ang_e, st_e]) == n
    e_esprit = wb.worst_error(np.sort(ang_e.astype(np.float64), axis=1), s["thetas"])
    print(f"{name}: Root-MUSIC {e_root:.2f} (float64 on the reference's items {e_root64:.2f}), ESPRIT {e_esprit:.2f} degrees")
    assert e_root <= 0.5
    assert not st_e.any() and e_esprit <= 0.5
    # the source count: one source in a bin, two in the focused item
    assert np.array_equal(count_ref.source_count(items_ref[:, 5], N, MDL_SNAPSHOTS, count_ref.MDL)[0], np.ones(n, np.int32))
    assert np.array_equal(count_ref.source_count(focused_ref.astype(np.complex64), N, MDL_SNAPSHOTS, count_ref.MDL)[0], np.full(n, 2))
    counts = np.empty(n, np.int32)
    assert doa.source_count(N, MDL_SNAPSHOTS, "mdl").work(n, [foc], [counts]) == n
    assert np.array_equal(counts, np.full(n, 2, np.int32)), counts


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_and_precision_32_is_unsupported():
    T = np.array(_table(BIG))
    bad = T.copy()
    bad[9, 2, 1] = np.inf
    for args in ((1, 64, T), (17, 64, T), (4, 0, T), (4, 257, T), (4, 64, bad), (4, 64, None)):
        with pytest.raises((doa.DoaError, ValueError)):
            doa.focus_covariance(*args)
    N, M, F, first, nb, n = BIG
    assert doa.get_internal_precision() == 64
    doa.set_internal_precision(32)
    try:
        blk32 = doa.focus_covariance(N, nb, T)
    finally:
        doa.set_internal_precision(64)
    out = np.empty((n, N * N), np.complex64)
    with pytest.raises(doa.DoaError) as ei:
        blk32.work(n, [_items(BIG).reshape(n * nb, N * N)], [out])
    assert ei.value.status == DOA_ERR_UNSUPPORTED and "precision 64" in str(ei.value)
    cov = _dev(_items(BIG).reshape(n * nb, N * N))
    with pytest.raises(doa.DoaError) as ei:
        blk32.work_dev(n, cov.data_ptr(), _dev(out).data_ptr())
    assert ei.value.status == DOA_ERR_UNSUPPORTED
