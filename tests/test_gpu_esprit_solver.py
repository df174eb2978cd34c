"""GPU tests of esprit_kernel's eigenvalue solver on inputs the simulated covariances of tests/test_gpu_esprit.py never give it.

a - d run the kernel alone on caller-supplied signal-subspace records (esprit_linear_array.record_debug): random orthonormal
subspaces, whose Psi is far from unitary, has eigenvalues of every modulus and about one eigenvalue in five outside the
visible region (rows that mix angles and NaN), and whose neighbours in a wave need very different numbers of QR steps;
records with gamma a factor of two on either side of DOA_ESPRIT_GAMMA_MIN; shift matrices (all eigenvalues zero, the
extreme non-normal case, and the Householder step's special cases).  e runs the public block on analytic covariances at every (N, M), with components outside the
visible region, tied signal eigenvalues and other spacings.

Every comparison uses BOUND_DEG = 1e-3 degrees (the project's parity bound) or bit identity.  An item of a - b is compared
with the definition when esprit_ref.comparable holds: every eigenvalue's predicted amplification amp <= 1e8 degrees per unit
relative perturbation (1e8 * 2^-52 = 2.2e-8 degrees, a factor of 4.5e4 below the bound for the algorithm's constant) and
| |c| - 1 | >= 1e-6 (the NaN decision is well posed).  At most 5 % of a shape's items may fail the gate; asserted first.

The figures these tests print on an MI355X are kept in profiles/esprit_test_figures.txt; run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

import doa
import esprit_ref as ref

pytestmark = pytest.mark.gpu

BOUND_DEG = 1e-3                   # the project's Root-MUSIC parity bound (tests/test_gpu_root_music.py)
N_WAVE = ref.N_ITEMS               # 67 items: a partial wave at every group width, for the tests that plant items
PLANT_AT = (1, 9, 30, 63)          # each shares its wave with ordinary items, at every group width


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _solve(N, W, records, counts=None, d=ref.D):
    """(angles [n, W], status [n]) of esprit_kernel alone on the records; identity items pass the trace test."""
    records = np.asarray(records).reshape(-1, 2 * N * N)
    return doa.esprit_linear_array(d, W, N).record_debug(ref.identity_items(records.shape[0], N), records, counts)


@functools.lru_cache(maxsize=None)
def _device(N, m, n=ref.N_RECORDS):
    ang, st = _solve(N, m, ref.random_records(N, m, n)[1])
    ang.setflags(write=False); st.setflags(write=False)
    return ang, st


def _assert_row_shape(ang, st):
    """Every item: all-NaN if and only if status != 0; finite angles ascending, NaN last."""
    nan = np.isnan(ang)
    assert np.array_equal(nan.all(axis=1), st != 0), (np.flatnonzero(nan.all(axis=1)), np.flatnonzero(st))
    assert not (nan[:, :-1] & ~nan[:, 1:]).any()                      # no finite angle after a NaN
    with np.errstate(invalid="ignore"):
        assert not (np.diff(ang, axis=1) < 0).any()                   # (a comparison with NaN is False)


def _worst_error(ang, a_ref, rows):
    """Largest |device - reference| over the finite entries of the rows (their NaN positions already agree)."""
    with np.errstate(invalid="ignore"):
        err = np.abs(ang[rows].astype(np.float64) - a_ref[rows].astype(np.float64))
    return float(np.nanmax(err)) if np.isfinite(err).any() else 0.0


# ---- a: random records against the definition --------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", ref.RECORD_SHAPES)
def test_random_records_match_the_definition(N, m):
    a_ref, st_ref, gamma, c, amp, ok = ref.record_reference(N, m)
    share = 1.0 - float(ok.mean())
    assert np.all(st_ref == 0)
    assert share <= ref.NONCOMPARABLE_CAP, share
    ang, st = _device(N, m)
    mixed = np.isnan(a_ref).any(axis=1) & ~np.isnan(a_ref).all(axis=1)
    same_nan = np.array_equal(np.isnan(ang[ok]), np.isnan(a_ref[ok]))
    worst = _worst_error(ang, a_ref, ok & (st == 0)) if same_nan else float("nan")
    print("records N=%d m=%d: %d items, %d rows mix angles and NaN, gamma >= %.3g, non-comparable share %.4f, worst |device - "
          "reference| %.3g deg = %.3g of the bound, status 3 on %d comparable and %d of the %d other items"
          % (N, m, len(st), int(mixed.sum()), gamma.min(), share, worst, worst / BOUND_DEG, int((st[ok] == 3).sum()),
             int((st[~ok] == 3).sum()), int((~ok).sum())))
    _assert_row_shape(ang, st)
    assert np.isin(st, (0, 3)).all(), np.unique(st)
    assert np.all(st[ok] == 0), np.flatnonzero(ok & (st != 0))
    assert same_nan
    assert worst <= BOUND_DEG


# ---- b: bit properties on the same records ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", ref.RECORD_SHAPES)
def test_a_record_alone_gives_the_bits_it_has_in_the_batch(N, m):
    rec = ref.random_records(N, m)[1]
    ang, st = _device(N, m)
    for k in (0, 101, 214, 327, ref.N_RECORDS - 1):                  # lanes 0, 5, 6, 7 and 2 of a 16-item wave
        one, st1 = _solve(N, m, rec[k:k + 1])
        assert st1[0] == st[k] and _same(one[0], ang[k]), k


@pytest.mark.parametrize("N,W", [(16, 15), (8, 7), (4, 3)])
def test_counted_records_equal_the_fixed_launches(N, W):
    """Counts cycle through -1, 0 .. N: items that iterate (m >= 3), closed forms (m = 1, 2), empty and refused items share
    every wave."""
    rec = ref.random_records(N, W)[1]
    values = list(range(-1, N + 1))
    counts = np.array([values[i % len(values)] for i in range(ref.N_RECORDS)], np.int32)
    ang, st = _solve(N, W, rec, counts)
    fixed = {m: _solve(N, m, rec) for m in range(1, W + 1)}
    want_st = np.where((counts < 0) | (counts > W), 2, 0).astype(np.int32)      # esprit_ref.esprit_counts' rule
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)
    for i, m in enumerate(counts):
        if m < 1 or m > W:
            assert np.isnan(ang[i]).all(), (i, m)
        else:
            a_m, st_m = fixed[m]
            assert st_m[i] == 0 and _same(ang[i, :m], a_m[i]) and np.isnan(ang[i, m:]).all(), (i, m)
    # the fixed W launch itself is the one test a compared with the definition
    assert _same(fixed[W][0], _device(N, W)[0])


# ---- c: gamma near its threshold, status only -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 5, 16])
def test_gamma_on_either_side_of_its_threshold(N):
    """m = 1, |Es[N-1]|^2 = 1 - 2^-29 and 1 - 2^-31: gamma a factor of two above and below DOA_ESPRIT_GAMMA_MIN = 2^-30;
    the rounding of the sum of squares (2^-53 relative) cannot move either across it."""
    Es, rec = ref.random_records(N, 1, N_WAVE)
    clean, st_clean = _solve(N, 1, rec)
    planted = np.array(Es)
    want = np.zeros(N_WAVE, np.int32)
    for k, pos in enumerate(PLANT_AT):
        g = 2.0 ** -29 if k % 2 == 0 else 2.0 ** -31
        col = np.zeros(N, np.complex128)
        col[0] = np.sqrt(g) * np.exp(0.3j)
        col[N - 1] = np.sqrt(1.0 - g) * np.exp(-1.1j * k)
        planted[pos, :, 0] = col
        want[pos] = 0 if k % 2 == 0 else 1
        assert ref.esprit_from_record(planted[pos], ref.D, 1)[1] == want[pos]
    ang, st = _solve(N, 1, ref.pack_records(planted, N))
    others = np.ones(N_WAVE, bool); others[list(PLANT_AT)] = False
    assert np.array_equal(st[~others], want[~others]), st[~others]
    assert np.isnan(ang[st == 1]).all()
    assert np.array_equal(st[others], st_clean[others]) and _same(ang[others], clean[others])


# ---- d: structured records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(4, 3), (8, 3), (8, 7), (16, 7)])
def test_shift_matrices_terminate(N, m):
    """Es = (e_0 .. e_{m-1}): Psi is the upper shift, already triangular, every Householder step with tail2 == 0; the columns
    in reverse order: Psi is the lower shift, one Jordan block; the columns (e_{m-1}, e_0, .. e_{m-2}): column 0 of Psi is
    e_{m-1}, the first Householder step has a0 == 0 with tail2 > 0.  All eigenvalues are zero, so the angles are not
    comparable; the solver has to end (at most 30 m steps by construction) with status 0 or 3 and leave its neighbours
    alone."""
    Es, rec = ref.random_records(N, m, N_WAVE)
    clean, st_clean = _solve(N, m, rec)
    upper = np.eye(N, m, dtype=np.complex128)
    shapes = {"upper": upper, "lower": upper[:, ::-1], "rotated": upper[:, [m - 1] + list(range(m - 1))]}
    for name, E in shapes.items():                         # what the names promise, from the definition of Psi (gamma = 1)
        Psi = E[:-1].conj().T @ E[1:]
        assert np.array_equal(Psi, {"upper": np.eye(m, k=1), "lower": np.eye(m, k=-1)}.get(name, Psi))
        assert not np.linalg.matrix_power(Psi, m).any()
    Psi = shapes["rotated"][:-1].conj().T @ shapes["rotated"][1:]
    assert Psi[1, 0] == 0 and Psi[m - 1, 0] == 1
    at = {"upper": (1, 30), "lower": (9, 63), "rotated": (17, 44)}     # each shares its wave with ordinary items
    planted = np.array(Es)
    for name, where in at.items():
        planted[list(where)] = shapes[name]
    ang, st = _solve(N, m, ref.pack_records(planted, N))
    print("shift matrices N=%d m=%d: status and angles of the %s"
          % (N, m, ", ".join("%s %s %s" % (k, st[list(w)].tolist(), ang[w[0]].tolist()) for k, w in at.items())))
    every = [i for w in at.values() for i in w]
    assert np.isin(st[every], (0, 3)).all(), st[every]
    assert np.array_equal(np.isnan(ang[every]).all(axis=1), st[every] != 0)
    for a, b in at.values():
        assert st[a] == st[b] and _same(ang[a], ang[b])
    others = np.ones(N_WAVE, bool); others[every] = False
    assert np.array_equal(st[others], st_clean[others]) and _same(ang[others], clean[others])


# ---- e: the public block on analytic covariances ---------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _block(N, M, R, d=ref.D):
    """(angles, status) of work_dev; work gives the same bits."""
    n = R.shape[0]
    blk = doa.esprit_linear_array(d, M, N)
    dR = _dev(R)
    ang = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert blk.work_dev(n, dR.data_ptr(), ang.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    ang, st = ang.cpu().numpy(), st.cpu().numpy()
    h_ang, h_st = np.empty((n, M), np.float32), np.empty(n, np.int32)
    assert blk.work(n, [R], [h_ang, h_st]) == n
    assert _same(h_ang, ang) and np.array_equal(h_st, st)
    return ang, st


def _compare_with_the_definition(name, N, M, R, d=ref.D, nan_counts=(0,), quiet=False):
    """The existing well-posedness gate (gamma >= 1e-4, gap >= 1e-4) and the solver gate hold for EVERY item (asserted, none
    left out); then status 0, the reference's NaN positions, the finite angles within BOUND_DEG.  Prints its figures first."""
    a_ref, st_ref, gamma, gap, amp, edge = ref.esprit_gated(R, d, M, N)
    ang, st = _block(N, M, R, d)
    same_nan = np.array_equal(np.isnan(ang), np.isnan(a_ref))
    worst = _worst_error(ang, a_ref, np.ones(len(st), bool)) if same_nan else float("nan")
    if not quiet:
        print("%s: %d items, gamma >= %.3g, gap >= %.3g, amp <= %.3g, NaN per row %s, worst |device - reference| %.3g deg = "
              "%.3g of the bound, status max %d" % (name, len(st), gamma.min(), gap.min(), amp.max(),
                                                    sorted(set(np.isnan(a_ref).sum(axis=1).tolist())), worst, worst / BOUND_DEG, st.max()))
    assert np.all(st_ref == 0)
    assert gamma.min() >= 1e-4 and gap.min() >= 1e-4, (name, gamma.min(), gap.min())
    assert amp.max() <= ref.AMP_MAX and edge.min() >= ref.EDGE_MIN, (name, amp.max(), edge.min())
    assert set(np.isnan(a_ref).sum(axis=1).tolist()) <= set(nan_counts), name
    assert np.all(st == 0), (name, st)
    assert same_nan, name
    assert worst <= BOUND_DEG, (name, worst)
    _assert_row_shape(ang, st)
    return worst, float(gamma.min()), float(gap.min()), float(amp.max())


@pytest.mark.parametrize("N", range(2, 17))
def test_block_matches_the_definition_at_every_shape(N):
    """Every M = 1 .. N-1: sources evenly spread over 25 .. 155 degrees, powers U(0.5, 2), sigma2 = 0.01, 19 items."""
    rows = [(M,) + _compare_with_the_definition("N=%d M=%d" % (N, M), N, M, ref.spread_items(N, M), quiet=True)
            for M in range(1, N)]
    worst = max(rows, key=lambda r: r[1])
    print("every shape N=%d, M=1..%d, %d items each: gamma >= %.3g, gap >= %.3g, amp <= %.3g, worst |device - reference| "
          "%.3g deg = %.3g of the bound (M=%d)" % (N, N - 1, ref.ANALYTIC_ITEMS, min(r[2] for r in rows), min(r[3] for r in rows),
                                                max(r[4] for r in rows), worst[1], worst[1] / BOUND_DEG, worst[0]))


@pytest.mark.parametrize("N", sorted(ref.OUT_OF_VISIBLE))
def test_components_outside_the_visible_region_read_nan(N):
    M = len(ref.OUT_OF_VISIBLE[N])
    R = ref.out_of_visible_items(N)
    worst, gamma, gap, amp = _compare_with_the_definition("out of visible N=%d M=%d" % (N, M), N, M, R, nan_counts=(1, 2))
    assert gamma >= 0.57 and gap >= 0.13 and amp < 100.0, (gamma, gap, amp)


def test_equal_power_sources_on_the_dft_grid():
    """Orthogonal steering vectors of equal power: the signal eigenvalues tie and the eigen stage's basis of the signal
    subspace is arbitrary; Psi's eigenvalues, and so the angles, are not."""
    _compare_with_the_definition("dft grid N=8 M=4", 8, 4, ref.dft_grid_items())


@pytest.mark.parametrize("d", [0.25, 0.5])
def test_other_spacings(d):
    thetas = (40.0, 85.0, 130.0)                                     # at least 20 degrees from endfire
    R = ref.spread_items(8, 3, d, thetas)
    _compare_with_the_definition("spacing d=%g N=8 M=3" % d, 8, 3, R, d)


def test_pipeline_reads_nan_for_a_component_outside_the_visible_region():
    """root_pipeline.set_estimator("esprit").work_dev on streams synthesized with the N = 8 phases of OUT_OF_VISIBLE: the
    angles against the definition on the covariance items the pipeline itself produced, and the block's bits on them."""
    N, K, n = 8, 256, 23
    phases = ref.OUT_OF_VISIBLE[N]
    M = len(phases)
    rng = np.random.default_rng(ref.ANALYTIC_SEED)
    t = np.arange(n * K, dtype=np.float64)
    src = np.exp(2j * np.pi * doa.sim.tone_frequencies(M)[:, None] * t[None, :])
    noise = (rng.standard_normal((N, n * K)) + 1j * rng.standard_normal((N, n * K))) * np.sqrt(ref.SIGMA2 / 2.0)
    x = (np.exp(1j * np.outer(np.arange(N), phases)) @ src + noise).astype(np.complex64)
    dev = doa.sim.stream_slab_torch([_dev(a) for a in x])
    pipe = doa.root_pipeline(N, K, 0, 0, ref.D, M, max_batch=n)
    pipe.set_estimator("esprit")
    cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
    ang = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert pipe.work_dev(n, [a.data_ptr() for a in dev], cov.data_ptr(), ang.data_ptr(), st.data_ptr(),
                         torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    R, ang, st = cov.cpu().numpy(), ang.cpu().numpy(), st.cpu().numpy()
    _compare_with_the_definition("pipeline, out of visible N=8 M=3", N, M, R, nan_counts=(1,))
    b_ang, b_st = _block(N, M, R)
    assert _same(ang, b_ang) and np.array_equal(st, b_st)
    assert np.isnan(ang[:, -1]).all() and not np.isnan(ang[:, :-1]).any()
