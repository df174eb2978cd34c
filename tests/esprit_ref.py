"""numpy restatement of LS-ESPRIT as doa.esprit_linear_array / root_pipeline.set_estimator("esprit") define it
(include/doa_hip.h), for its tests, and the scenario table they share (importable like capon_ref.py).
Not a block of the reference: the definition is this project's, stated once in the header and written out here.

Input item: column-major N x N complex64, only the upper triangle read, of the diagonal the real part: H = the Hermitian
matrix these define.  In complex128, d = float64(float32(norm_spacing)):

    (w, V) = eigh(H), ascending (ties: lower index first, the eig_sym rule)
    Es     = the eigenvectors of the M largest eigenvalues              (N x M, orthonormal)
    Es1    = rows 0 .. N-2,   Es2 = rows 1 .. N-1
    gamma  = 1 - sum_k |Es[N-1, k]|^2                                   (the smallest eigenvalue of Es1^H Es1)
    Psi    = (Es1^H Es1)^-1 Es1^H Es2                                   (M x M)
    c_k    = arg(eigenvalue_k of Psi) / (2 pi d)
    angle_k = float32(180 / pi * acos(c_k)), NaN when |c_k| > 1;  the M angles sorted ascending, NaN last
    status 1: trace(H) > 0 does not hold, an entry is not finite, or gamma > 2^-30 does not hold -> an all-NaN row
    status 2 (counts entries): the item's count lies outside 0 .. min(W, N-1); count 0: all NaN, status 0

For the solver tests (tests/test_gpu_esprit_solver.py) the same definition applied to a GIVEN orthonormal Es
(esprit_from_record), with the predicted sensitivity of every angle and the gate derived from it (comparable), and the
inputs of those tests: random_records / pack_records (signal-subspace records, gr-doa_amd/csrc/kernels.hpp) and
analytic_covariance.
"""
import functools

import numpy as np

import doa
import doa_oracle as oracle
from capon_ref import hermitian_from_upper           # (the tests use it through this module too)

GAMMA_MIN = 2.0 ** -30
SEED = 11
D = 0.4
K = 256
N_ITEMS = 67               # a partial wave at every group width (16, 8 and 4 items per wave)

# (N, M) -> source directions in degrees, all within 25 .. 155
ANGLES = {
    (2, 1): (70.0,), (3, 1): (70.0,), (3, 2): (50.0, 110.0), (4, 1): (70.0,), (4, 2): (30.0, 123.0),
    (4, 3): (40.0, 85.0, 130.0), (5, 2): (50.0, 100.0), (5, 4): (35.0, 70.0, 105.0, 140.0), (8, 1): (70.0,),
    (8, 3): (60.0, 75.0, 120.0), (8, 7): (30.0, 48.0, 66.0, 84.0, 102.0, 120.0, 140.0), (9, 4): (40.0, 70.0, 100.0, 130.0),
    (16, 1): (70.0,), (16, 3): (40.0, 42.5, 120.0),
    (16, 15): tuple(25.0 + 9.25 * i for i in range(15)),       # the widest even spread: gamma ~ 2e-4, eigen-gap ~ 1e-3
}
# every shape at 20 dB and at 5 dB, (16, 15) at 20 dB only (at 5 dB the definition itself yields NaN angles there)
CASES = tuple((N, M, snr) for (N, M) in ANGLES for snr in (20.0, 5.0) if not ((N, M) == (16, 15) and snr == 5.0))


def signal_subspace(H, M):
    """(Es [N, M], w ascending) of a Hermitian matrix; Es columns by descending eigenvalue."""
    w, V = np.linalg.eigh(H)
    N = H.shape[0]
    return V[:, [N - 1 - k for k in range(M)]], w


def esprit_item(item, d, M, N):
    """(angles [M] float32 sorted NaN last, status, gamma, relative signal-to-noise eigen-gap) of one item."""
    nan_row = np.full(M, np.nan, np.float32)
    H = hermitian_from_upper(item, N)
    if not np.all(np.isfinite(H)) or not (H.diagonal().real.sum() > 0):
        return nan_row, 1, np.nan, np.nan
    Es, w = signal_subspace(H, M)
    gap = (w[N - M] - w[N - M - 1]) / w[N - 1]
    gamma = 1.0 - float(np.sum(np.abs(Es[N - 1, :]) ** 2))
    if not (gamma > GAMMA_MIN):
        return nan_row, 1, gamma, gap
    Es1, Es2 = Es[:-1, :], Es[1:, :]
    Psi = np.linalg.solve(Es1.conj().T @ Es1, Es1.conj().T @ Es2)
    lam = np.linalg.eigvals(Psi)
    c = np.arctan2(lam.imag, lam.real) / (2.0 * np.pi * float(np.float32(d)))
    with np.errstate(invalid="ignore"):
        ang = (180.0 / np.pi * np.arccos(c)).astype(np.float32)
    return np.sort(ang), 0, gamma, gap


def esprit(R_items, d, M, N):
    """(angles [n, M] float32, status [n] int32, gamma [n], gap [n]) of doa.esprit_linear_array(d, M, N)."""
    R_items = np.asarray(R_items).reshape(-1, N * N)
    n = R_items.shape[0]
    ang = np.empty((n, M), np.float32)
    st = np.zeros(n, np.int32)
    gamma, gap = np.empty(n), np.empty(n)
    for i in range(n):
        ang[i], st[i], gamma[i], gap[i] = esprit_item(R_items[i], d, M, N)
    return ang, st, gamma, gap


def esprit_counts(R_items, counts, d, W, N):
    """(angles [n, W], status [n]) of the counts entries."""
    R_items = np.asarray(R_items).reshape(-1, N * N)
    n = R_items.shape[0]
    ang = np.full((n, W), np.nan, np.float32)
    st = np.zeros(n, np.int32)
    for i, m in enumerate(np.asarray(counts).astype(int)):
        if m < 0 or m > min(W, N - 1):
            st[i] = 2
        elif m > 0:
            a, st[i], _, _ = esprit_item(R_items[i], d, m, N)
            if st[i] == 0:
                ang[i, :m] = a
    return ang, st


@functools.lru_cache(maxsize=None)
def covariance(N, thetas, snr_db, k=K, d=D, n_items=N_ITEMS, seed=SEED):
    """[n_items, N*N] complex64 (oracle.autocorrelate, overlap 0, avg_method 0), read-only."""
    x = doa.sim.make_streams(N, n_items * k, list(thetas), d, snr_db=snr_db, seed=seed)
    R = oracle.autocorrelate(x, k, 0, 0, n_items)
    R.setflags(write=False)
    return R


def case_covariance(N, M, snr_db):
    return covariance(N, ANGLES[(N, M)], snr_db)


def failure_items(N, good):
    """(singular: gamma = 0 exactly for one source, zero, NaN, Inf) items of size N; `good` supplies the finite entries."""
    sing = np.diag([1.0] * (N - 1) + [5.0]).astype(np.complex64).reshape(-1)
    zero = np.zeros(N * N, np.complex64)
    one_nan = np.array(good); one_nan[0 + (N - 1) * N] = np.nan        # upper triangle: row 0, last column
    one_inf = np.array(good); one_inf[1 + 1 * N] = np.inf              # on the diagonal
    return [sing, zero, one_nan, one_inf]


# ---- the solver on given subspace records ----------------------------------------------------------------------------------
AMP_MAX = 1e8              # degrees per unit relative perturbation: 1e8 * 2^-52 = 2.2e-8 deg, 4.5e4 below the 1e-3 deg bound
EDGE_MIN = 1e-6            # | |c| - 1 | below this: whether the angle is NaN is not decided by the definition in double
RECORD_SEED = 29
N_RECORDS = 403            # 25 waves of 16 items + 3, 50 of 8 + 3, 100 of 4 + 3: a partial wave at every group width
RECORD_SHAPES = ((3, 2), (4, 3), (5, 3), (6, 3), (8, 7), (9, 8), (12, 5), (16, 8), (16, 15))
NONCOMPARABLE_CAP = 0.05


def esprit_from_record(Es, d, m):
    """The definition on a given orthonormal Es (N x >= m complex128, the first m columns taken):
    (angles [m] float32 sorted NaN last, status 0 / 1, gamma, c [m], amp [m]); c_k and amp_k in the order of eigvals, where
        amp_k = kappa_k ||Psi||_2 / |lambda_k| / (2 pi d sqrt(|1 - c_k^2|)) * (180 / pi) / gamma
    is the predicted change of angle k in degrees per unit relative perturbation of Es: kappa_k = ||x_k|| ||y_k|| the
    condition number of the eigenvalue (x_k the right eigenvector, y_k the row of inv(V)), / |lambda_k| from d arg(lambda),
    / (2 pi d) to c, / sqrt(|1 - c^2|) through acos, 1 / gamma from forming Psi.  Status 1: c and amp are NaN."""
    Es = np.asarray(Es, np.complex128)[:, :m]
    N = Es.shape[0]
    nan = np.full(m, np.nan)
    gamma = 1.0 - float(np.sum(np.abs(Es[N - 1, :]) ** 2))
    if not (gamma > GAMMA_MIN):
        return nan.astype(np.float32), 1, gamma, nan, nan
    Es1, Es2 = Es[:-1, :], Es[1:, :]
    Psi = np.linalg.solve(Es1.conj().T @ Es1, Es1.conj().T @ Es2)
    lam, V = np.linalg.eig(Psi)
    d64 = float(np.float32(d))
    c = np.arctan2(lam.imag, lam.real) / (2.0 * np.pi * d64)
    with np.errstate(all="ignore"):
        ang = (180.0 / np.pi * np.arccos(c)).astype(np.float32)
        try:
            kappa = np.linalg.norm(V, axis=0) * np.linalg.norm(np.linalg.inv(V), axis=1)
        except np.linalg.LinAlgError:                      # a defective Psi: no finite sensitivity
            kappa = np.full(m, np.inf)
        amp = kappa * np.linalg.norm(Psi, 2) / np.abs(lam) / (2.0 * np.pi * d64 * np.sqrt(np.abs(1.0 - c * c))) \
            * (180.0 / np.pi) / gamma
    amp = np.where(np.isnan(amp), np.inf, amp)
    return np.sort(ang), 0, gamma, c, amp


def comparable(c, amp):
    """The gate of the solver tests: every eigenvalue has amp <= 1e8 and | |c| - 1 | >= 1e-6."""
    return bool(np.all(amp <= AMP_MAX) and np.all(np.abs(np.abs(c) - 1.0) >= EDGE_MIN))


def pack_records(Es, N):
    """[n, 2 N^2] float64 records (kernels.hpp: [2 (k N + row)] = Re Es[row][k], + 1 = Im) from Es [n, N, m]; the columns
    m .. N-1, which the kernel may not read, are NaN."""
    Es = np.asarray(Es, np.complex128)
    n, _, m = Es.shape
    rec = np.full((n, N, N), np.nan + 1j * np.nan, np.complex128)          # [item][k][row]
    rec[:, :m, :] = Es.transpose(0, 2, 1)
    return np.ascontiguousarray(rec).view(np.float64).reshape(n, 2 * N * N)


@functools.lru_cache(maxsize=None)
def random_records(N, m, n=N_RECORDS, seed=RECORD_SEED):
    """(Es [n, N, m] complex128 orthonormal: the Q of the QR factorisation of complex Gaussian matrices, records
    [n, 2 N^2]), read-only."""
    rng = np.random.default_rng([seed, N, m])
    A = rng.standard_normal((n, N, m)) + 1j * rng.standard_normal((n, N, m))
    Es = np.stack([np.linalg.qr(a)[0] for a in A])
    rec = pack_records(Es, N)
    Es.setflags(write=False); rec.setflags(write=False)
    return Es, rec


@functools.lru_cache(maxsize=None)
def record_reference(N, m, d=D, n=N_RECORDS, seed=RECORD_SEED):
    """(angles [n, m] float32, status [n], gamma [n], c [n, m], amp [n, m], comparable [n] bool) of random_records(N, m)."""
    Es, _ = random_records(N, m, n, seed)
    ang, c, amp = np.empty((n, m), np.float32), np.empty((n, m)), np.empty((n, m))
    st, gamma, ok = np.zeros(n, np.int32), np.empty(n), np.zeros(n, bool)
    for i in range(n):
        ang[i], st[i], gamma[i], c[i], amp[i] = esprit_from_record(Es[i], d, m)
        ok[i] = st[i] == 0 and comparable(c[i], amp[i])
    for a in (ang, st, gamma, c, amp, ok):
        a.setflags(write=False)
    return ang, st, gamma, c, amp, ok


def identity_items(n, N):
    """[n, N*N] complex64 identity items: a positive trace, finite; all the record entry reads of them."""
    return np.tile(np.eye(N, dtype=np.complex64).reshape(-1), (n, 1))


def analytic_covariance(N, phases, powers, sigma2):
    """One item [N*N] complex64, column-major: A P A^H + sigma2 I with a_n = exp(i n phase), rounded to complex64."""
    A = np.exp(1j * np.outer(np.arange(N), np.asarray(phases, np.float64)))
    R = (A * np.asarray(powers, np.float64)[None, :]) @ A.conj().T + float(sigma2) * np.eye(N)
    return R.astype(np.complex64).reshape(-1, order="F")


def phases_of(thetas_deg, d=D):
    """The per-element phases 2 pi d cos(theta) of sources at the given directions (doa.sim.manifold's convention)."""
    return 2.0 * np.pi * float(np.float32(d)) * np.cos(np.deg2rad(np.asarray(thetas_deg, np.float64)))


# ---- analytic covariances for the public block ------------------------------------------------------------------------------
ANALYTIC_SEED = 31
ANALYTIC_ITEMS = 19        # a partial wave at every group width
SIGMA2 = 0.01
# N -> per-element phases with components outside the visible region: at d = 0.4 a phase of 0.9 pi is c = 1.125
OUT_OF_VISIBLE = {
    4: (0.9 * np.pi, 0.3 * np.pi),
    8: (0.9 * np.pi, -0.5 * np.pi, 0.1 * np.pi),
    16: (-0.95 * np.pi, 0.9 * np.pi, 0.2 * np.pi, 0.25 * np.pi),
}


def spread_angles(M):
    """M directions evenly spread over 25 .. 155 degrees (70 for one)."""
    return (70.0,) if M == 1 else tuple(np.linspace(25.0, 155.0, M))


def _read_only(R):
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def spread_items(N, M, d=D, thetas=None):
    """[19, N*N] analytic items: sources at spread_angles(M) (or thetas), powers drawn from U(0.5, 2), sigma2 = 0.01."""
    th = spread_angles(M) if thetas is None else thetas
    powers = np.random.default_rng([ANALYTIC_SEED, N, M]).uniform(0.5, 2.0, (ANALYTIC_ITEMS, M))
    return _read_only(np.stack([analytic_covariance(N, phases_of(th, d), p, SIGMA2) for p in powers]))


@functools.lru_cache(maxsize=None)
def out_of_visible_items(N):
    """[19, N*N] analytic items of OUT_OF_VISIBLE[N]: powers 1 .. M in item 0, all of them times one factor from U(1, 2) in
    each of the others (a higher signal-to-noise ratio keeps the eigen-gap of item 0)."""
    ph = OUT_OF_VISIBLE[N]
    scale = np.random.default_rng([ANALYTIC_SEED, N]).uniform(1.0, 2.0, ANALYTIC_ITEMS)
    scale[0] = 1.0
    return _read_only(np.stack([analytic_covariance(N, ph, np.arange(1.0, len(ph) + 1.0) * s, SIGMA2) for s in scale]))


@functools.lru_cache(maxsize=None)
def dft_grid_items(N=8, M=4):
    """[19, N*N]: equal-power sources at phases 2 pi k / N, k = 0 .. M-1 (orthogonal steering vectors: the signal eigenvalues
    tie), the one item at 19 power-of-two scales."""
    item = analytic_covariance(N, 2.0 * np.pi * np.arange(M) / N, np.ones(M), SIGMA2)
    return _read_only(np.stack([item * np.float32(2.0 ** (k - 9)) for k in range(ANALYTIC_ITEMS)]).astype(np.complex64))


def esprit_gated(R_items, d, M, N):
    """esprit() and, per item, the largest amp and the smallest | |c| - 1 | of esprit_from_record on the item's own signal
    subspace: (angles, status, gamma, gap, amp_max [n], edge_min [n])."""
    R_items = np.asarray(R_items).reshape(-1, N * N)
    ang, st, gamma, gap = esprit(R_items, d, M, N)
    amp_max, edge_min = np.full(len(R_items), np.inf), np.zeros(len(R_items))
    for i, item in enumerate(R_items):
        if st[i] == 0:
            _, _, _, c, amp = esprit_from_record(signal_subspace(hermitian_from_upper(item, N), M)[0], d, M)
            amp_max[i], edge_min[i] = amp.max(), np.abs(np.abs(c) - 1.0).min()
    return ang, st, gamma, gap, amp_max, edge_min
