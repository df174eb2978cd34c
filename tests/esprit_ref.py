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
"""
import functools

import numpy as np

import doa
import doa_oracle as oracle
from capon_ref import hermitian_from_upper

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
