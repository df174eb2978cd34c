"""numpy restatement of the Capon (MVDR) spectrum of doa.capon_lin_array / music_pipeline.set_estimator("capon")
(include/doa_hip.h), for its tests, and the scenario table they share (importable like spatial_smooth_ref.py).
Not a block of the reference: the definition is this project's, stated once in the header and written out here.

Input item: column-major N x N complex64, only the upper triangle read, of the diagonal the real part: H = the Hermitian
matrix these define.  In complex128:

    mu  = (sum_i H[i,i]) / N
    A   = H / mu + delta I
    W   = A^-1                              (np.linalg.inv; the literal Cholesky below gives the pivots and the status)
    Q_i = Re(a_i^H W a_i);  out = 1 / Q;  spectrum = 10 log10(out / max out)          (the fp64 oracle's formulas)
    status 1: mu > 0 does not hold, a Cholesky pivot s_j fails s_j > 2^-44 A[j,j], or anything is not finite
              -> an all-NaN row
"""
import functools

import numpy as np

import doa
import doa_oracle as oracle

PIVOT_MIN = 2.0 ** -44
P = 1024
SEED = 3
N_ITEMS = 8

# (N, thetas, SNR dB, K, delta, d): every kernel form, every padded scan size, the rank-deficient use case (row 4)
TABLE = (
    (4, (30.0, 123.0), 20.0, 1024, 0.0, 0.4),
    (4, (30.0, 123.0), 20.0, 1024, 1e-3, 0.4),
    (8, (60.0, 75.0, 120.0), 10.0, 256, 0.0, 0.5),
    (16, (40.0, 90.0, 100.0), 20.0, 64, 0.0, 0.5),
    (16, (40.0, 90.0, 100.0), 20.0, 8, 1e-2, 0.5),
    (3, (70.0,), 40.0, 32, 0.0, 0.5),
    (2, (70.0,), 40.0, 32, 0.0, 0.5),
    (5, (50.0, 100.0), 30.0, 64, 0.0, 0.5),
    (11, (50.0, 100.0), 30.0, 64, 0.0, 0.5),
)
RANK_DEFICIENT_ROW = 4


def hermitian_from_upper(item, N):
    """The N x N complex128 Hermitian matrix an item's upper triangle defines (diagonal: real parts)."""
    A = np.asarray(item).reshape(N, N, order="F").astype(np.complex128)
    U = np.triu(A, 1)
    return U + U.conj().T + np.diag(A.diagonal().real)


def loaded(item, N, delta):
    """(A, mu) of one item."""
    H = hermitian_from_upper(item, N)
    mu = H.diagonal().real.sum() / N
    with np.errstate(all="ignore"):
        return H / mu + float(delta) * np.eye(N), mu


def cholesky(A):
    """The literal Cholesky A = L L^H, column by column: (L, pivots s_j); nothing is checked here."""
    N = A.shape[0]
    L = np.zeros((N, N), np.complex128)
    s = np.zeros(N)
    with np.errstate(all="ignore"):
        for j in range(N):
            s[j] = A[j, j].real - np.sum(np.abs(L[j, :j]) ** 2)
            L[j, j] = np.sqrt(s[j])
            for i in range(j + 1, N):
                L[i, j] = (A[i, j] - np.sum(L[i, :j] * np.conj(L[j, :j]))) / L[j, j]
    return L, s


def inverse_cholesky(A):
    """W = L^-H L^-1 from the literal Cholesky, by forward substitution."""
    N = A.shape[0]
    L, _ = cholesky(A)
    M = np.zeros((N, N), np.complex128)
    for j in range(N):
        M[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, N):
            M[i, j] = -np.sum(L[i, j:i] * M[j:i, j]) / L[i, i]
    return M.conj().T @ M


def status(item, N, delta):
    A, mu = loaded(item, N, delta)
    if not (mu > 0) or not np.all(np.isfinite(A)):
        return 1
    _, s = cholesky(A)
    if not np.all(np.isfinite(s)) or not np.all(s > PIVOT_MIN * A.diagonal().real):
        return 1
    return 0


def capon(R_items, d, N, P_len, delta):
    """(spectrum [n, P] float64 dB, Q [n, P] float64, W [n, N, N] complex128, status [n] int32); status-1 items are NaN."""
    R_items = np.asarray(R_items).reshape(-1, N * N)
    n = R_items.shape[0]
    steer = oracle.music_steering(d, N, P_len, "f64")
    spec, q = np.full((n, P_len), np.nan), np.full((n, P_len), np.nan)
    W = np.full((n, N, N), np.nan + 0j)
    st = np.zeros(n, np.int32)
    for i in range(n):
        st[i] = status(R_items[i], N, delta)
        if st[i]:
            continue
        A, _ = loaded(R_items[i], N, delta)
        W[i] = np.linalg.inv(A)
        q[i] = oracle.music_null_spectrum(W[i], steer)
        spec[i] = oracle.music_db_from_q(q[i], "f64")
    return spec, q, W, st


def condition_numbers(R_items, N, delta):
    return np.array([np.linalg.cond(loaded(it, N, delta)[0]) for it in np.asarray(R_items).reshape(-1, N * N)])


@functools.lru_cache(maxsize=None)
def streams(N, thetas, snr_db, K, d, n_items=N_ITEMS):
    x = doa.sim.make_streams(N, n_items * K, list(thetas), d, snr_db=snr_db, seed=SEED)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def covariance(N, thetas, snr_db, K, d, n_items=N_ITEMS):
    """[n_items, N*N] complex64 (oracle.autocorrelate, overlap 0, avg_method 0), read-only."""
    R = oracle.autocorrelate(streams(N, thetas, snr_db, K, d, n_items), K, 0, 0, n_items)
    R.setflags(write=False)
    return R


def row_covariance(row, n_items=N_ITEMS):
    N, thetas, snr_db, K, delta, d = TABLE[row]
    return covariance(N, thetas, snr_db, K, d, n_items)


def angle_error(locs, thetas):
    """max over items of the largest |estimate - truth| after sorting both ([n, M] estimates in any order)."""
    return float(np.abs(np.sort(np.asarray(locs, np.float64), axis=1) - np.sort(np.asarray(thetas))[None, :]).max())
