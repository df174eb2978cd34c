"""numpy restatement of the iterative adaptive (IAA) power spectrum of doa.iaa_lin_array (include/doa_hip.h), for its
tests, and the scenario table they share (importable like capon_ref.py).  Not a block of the reference: the definition is
this project's, stated once in the header and written out here.

Input item: column-major N x N complex64, only the upper triangle read, of the diagonal the real part: H = the Hermitian
matrix these define.  a_k = column k of oracle.music_steering(d, N, P, "f64").  In complex128:

    mu   = (sum_i H[i,i]) / N ;  Hn = H / mu
    p_k  = Re(a_k^H Hn a_k) / N^2
    repeat L = iterations times:
        R   = sum_k p_k a_k a_k^H + delta I
        W   = R^-1                     (np.linalg.inv; the literal Cholesky of capon_ref gives the pivots and the status)
        B   = W Hn W
        g_k = Re(a_k^H W a_k) ;  n_k = max(Re(a_k^H B a_k), 0)
        p_k = n_k / g_k^2
    spectrum row = 10 log10(p / max p), from out = float32(p) and the float32 quotient out / max out
    power row    = mu p_k
    status 1: mu > 0 does not hold, a Cholesky pivot of any iteration fails s_j > 2^-44 R[j,j], or anything is not finite
              -> both rows all NaN
"""
import functools

import numpy as np

import doa
import doa_oracle as oracle
import capon_ref
import spatial_smooth_ref as ssref

PIVOT_MIN = capon_ref.PIVOT_MIN
MAX_PSPECTRUM_LEN = 4096
MAX_ITERATIONS = 32
DEFAULT_ITERATIONS = 10
SEED = 3


def db_row(p):
    """The spectrum row of p [P] float64: float32 out, float32 quotient, 0 dB exactly at the largest rounded value (the
    logarithm itself in double)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.asarray(p, np.float64).astype(np.float32)
        q = (out / out.max()).astype(np.float32)
        return 10.0 * np.log10(q.astype(np.float64))


def _pivots(R):
    """The Cholesky pivots s_j = L[j,j]^2 of R (LAPACK's factorisation forms the same differences as the literal loop of
    capon_ref.cholesky, without the Python loop), or None where it stops at a pivot that is not positive."""
    try:
        return np.linalg.cholesky(R).diagonal().real ** 2
    except np.linalg.LinAlgError:
        return None


def _quad(Ac, X, steer):
    """Re(a_k^H X a_k) for every k."""
    return np.sum(Ac * (X @ steer), axis=0).real


def iaa_item(item, steer, N, delta, iterations, perturb=None):
    """One item: (list of the iterates (p [P] float64, lags [N] complex128 of the R it came from), one per iteration, or
    None; mu; status; largest condition number of an iterate's R).  perturb: optional callable applied to every iterate p
    before it is used (the sensitivity study of the tests)."""
    H = capon_ref.hermitian_from_upper(item, N)
    mu = H.diagonal().real.sum() / N
    if not (mu > 0) or not np.all(np.isfinite(H)):
        return None, mu, 1, np.inf
    Hn = H / mu
    Ac = steer.conj()
    p = _quad(Ac, Hn, steer) / N ** 2
    w_pow = steer * Ac[0][None, :]                       # row l: w_k^l = a_k[l] conj(a_k[0])
    cond, hist = 0.0, []
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            if perturb is not None:
                p = perturb(p)
            R = (steer * p[None, :]) @ Ac.T + float(np.float32(delta)) * np.eye(N)     # delta is a float argument of create
            lags = w_pow @ p
            if not np.all(np.isfinite(R)):
                return None, mu, 1, np.inf
            s = _pivots(R)
            if s is None or not np.all(np.isfinite(s)) or not np.all(s > PIVOT_MIN * R.diagonal().real):
                return None, mu, 1, np.inf
            cond = max(cond, float(np.linalg.cond(R)))
            W = np.linalg.inv(R)
            B = W @ Hn @ W
            g = _quad(Ac, W, steer)
            nn = np.maximum(_quad(Ac, B, steer), 0.0)
            p = nn / g ** 2
            hist.append((p, lags))
    if not np.all(np.isfinite(p)):
        return None, mu, 1, cond
    return hist, mu, 0, cond


def iaa(R_items, d, N, P_len, delta=0.0, iterations=DEFAULT_ITERATIONS, perturb=None, every=False):
    """dict of spectrum [n, P] float64 dB, p [n, P] float64, power [n, P] float64 (= mu p), lags [n, N] complex128 (of the
    last iteration's R), mu [n], status [n] int32, cond [n] (the largest condition number of any iterate's R); status-1
    items are NaN.  every: also p_all [n, L, P] and lags_all [n, L, N], the same after each iteration 1..L (one run serves
    every smaller iteration count of the items whose status is 0)."""
    R_items = np.asarray(R_items).reshape(-1, N * N)
    n, L = R_items.shape[0], iterations
    steer = oracle.music_steering(d, N, P_len, "f64")
    out = dict(spectrum=np.full((n, P_len), np.nan), p=np.full((n, P_len), np.nan), power=np.full((n, P_len), np.nan),
               lags=np.full((n, N), np.nan + 0j), mu=np.zeros(n), status=np.zeros(n, np.int32), cond=np.zeros(n))
    if every:
        out["p_all"], out["lags_all"] = np.full((n, L, P_len), np.nan), np.full((n, L, N), np.nan + 0j)
    for i in range(n):
        hist, mu, st, cond = iaa_item(R_items[i], steer, N, delta, L, perturb)
        out["status"][i], out["cond"][i], out["mu"][i] = st, cond, mu
        if st:
            continue
        p, lags = hist[-1]
        out["p"][i], out["power"][i], out["lags"][i], out["spectrum"][i] = p, mu * p, lags, db_row(p)
        if every:
            for t in range(L):
                out["p_all"][i, t], out["lags_all"][i, t] = hist[t]
    return out


def peaks(spectrum, M, P_len):
    """(values, locations in degrees) [n, M] of the M largest local maxima of each row (oracle.find_local_max)."""
    return oracle.find_local_max(np.asarray(spectrum, np.float32), M, P_len, 0.0, 180.0)


def power_at_peaks(power, locs, P_len):
    """power [n, P] at the grid cells of locs [n, M] degrees, columns sorted by angle."""
    idx = np.rint(np.sort(np.asarray(locs, np.float64), axis=1) * P_len / 180.0).astype(int)
    return np.take_along_axis(np.asarray(power), np.clip(idx, 0, P_len - 1), axis=1)


angle_error = capon_ref.angle_error


# ---- the item sets ---------------------------------------------------------------------------------------------------
# the block test: 67 items per array size from capon_ref's generators (a partial wave of items at the end), unread parts spoiled
ROW_OF_N = {4: 0, 8: 2, 16: 3, 3: 5, 2: 6, 5: 7, 11: 8}
N_BLOCK = 67
# (N, P): every array size class at P = 256, the two long grids, a grid that is no multiple of 64 and one shorter than a wave
BLOCK_CASES = tuple((N, 256) for N in (2, 3, 4, 5, 8, 11, 16)) + ((4, 1024), (16, 4096), (8, 1001), (3, 37))
BLOCK_DELTAS = (0.0, 1e-2)
BLOCK_ITERATIONS = (1, 2, 10)


def spoil_unread_parts(R, N):
    """Strict lower triangle NaN, imaginary part of the diagonal 7.0: neither may be read."""
    R = np.array(R).reshape(-1, N, N)                       # [item][col][row]
    for col in range(N):
        R[:, col, col + 1:] = np.nan + 1j * np.nan
        R[:, col, col] = R[:, col, col].real + 7.0j
    return R.reshape(-1, N * N)


def block_spacing(N):
    return capon_ref.TABLE[ROW_OF_N[N]][5]


@functools.lru_cache(maxsize=None)
def block_items(N):
    n_, thetas, snr_db, K, delta, d = capon_ref.TABLE[ROW_OF_N[N]]
    R = spoil_unread_parts(capon_ref.covariance(N, thetas, snr_db, K, d, N_BLOCK), N)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def block_reference(N, P_len, delta):
    """One run of max(BLOCK_ITERATIONS) iterations with every iterate kept."""
    return iaa(block_items(N), block_spacing(N), N, P_len, delta, max(BLOCK_ITERATIONS), every=True)


@functools.lru_cache(maxsize=None)
def wishart(N, n, seed):
    """n well-conditioned random covariance items X X^H / 4N (X: N x 4N complex normal), unread parts spoiled."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, N, 4 * N)) + 1j * rng.standard_normal((n, N, 4 * N))
    H = X @ X.conj().transpose(0, 2, 1) / (4 * N)                         # [item][row][col]
    R = spoil_unread_parts(H.transpose(0, 2, 1).reshape(n, N * N).astype(np.complex64), N)
    R.setflags(write=False)
    return R


BAD_AT = (1, 9, 30, 63, 65)


def bad_items(N, good):
    """Capon's five: all ones (singular), zero, minus the identity, one NaN in the upper triangle, one Inf on the diagonal."""
    ones = np.ones(N * N, np.complex64)
    zero = np.zeros(N * N, np.complex64)
    minus_eye = -np.eye(N, dtype=np.complex64).reshape(-1)
    one_nan = np.array(good); one_nan[0 + (N - 1) * N] = np.nan
    one_inf = np.array(good); one_inf[1 + 1 * N] = np.inf
    return [ones, zero, minus_eye, one_nan, one_inf]


# rank-one items: one snapshot each, autocorrelate(x, 1, 0, 0, 16) of 16 samples; name: (N, thetas, SNR dB, d)
K1_SETS = {
    "k1_n8": (8, (60.0, 100.0), 25.0, 0.5),
    "k1_n16": (16, (40.0, 90.0, 100.0), 25.0, 0.5),
}
K1_ITEMS = 16
K1_P = 1024


@functools.lru_cache(maxsize=None)
def k1_covariance(name):
    """[16, N*N] complex64 items of rank one, read-only."""
    N, thetas, snr_db, d = K1_SETS[name]
    x = doa.sim.make_streams(N, K1_ITEMS, list(thetas), d, snr_db=snr_db, seed=SEED)
    R = oracle.autocorrelate(x, 1, 0, 0, K1_ITEMS)
    R.setflags(write=False)
    return R


# two incoherent tones 30 dB apart: amplitudes 1 and 10^-1.5 on 8 elements, noise 40 dB under the strong one
PAIR = dict(N=8, thetas=(60.0, 100.0), amps=(1.0, 10.0 ** -1.5), snr_db=40.0, K=256, n=8, d=0.5, P=1024)


@functools.lru_cache(maxsize=None)
def pair_covariance():
    c = PAIR
    rng = np.random.default_rng(SEED)
    T = c["n"] * c["K"]
    A = doa.sim.manifold(c["d"], c["N"], c["thetas"])
    t = np.arange(T, dtype=np.float64)
    src = np.exp(2j * np.pi * doa.sim.tone_frequencies(2)[:, None] * t[None, :]) * np.asarray(c["amps"])[:, None]
    sigma = 10.0 ** (-c["snr_db"] / 20.0)
    w = (rng.standard_normal((c["N"], T)) + 1j * rng.standard_normal((c["N"], T))) / np.sqrt(2.0)
    x = np.ascontiguousarray((A @ src + sigma * w).astype(np.complex64))
    R = oracle.autocorrelate(x, c["K"], 0, 0, c["n"])
    R.setflags(write=False)
    return R


def coherent_truth(name):
    """(N, thetas, true powers |rho|^2) of a coherent scenario of spatial_smooth_ref."""
    N, S, fb, th, rho = ssref.SCENARIOS[name]
    return N, th, tuple(abs(r) ** 2 for r in rho)
