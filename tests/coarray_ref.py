"""The definition of doa.coarray_covariance and doa.coarray_lags (include/doa_hip.h), restated in numpy for the tests, with the
signal model of a sparse linear array and the scenario table.  Not a block of the reference: the definition is this project's.

positions[n] is the position of stream n in units of the element spacing, counted as MUSIC_lin_array numbers its elements
(element n of its uniform array is position n).  lag(a, b) = positions[a] - positions[b]; c_l = the number of ordered pairs
with lag l; Lc = the largest L such that every lag 0 .. L-1 occurs; Lv = virtual_size, 0 meaning min(Lc, 16).

Input item: column-major N x N complex64, only the upper triangle read, of the diagonal the real part: H = the Hermitian
matrix these define.  Output item: column-major Lv x Lv complex64, full, exactly Hermitian.

    for l = 0 .. Lv-1:
      s[l] = sum (double) H[a,b] over the pairs with lag(a,b) = l,
             ascending column b, then ascending row a; re and im separately; l = 0: real parts only
      r[l] = s[l] * (1.0 / c_l)           (1.0 / c_l formed in double; r stays in double)
    T[i,j] = r[i-j] for i >= j, conj(r[j-i]) for i < j          (row i, column j)

    mode "toeplitz":  out[i,j] = (float) T[i,j]
    mode "smoothed":  out[i,j] = (float)( (sum_k T[i,k] conj(T[j,k])) * (1.0 / Lv) ),  i <= j, in double; mirror conjugated
    Im out[i,i] = +0.0;  out[j,i] = conj(out[i,j])

In "toeplitz" mode no product feeds an addition, so a device that does these operations in this order is bit-identical.
"""
import functools

import numpy as np

import doa_oracle as oracle
import wideband_ref as wb

MAX_ANT_ELE = 16


def lags(positions):
    """(Lc, counts[Lc]): the contiguous size of the difference co-array and c_l for l < Lc."""
    p = [int(v) for v in positions]
    count = {}
    for a in p:
        for b in p:
            count[a - b] = count.get(a - b, 0) + 1
    Lc = 0
    while Lc in count:
        Lc += 1
    return Lc, [count[l] for l in range(Lc)]


def default_size(positions):
    return min(lags(positions)[0], MAX_ANT_ELE)


def pairs_of_lag(positions, l):
    """The (a, b) with lag(a, b) = l in the definition's order: ascending column b, then ascending row a."""
    p = [int(v) for v in positions]
    N = len(p)
    return [(a, b) for b in range(N) for a in range(N) if p[a] - p[b] == l]


def toeplitz_of(r):
    """T [n, Lv, Lv] complex128 ([item][row][col]) from r [n, Lv]."""
    Lv = r.shape[1]
    i, j = np.indices((Lv, Lv))
    return np.where(i >= j, r[:, np.abs(i - j)], np.conj(r[:, np.abs(i - j)]))


def lag_means(items, positions, Lv):
    """r [n, Lv] complex128 of [n, N*N] complex64 items."""
    N = len(positions)
    R = np.asarray(items).reshape(-1, N, N)                      # [item][col][row]
    re, im = R.real.astype(np.float64), R.imag.astype(np.float64)
    n = R.shape[0]
    r = np.zeros((n, Lv), np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(Lv):
            pairs = pairs_of_lag(positions, l)
            sr, si = np.zeros(n), np.zeros(n)
            for a, b in pairs:
                if a <= b:                                       # H[a,b] is read where it stands
                    sr = sr + re[:, b, a]
                    if l:
                        si = si + im[:, b, a]
                else:                                            # H[a,b] = conj(H[b,a])
                    sr = sr + re[:, a, b]
                    if l:
                        si = si + (-im[:, a, b])
            inv = 1.0 / len(pairs)
            r[:, l] = sr * inv + 1j * (si * inv)
    return r


def coarray64(items, positions, virtual_size=0, mode="smoothed"):
    """The definition before its one rounding: [n, Lv*Lv] complex128 column-major items, exactly Hermitian."""
    Lv = virtual_size or default_size(positions)
    T = toeplitz_of(lag_means(items, positions, Lv))             # [item][row][col]
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "toeplitz":
            full = T
        else:
            full = np.einsum("nik,njk->nij", T, np.conj(T)) * (1.0 / Lv)
    i, j = np.indices((Lv, Lv))
    out = np.where(i <= j, full, np.conj(full.transpose(0, 2, 1)))          # [item][row][col]; the mirror conjugated
    d = np.arange(Lv)
    out[:, d, d] = out[:, d, d].real                             # Im out[i,i] = +0.0
    return out.transpose(0, 2, 1).reshape(-1, Lv * Lv)


def coarray_covariance(items, positions, virtual_size=0, mode="smoothed"):
    """[n, Lv*Lv] complex64: what the block writes (bit for bit in toeplitz mode).  Rounding to float commutes with the sign,
    so the rounded mirror is still the bitwise conjugate."""
    out64 = coarray64(items, positions, virtual_size, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.empty(out64.shape, np.complex64)
        out.real, out.imag = out64.real.astype(np.float32), out64.imag.astype(np.float32)
    return out


# ---- the signal model: x = A s + sigma w on a sparse linear array --------------------------------------------------------------
def manifold(positions, thetas_deg, d):
    """A[n, m] = exp(-2 pi j d cos(theta_m) (c - positions[n])), c the middle of the aperture (doa.sim.manifold's convention:
    the location falls as the position rises)."""
    p = np.asarray(positions, np.float64)
    c = 0.5 * (p.max() + p.min())
    th = np.deg2rad(np.asarray(thetas_deg, np.float64))
    return np.exp(-2j * np.pi * d * np.cos(th)[None, :] * (c - p)[:, None])


def make_streams(positions, thetas_deg, n_samples, d, snr_db, seed):
    """[N, n_samples] complex64: unit-power complex Gaussian sources, white noise snr_db below each."""
    rng = np.random.default_rng(seed)
    M, N = len(thetas_deg), len(positions)
    s = (rng.standard_normal((M, n_samples)) + 1j * rng.standard_normal((M, n_samples))) / np.sqrt(2.0)
    w = (rng.standard_normal((N, n_samples)) + 1j * rng.standard_normal((N, n_samples))) / np.sqrt(2.0)
    return np.ascontiguousarray((manifold(positions, thetas_deg, d) @ s + 10.0 ** (-snr_db / 20.0) * w).astype(np.complex64))


def exact_covariance(positions, thetas_deg, powers, sigma2, d):
    """[N, N] complex128: A diag(p) A^H + sigma2 I."""
    A = manifold(positions, thetas_deg, d)
    return (A * np.asarray(powers, np.float64)[None, :]) @ A.conj().T + sigma2 * np.eye(len(positions))


D, P_USE, SNR_DB, SEED, N_SNAP = 0.5, 2048, 10.0, 1, 16
MRA4, NESTED6 = (0, 1, 4, 6), (0, 1, 2, 3, 7, 11)
SCENARIOS = {
    "mra4_5": dict(positions=MRA4, thetas=[40.0, 65.0, 90.0, 115.0, 140.0], K=4096),
    "mra4_6": dict(positions=MRA4, thetas=[30.0, 55.0, 75.0, 100.0, 125.0, 150.0], K=8192),
    "nested6_8": dict(positions=NESTED6, thetas=[25.0, 45.0, 60.0, 75.0, 90.0, 105.0, 120.0, 140.0], K=4096),
}


@functools.lru_cache(maxsize=None)
def scenario_streams(name, seed=SEED):
    s = SCENARIOS[name]
    x = make_streams(s["positions"], s["thetas"], N_SNAP * s["K"], D, SNR_DB, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def scenario_items(name, seed=SEED):
    """[16, N*N] complex64 (oracle.autocorrelate, overlap 0, avg_method 0), read-only."""
    R = oracle.autocorrelate(scenario_streams(name, seed), SCENARIOS[name]["K"], 0, 0, N_SNAP)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def scenario_coarray(name, seed=SEED):
    """The reference's smoothed co-array items of a scenario, [16, Lv*Lv] complex64, read-only."""
    out = coarray_covariance(scenario_items(name, seed), SCENARIOS[name]["positions"])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scenario_music(name, seed=SEED):
    """[16, M] directions (degrees, ascending) of the float64 MUSIC spectrum of the reference's co-array items."""
    s = SCENARIOS[name]
    M, Lv = len(s["thetas"]), default_size(s["positions"])
    dB = oracle.music_lin_array(scenario_coarray(name, seed), D, M, Lv, P_USE, "f64")
    return wb.peaks(dB, M, P_USE)


def count_peaks(dB):
    """The number of interior local maxima (strictly above both neighbours) of every row."""
    dB = np.asarray(dB, np.float64)
    return ((dB[:, 1:-1] > dB[:, :-2]) & (dB[:, 1:-1] > dB[:, 2:])).sum(axis=1)
