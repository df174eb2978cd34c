"""numpy restatement of the spatial smoothing of doa.spatial_smooth / music_pipeline.set_spatial_smoothing
(include/doa_hip.h), for its tests, and the coherent-source scenarios they share (importable like source_count_ref.py).
Not a block of the reference: the definition is this project's, stated once in the header and written out here literally.

Input item: column-major N x N complex64, only the upper triangle read, of the diagonal the real part (its imaginary part
is taken as 0): H = the Hermitian matrix these define.  Output item: column-major S x S complex64, full Hermitian.  With
L = N - S + 1, for 0 <= i <= j < S:

    f[i,j]   = sum_{l=0}^{L-1} (double) H[i+l, j+l]        l ascending, re and im separately
    fb == 0 : s = f[i,j]
    fb == 1 : s = 0.5 * (f[i,j] + f[S-1-j, S-1-i])
    out[i,j] = (float)(s * (1.0 / L))                      1.0 / L formed in double; one rounding per component
    out[j,i] = conj(out[i,j]);  Im out[i,i] = +0.0

No product feeds an addition, so a device implementation that does these operations in this order is bit-identical.
"""
import functools

import numpy as np

import doa
import doa_oracle as oracle


def smooth(R_items, N, S, fb):
    """[n, S*S] complex64 from [n, N*N] complex64 items (column-major), as defined above."""
    R = np.asarray(R_items).reshape(-1, N, N)            # [item][col][row]
    n, L = R.shape[0], N - S + 1
    re = R.real.astype(np.float64).transpose(0, 2, 1)     # [item][row][col]
    im = R.imag.astype(np.float64).transpose(0, 2, 1)
    fr, fi = np.zeros((n, S, S)), np.zeros((n, S, S))
    for i in range(S):
        for j in range(i, S):
            sr, si = np.zeros(n), np.zeros(n)
            for l in range(L):                           # ascending
                sr = sr + re[:, i + l, j + l]
                if i != j:                               # diagonal: the imaginary part is taken as 0
                    si = si + im[:, i + l, j + l]
            fr[:, i, j], fi[:, i, j] = sr, si
    inv = 1.0 / L
    out = np.zeros((n, S, S), np.complex64)              # [item][col][row]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(S):
            for j in range(i, S):
                sr, si = fr[:, i, j], fi[:, i, j]
                if fb:
                    sr = 0.5 * (sr + fr[:, S - 1 - j, S - 1 - i])
                    si = 0.5 * (si + fi[:, S - 1 - j, S - 1 - i])
                o_re, o_im = (sr * inv).astype(np.float32), (si * inv).astype(np.float32)
                out.real[:, j, i], out.imag[:, j, i] = o_re, o_im          # element (row i, col j)
                if i != j:
                    out.real[:, i, j], out.imag[:, i, j] = o_re, -o_im     # its conjugate at (row j, col i)
    return out.reshape(n, S * S)


# ---- coherent scenarios: x = A(theta) (rho (x) s) + sigma w, one tone through M paths with complex path gains rho ----------
K, N_SNAP, D, P, SNR_DB, SEED, TONE = 256, 24, 0.5, 1024, 20.0, 3, 0.0417
_RHO2 = (1.0, 0.8 * np.exp(1j))
_RHO3 = (1.0, 0.8 * np.exp(1j), 0.9 * np.exp(-2j))
# name: (N, S, forward-backward, source angles, path gains)
SCENARIOS = {
    "A": (8, 6, 1, (60.0, 100.0), _RHO2),
    "B": (4, 3, 1, (60.0, 110.0), _RHO2),
    "C": (16, 12, 1, (50.0, 75.0, 120.0), _RHO3),
    "A_forward": (8, 6, 0, (60.0, 100.0), _RHO2),
}
TABLE = ("A", "B", "C")              # the rows with forward-backward smoothing


def coherent_streams(N, thetas, rho, n_samples, d=D, snr_db=SNR_DB, seed=SEED, tone=TONE):
    """[N, n_samples] complex64: fully coherent sources at `thetas` (one tone, path gains rho) plus white noise."""
    rng = np.random.default_rng(seed)
    A = doa.sim.manifold(d, N, thetas)
    s = np.exp(2j * np.pi * tone * np.arange(n_samples, dtype=np.float64))
    x = A @ (np.asarray(rho, np.complex128)[:, None] * s[None, :])
    sigma = 10.0 ** (-snr_db / 20.0)
    w = (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) / np.sqrt(2.0)
    return np.ascontiguousarray((x + sigma * w).astype(np.complex64))


@functools.lru_cache(maxsize=None)
def streams(name):
    N, S, fb, th, rho = SCENARIOS[name]
    x = coherent_streams(N, th, rho, N_SNAP * K)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def covariance(name):
    """[24, N*N] complex64 (oracle.autocorrelate, overlap 0, avg_method 0), read-only."""
    R = oracle.autocorrelate(streams(name), K, 0, 0, N_SNAP)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def smoothed(name):
    N, S, fb, th, rho = SCENARIOS[name]
    Rs = smooth(covariance(name), N, S, fb)
    Rs.setflags(write=False)
    return Rs


def exact_covariance(name):
    """The noise-free covariance A rho rho^H A^H as one complex64 item [1, N*N]: signal rank one."""
    N, S, fb, th, rho = SCENARIOS[name]
    v = doa.sim.manifold(D, N, th) @ np.asarray(rho, np.complex128)
    return np.outer(v, v.conj()).reshape(1, N * N, order="F").astype(np.complex64)


def angle_error(locs, thetas):
    """max over items of the largest |estimate - truth| after sorting both ([n, M] estimates in any order)."""
    return float(np.abs(np.sort(np.asarray(locs, np.float64), axis=1) - np.sort(np.asarray(thetas))[None, :]).max())
