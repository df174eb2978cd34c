"""The definition of doa.wideband_music (include/doa_hip.h), restated in numpy for the tests, with the wideband signal
generator, the scenario table and the parity shapes of its tests.

    nu_f     = fftfreq(F)[f]                             f_j = (first_bin + j) mod F
    d_f      = float64(float32(d)) (1 + nu_f rho)        the element spacing in wavelengths at bin f
    psi_j,p  = -2 pi cos(theta_p) d_fj                   theta: oracle.music_theta_grid (float-accumulated)
    Q_ij(p)  = Re(a^H P_N a),  a_n = exp(i psi_j,p (N - 1 - 2n) / 2),  P_N = oracle.noise_projector(item, M or c_ij, N, "f64")
    used     : 0 < w_ij < inf, and with counts 1 <= c_ij <= N - 1 (usable weight and c_ij == 0: skipped; any other c_ij: status 2)
    null_mean: Q_i = sum_j w Q_ij / sum_j w              power_sum: Q_i = sum_j w / sum_j (w / Q_ij)
    row      = 10 log10(out / max out), out = 1 / float32(Q_i)
    status   : 0 ok, 1 no bin used, 2 a count outside 0..N-1, 3 a used bin's item is not finite (2 wins over 3); != 0: NaN row
"""
import numpy as np

import doa_oracle as oracle
import channel_covariance_ref as ccref

COMBINE = ("null_mean", "power_sum")


def bin_spacing(d, rho, F, f):
    nu = np.fft.fftfreq(F)[f]
    return float(np.float32(d)) * (1.0 + nu * rho)


def steering(d_f, N, P):
    """[N, P] complex128: a_n = exp(i psi_p (N - 1 - 2n) / 2), psi_p = -2 pi cos(theta_p) d_f."""
    theta = oracle.music_theta_grid(P).astype(np.float64)
    psi = -1.0 * 2 * np.pi * np.cos(theta) * d_f
    half = (N - 1 - 2 * np.arange(N)) / 2.0
    return np.exp(1j * psi[None, :] * half[:, None])


def wideband_music(items, d, M, N, P, F, first_bin=0, num_bins=None, rho=0.0, combine="null_mean", weights=None, counts=None):
    """items: [n, nb, N*N] complex (column-major covariance items).  Returns (dB [n, P] float64, Q [n, P] float64,
    status [n] int32, Qb [n, nb, P] float64 with NaN rows for the bins that are not used)."""
    items = np.asarray(items)
    n, nb = items.shape[0], items.shape[1]
    assert nb == (F if num_bins is None else num_bins) and combine in COMBINE
    sel = ccref.selected_bins(F, first_bin, nb)
    A = [steering(bin_spacing(d, rho, F, f), N, P) for f in sel]
    w_all = np.ones((n, nb)) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(n, nb)
    c_all = None if counts is None else np.asarray(counts).reshape(n, nb)
    dB = np.full((n, P), np.nan)
    Q = np.full((n, P), np.nan)
    Qb = np.full((n, nb, P), np.nan)
    status = np.zeros(n, np.int32)
    for i in range(n):
        used, bad_count, not_finite = [], False, False
        for j in range(nb):
            w = w_all[i, j]
            if not (0.0 < w < np.inf):
                continue
            c = M if c_all is None else int(c_all[i, j])
            if c_all is not None and c == 0:
                continue
            if not 1 <= c <= N - 1:
                bad_count = True
                continue
            if not np.all(np.isfinite(items[i, j].reshape(N, N, order="F")[np.triu_indices(N)])):   # what the eigen stage reads
                not_finite = True
                continue
            used.append((j, w, c))
        status[i] = 2 if bad_count else 3 if not_finite else 0 if used else 1
        if status[i]:
            continue
        num, wsum = np.zeros(P), 0.0
        for j, w, c in used:
            Qb[i, j] = oracle.music_null_spectrum(oracle.noise_projector(items[i, j], c, N, "f64"), A[j])
            num = num + (w * Qb[i, j] if combine == "null_mean" else w / Qb[i, j])
            wsum = wsum + w
        Q[i] = num / wsum if combine == "null_mean" else wsum / num
        out = 1.0 / Q[i].astype(np.float32).astype(np.float64)
        dB[i] = 10.0 * np.log10(out / out.max())
    return dB, Q, status, Qb


# ---- the generator: white Gaussian sources with TRUE TIME DELAYS between the elements ---------------------------------------
def make_streams(N, n_samples, thetas_deg, d, rho, snr_db, seed, F=64, bands=None):
    """[N, n_samples] complex64.  Source m is white complex Gaussian of unit variance; the array response
    exp(i (-2 pi cos theta_m) loc_n d (1 + nu rho)), loc_n = (N - 1 - 2n) / 2, is applied to the FFT of the WHOLE record at
    every frequency nu (cycles per sample), which is a true time delay between the elements.  bands (optional): per source a
    (first, last) pair of bins of an F-point FFT it occupies, inclusive; the rest of its spectrum is zeroed and what is left
    is scaled back to unit power, so that snr_db is a source's signal-to-noise ratio whatever band it occupies.  Noise:
    10^(-snr/20) / sqrt(2) (g1 + i g2) per element and sample."""
    rng = np.random.default_rng(seed)
    nu = np.fft.fftfreq(n_samples)
    loc = (N - 1 - 2 * np.arange(N)) / 2.0
    X = np.zeros((N, n_samples), np.complex128)
    for m, th in enumerate(thetas_deg):
        s = (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)) / np.sqrt(2.0)
        S = np.fft.fft(s)
        if bands is not None:
            b = np.floor(nu * F + 0.5).astype(int) % F              # the F-point bin nearest to nu
            mask = (b >= bands[m][0]) & (b <= bands[m][1])
            S = S * mask / np.sqrt(mask.mean())
        k = -2.0 * np.pi * np.cos(np.deg2rad(th))
        X += S[None, :] * np.exp(1j * k * loc[:, None] * d * (1.0 + nu[None, :] * rho))
    x = np.fft.ifft(X, axis=1)
    g = rng.standard_normal((2, N, n_samples))
    x = x + 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0) * (g[0] + 1j * g[1])
    return x.astype(np.complex64)


D, RHO, P_USE, SEED = 0.4, 0.4, 1024, 1
# name -> N, M, K, F, source directions, SNR in dB, snapshots, bands
SCENARIOS = {
    "two": dict(N=4, M=2, K=1024, F=64, thetas=[40.0, 75.0], snr=15.0, n=6, bands=None),
    "four": dict(N=8, M=4, K=2048, F=64, thetas=[30.0, 60.0, 75.0, 120.0], snr=10.0, n=3, bands=None),
    "split": dict(N=4, M=1, K=1024, F=64, thetas=[50.0, 110.0], snr=15.0, n=6, bands=[(4, 27), (36, 59)]),
}


def scenario_streams(name, seed=SEED):
    s = SCENARIOS[name]
    return make_streams(s["N"], s["n"] * s["K"], s["thetas"], D, RHO, s["snr"], seed, s["F"], s["bands"])


def scenario_items(name, seed=SEED):
    """(streams, [n, F, N*N] complex64 items of all F bins: the float64 channel covariance, Hann, overlap 0, rounded)."""
    s = SCENARIOS[name]
    x = scenario_streams(name, seed)
    R, _ = ccref.channel_covariance(x, s["K"], 0, s["F"], "hann", s["n"])
    return x, R.astype(np.complex64)


def peaks(dB, num, P=P_USE):
    """Directions (degrees, ascending) of the `num` largest local maxima of every row, by oracle.find_local_max."""
    _, loc = oracle.find_local_max(np.asarray(dB, dtype=np.float32), num, P, 0.0, 180.0)
    return np.sort(np.asarray(loc, dtype=np.float64).reshape(len(dB), num), axis=1)


def worst_error(found, truth):
    """Largest |found - truth| in degrees over snapshots and sources (both ascending)."""
    return float(np.abs(np.asarray(found) - np.sort(np.asarray(truth))[None, :]).max())


# ---- the parity shapes of the GPU tests: N, M, F, first_bin, nb, P, n;  K = 2 max(N, 4) F, 15 dB ----------------------------
PARITY_SHAPES = [
    (2, 1, 16, 0, 16, 256, 3), (3, 2, 16, 14, 5, 63, 3), (4, 2, 64, 0, 64, 1024, 9), (4, 1, 32, 7, 1, 65, 3), (5, 2, 16, 0, 16, 257, 3),
    (8, 4, 64, 60, 8, 1024, 3), (11, 3, 32, 0, 32, 720, 2), (16, 3, 32, 0, 32, 4096, 2), (4, 2, 16, 0, 16, 4097, 2),
    (4, 2, 16, 0, 3, 16384, 2), (4, 1, 16, 0, 2, 1, 3),
]


def parity_items(shape, seed=7):
    """[n, nb, N*N] complex64 items of a parity shape: M sources spread over 25..155 degrees."""
    N, M, F, first, nb, _P, n = shape
    K = 2 * max(N, 4) * F
    thetas = list(np.linspace(25.0, 155.0, M + 2)[1:-1])
    x = make_streams(N, n * K, thetas, D, RHO, 15.0, [seed, N, F], F)
    R, _ = ccref.channel_covariance(x, K, 0, F, "hann", n, first, nb)
    return R.astype(np.complex64)
