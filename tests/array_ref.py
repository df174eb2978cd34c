"""numpy restatement of the steering-table spectra doa.MUSIC_array / doa.capon_array / music_pipeline.set_steering_table
(include/doa_hip.h), for their tests, and the scenario table they share (importable like capon_ref.py).
Not blocks of the reference: the definition is this project's, stated once in the header and written out here.

A steering table is [P, N] complex128, row i = the array response a_i towards direction i.  For the item's Hermitian matrix X
(the noise projector P_N for MUSIC, W = (H / mu + delta I)^-1 for Capon, exactly as capon_ref.py states it), in double:

    Q_i = Re(a_i^H X a_i);  out = 1 / Q;  spectrum = 10 log10(out / max out)          (the fp64 oracle's formulas)

The planar table: az_i = az_min + i (az_max - az_min) / P, elevation theta from the array normal,
    a_i[n] = exp(+j 2 pi sin(theta) (x_n cos az_i + y_n sin az_i)).
"""
import functools

import numpy as np

import doa
import doa_oracle as oracle
import capon_ref

P = 720
SEED = 3
N_ITEMS = 8


def uca(N):
    """[N, 2] positions of a uniform circular array with half a wavelength between neighbours."""
    radius = 0.5 / (2.0 * np.sin(np.pi / N))
    ang = 2.0 * np.pi * np.arange(N) / N
    return np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1)


def ula(N, d=0.5):
    return np.stack([d * (np.arange(N) - (N - 1) / 2.0), np.zeros(N)], axis=1)


def steering(positions, az_deg, elevation=90.0):
    """[len(az), N] complex128: the formula above at the given azimuths (degrees)."""
    xy = np.asarray(positions, np.float64)
    az = np.deg2rad(np.atleast_1d(np.asarray(az_deg, np.float64)))
    proj = xy[None, :, 0] * np.cos(az)[:, None] + xy[None, :, 1] * np.sin(az)[:, None]
    ph = 2.0 * np.pi * np.sin(np.deg2rad(float(elevation))) * proj
    return np.cos(ph) + 1j * np.sin(ph)


def grid(P_len, az_min=0.0, az_max=360.0):
    return az_min + np.arange(P_len, dtype=np.float64) * (az_max - az_min) / P_len


def planar_table(positions, P_len, az_min=0.0, az_max=360.0, elevation=90.0):
    return steering(positions, grid(P_len, az_min, az_max), elevation)


# name -> (positions, sources (deg), SNR dB, K)
SCENARIOS = {
    "uca5": (uca(5), (70.3, 250.2), 20.0, 256),
    "uca8": (uca(8), (40.3, 200.2, 260.1), 10.0, 256),
    "sq4": (uca(4), (100.2, 300.4), 20.0, 1024),
    "uca16": (uca(16), (30.1, 180.3, 200.2), 20.0, 64),
    "uca3": (uca(3), (130.0,), 30.0, 64),
    "rand11": (np.random.default_rng(5).uniform(-1, 1, (11, 2)), (50.0, 100.0, 310.0), 20.0, 128),
}
NAME_OF_N = {5: "uca5", 8: "uca8", 4: "sq4", 16: "uca16", 3: "uca3", 11: "rand11"}


def make_streams(positions, sources, snr_db, n_samples, seed=SEED):
    """[N, n_samples] complex64: steering(sources) @ tones plus noise 10^(-snr/20) / sqrt(2) (g1 + j g2)."""
    rng = np.random.default_rng(seed)
    M = len(sources)
    t = np.arange(n_samples, dtype=np.float64)
    tones = np.exp(2j * np.pi * doa.sim.tone_frequencies(M)[:, None] * t[None, :])
    x = steering(positions, sources).T @ tones
    g1 = rng.standard_normal(x.shape)
    g2 = rng.standard_normal(x.shape)
    x = x + 10.0 ** (-float(snr_db) / 20.0) / np.sqrt(2.0) * (g1 + 1j * g2)
    return np.ascontiguousarray(x.astype(np.complex64))


@functools.lru_cache(maxsize=None)
def streams(name, n_items=N_ITEMS):
    pos, src, snr_db, K = SCENARIOS[name]
    x = make_streams(pos, src, snr_db, n_items * K)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def covariance(name, n_items=N_ITEMS):
    """[n_items, N*N] complex64 (oracle.autocorrelate, overlap 0, avg_method 0), read-only."""
    K = SCENARIOS[name][3]
    R = oracle.autocorrelate(streams(name, n_items), K, 0, 0, n_items)
    R.setflags(write=False)
    return R


def music(R_items, table, M):
    """(spectrum [n, P] float64 dB, Q [n, P] float64, P_N [n, N, N] complex128)."""
    table = np.asarray(table, np.complex128)
    P_len, N = table.shape
    R_items = np.asarray(R_items).reshape(-1, N * N)
    n = R_items.shape[0]
    spec, q, X = np.empty((n, P_len)), np.empty((n, P_len)), np.empty((n, N, N), np.complex128)
    for i in range(n):
        X[i] = oracle.noise_projector(capon_ref.hermitian_from_upper(R_items[i], N).reshape(-1, order="F"), M, N, "f64")
        q[i] = oracle.music_null_spectrum(X[i], table.T)
        spec[i] = oracle.music_db_from_q(q[i], "f64")
    return spec, q, X


def capon(R_items, table, delta):
    """(spectrum, Q, W [n, N, N] complex128, status [n] int32); status-1 items are NaN (capon_ref.py's rule)."""
    table = np.asarray(table, np.complex128)
    P_len, N = table.shape
    R_items = np.asarray(R_items).reshape(-1, N * N)
    n = R_items.shape[0]
    spec, q = np.full((n, P_len), np.nan), np.full((n, P_len), np.nan)
    W = np.full((n, N, N), np.nan + 0j)
    st = np.zeros(n, np.int32)
    for i in range(n):
        st[i] = capon_ref.status(R_items[i], N, delta)
        if st[i]:
            continue
        A, _ = capon_ref.loaded(R_items[i], N, delta)
        W[i] = np.linalg.inv(A)
        q[i] = oracle.music_null_spectrum(W[i], table.T)
        spec[i] = oracle.music_db_from_q(q[i], "f64")
    return spec, q, W, st


def angle_error(locs, sources):
    """max over items of the largest |estimate - truth| after sorting both ([n, M] estimates in any order)."""
    return float(np.abs(np.sort(np.asarray(locs, np.float64), axis=1) - np.sort(np.asarray(sources))[None, :]).max())


def angle_cap(P_len, span=360.0):
    """0.6 degrees plus one grid step of the axis."""
    return 0.6 + span / P_len
