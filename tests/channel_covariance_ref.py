"""The definition of doa.channel_covariance (include/doa_hip.h), restated in numpy for the tests.

    B = K / F blocks per snapshot, snapshot i starts at sample i (K - overlap), block b covers [bF, bF + F):
    X[a,b,f]   = sum_t w[t] x_a[s_i + bF + t] exp(-2 pi i f t / F)
    R_i,f[p,q] = 1 / (B W2) sum_b X[p,b,f] conj(X[q,b,f]),        W2 = sum_t w[t]^2  (double, from the float32 w)

channel_covariance() is that formula in float64 (the truth the device is held to); channel_covariance_f32() does the
device's steps in float32 (windowed sample, radix-2 FFT with twiddles rounded from double, float accumulation over the
blocks, one final scale) and serves only as a yardstick for what float32 arithmetic can reach.
Items are returned as the block writes them: [n, num_bins, N*N], each matrix column-major, R[p,q] at p + q N."""
import numpy as np

WINDOWS = ("rect", "hann", "hamming", "blackman")

# the use case: five tones at different frequencies and directions on a 4-element half-wavelength ULA, 20 dB SNR --
# one emitter more than the whole-band covariance of four antennas can separate
THETAS = [25.0, 60.0, 88.0, 120.0, 155.0]
BINS = [5, 17, 30, 41, 55]                          # of 64
FREQS = [(b + 0.08) / 64.0 for b in BINS]           # near, not on, the bin centres


def five_emitters(n=6):
    """[4, n * 1024] complex64 streams of the use case."""
    from doa import sim
    return sim.make_streams(4, n * 1024, THETAS, 0.5, snr_db=20.0, seed=3, freqs=FREQS)


def window(name, fft_len):
    """Periodic window of fft_len points, computed in double and rounded to float32."""
    t = 2.0 * np.pi * np.arange(fft_len, dtype=np.float64) / fft_len
    if name == "rect":
        w = np.ones(fft_len)
    elif name == "hann":
        w = 0.5 - 0.5 * np.cos(t)
    elif name == "hamming":
        w = 0.54 - 0.46 * np.cos(t)
    elif name == "blackman":
        w = 0.42 - 0.5 * np.cos(t) + 0.08 * np.cos(2.0 * t)
    else:
        raise ValueError(f"unknown window {name!r}")
    return w.astype(np.float32)


def _window_of(w, fft_len):
    w = window(w, fft_len) if isinstance(w, str) else np.asarray(w, dtype=np.float32)
    assert w.shape == (fft_len,)
    return w


def selected_bins(fft_len, first_bin=0, num_bins=None):
    nb = fft_len if num_bins is None else int(num_bins)
    return (int(first_bin) + np.arange(nb)) % fft_len


def _blocks(x, K, overlap, F, n):
    """[n, N, B, F] view of the snapshots' blocks (complex128)."""
    x = np.asarray(x)
    N, S, B = x.shape[0], K - overlap, K // F
    assert K % F == 0 and x.shape[1] >= (n - 1) * S + K
    return np.stack([x[:, i * S:i * S + K].reshape(N, B, F) for i in range(n)]).astype(np.complex128)


def channel_covariance(x, K, overlap, F, w, n, first_bin=0, num_bins=None):
    """float64 definition.  x: [N, >= (n-1)(K-overlap)+K] complex.  Returns (R [n, num_bins, N*N] complex128,
    power [n, F] float64: the trace of every bin's matrix, all F bins whatever the selection)."""
    w = _window_of(w, F).astype(np.float64)
    B = K // F
    X = np.fft.fft(_blocks(x, K, overlap, F, n) * w, axis=-1)                   # [n, N, B, F]
    R = np.einsum("ipbf,iqbf->ifpq", X, X.conj()) / (B * np.sum(w * w))          # [n, F, p, q]
    power = np.einsum("ifpp->if", R).real
    N = R.shape[-1]
    items = R.transpose(0, 1, 3, 2).reshape(n, F, N * N)                         # column-major: p + q N
    return items[:, selected_bins(F, first_bin, num_bins)], power


def _fft_f32(v):
    """Radix-2 decimation-in-frequency FFT along the last axis in complex64, twiddles rounded from double; natural order out."""
    v = np.array(v, dtype=np.complex64)
    F = v.shape[-1]
    lg = F.bit_length() - 1
    assert 1 << lg == F
    k = np.arange(F // 2)
    tw = np.exp(-2j * np.pi * k / F).astype(np.complex64)
    L = F
    while L >= 2:
        h = L // 2
        u = v.reshape(v.shape[:-1] + (F // L, L))
        a, b = u[..., :h], u[..., h:]
        u = np.concatenate([a + b, ((a - b) * tw[(np.arange(h) * (F // L))]).astype(np.complex64)], axis=-1)
        v = u.reshape(v.shape).astype(np.complex64)
        L = h
    rev = np.array([int(format(i, f"0{lg}b")[::-1], 2) for i in range(F)])
    return v[..., rev]


def channel_covariance_f32(x, K, overlap, F, w, n, first_bin=0, num_bins=None):
    """The same steps in float32 (a yardstick, not a bit-exact model of the device)."""
    w = _window_of(w, F)
    B = K // F
    S = K - overlap
    x = np.asarray(x, dtype=np.complex64)
    N = x.shape[0]
    scale = np.float32(1.0 / (B * np.sum(w.astype(np.float64) ** 2)))
    out = np.empty((n, F, N * N), np.complex64)
    for i in range(n):
        blk = x[:, i * S:i * S + K].reshape(N, B, F)
        X = _fft_f32((blk * w).astype(np.complex64))                             # [N, B, F]
        acc = np.zeros((F, N, N), np.complex64)
        for b in range(B):
            acc = (acc + np.einsum("pf,qf->fpq", X[:, b, :], X[:, b, :].conj()).astype(np.complex64)).astype(np.complex64)
        out[i] = (acc * scale).astype(np.complex64).transpose(0, 2, 1).reshape(F, N * N)
    power = np.zeros((n, F), np.float32)
    for p in range(N):
        power = (power + out[:, :, p + p * N].real).astype(np.float32)
    return out[:, selected_bins(F, first_bin, num_bins)], power


def music_angle(R_item, norm_spacing, N, grid=1 << 14):
    """Single-source MUSIC on one column-major item with numpy eigh: the direction (degrees) of the largest peak of
    1 / (a^H U_n U_n^H a) on `grid` points of [0, 180)."""
    R = np.asarray(R_item, dtype=np.complex128).reshape(N, N, order="F")
    _, V = np.linalg.eigh(R)
    Un = V[:, :N - 1]
    theta = np.arange(grid) * (180.0 / grid)
    loc = norm_spacing * ((N - 1) / 2.0 - np.arange(N))
    A = np.exp(-2j * np.pi * np.cos(np.deg2rad(theta))[None, :] * loc[:, None])
    q = np.sum(np.abs(Un.conj().T @ A) ** 2, axis=0)
    return float(theta[np.argmin(q)])
