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


FFT_LENS = (16, 32, 64, 128, 256)


def round_structures(F):
    """Block counts B = K / F that reach every guard of the kernel's round loop for this F.  A wave takes CB = max(1, 64 / F)
    blocks side by side and a round RB = 4 CB blocks (csrc/channel_covariance.hip); the counts follow from those two:
        1                a single block
        CB - 1, CB + 1   a wave with some of its side-by-side blocks empty; a second wave with one block (CB > 1 only)
        RB - 1, RB       one round less one block; exactly one round
        RB + 1           a second round of one block
        2 RB + CB + 1    a third round that ends inside the second wave
        3 RB             several full rounds
    F = 16: 1 3 5 15 16 17 37 48;  F = 32: 1 3 7 8 9 19 24;  F >= 64: 1 3 4 5 10 12."""
    CB = max(1, 64 // F)
    RB = 4 * CB
    counts = {1, RB - 1, RB, RB + 1, 2 * RB + CB + 1, 3 * RB}
    if CB > 1:
        counts |= {CB - 1, CB + 1}
    return sorted(counts)


def partial_third_round(F):
    """The count of round_structures(F) with two full rounds and a third that ends inside the second wave."""
    CB = max(1, 64 // F)
    return 2 * (4 * CB) + CB + 1


def sweep_samples(N, F, B, n=3):
    """The sweep's input: int16 [N, n B F, 2] over the whole int16 range, seeded by the shape.  doa.sim.from_sc16 widens
    it to the complex64 samples the fc32 runs take, so every format and route sees the same values."""
    return np.random.default_rng([N, F, B]).integers(-32768, 32768, size=(N, n * B * F, 2), dtype=np.int16)


def sweep_window(case, F):
    """Window number `case` of the sweep: the four named ones, then a random positive one (float32 [F])."""
    names = WINDOWS + ("custom",)
    name = names[case % len(names)]
    if name == "custom":
        return name, (0.25 + np.random.default_rng(F).random(F)).astype(np.float32)
    return name, name


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_items_match(cov, pw, R64, p64, N, F, label=None):
    """What every full-band output of the block is held to.  cov [n, F, N*N] complex64 and pw [n, F] float32 from the device,
    R64 and p64 from channel_covariance().  Parity: |R_hip - R_f64| <= 2e-6 max|R|, the maximum over all bins of the
    snapshot.  The item contract, bit for bit: the lower triangle is the conjugate of the upper one, diagonal imaginary
    parts are +0, power is the in-order float sum of the stored diagonals (and within 2e-6 N max|R| of float64).
    Prints the worst parity error as a fraction of max|R| under `label` before asserting, and returns it."""
    n = cov.shape[0]
    assert cov.shape == (n, F, N * N) and pw.shape == (n, F) and cov.dtype == np.complex64 and pw.dtype == np.float32
    scale = np.abs(R64).reshape(n, -1).max(axis=1)
    err = np.abs(cov - R64).reshape(n, -1).max(axis=1) / scale
    if label:
        print(f"{label}: {err.max():.2e} of max|R|")
    assert err.max() <= 2e-6
    # exactly Hermitian: the lower triangle is the bitwise conjugate of the upper one, diagonal imaginary parts are +0
    M = cov.reshape(n, F, N, N)                                    # [i, f, q, p] = R[p, q]
    assert np.array_equal(bits(M.real), bits(M.real.transpose(0, 1, 3, 2)))
    assert np.array_equal(bits(M.imag), bits(-M.imag.transpose(0, 1, 3, 2)) * (1 - np.eye(N, dtype=np.uint32)))
    # power: the in-order float sum of the returned diagonals, bit for bit
    want = np.zeros((n, F), np.float32)
    for p in range(N):
        want = want + M[:, :, p, p].real
    assert np.array_equal(bits(pw), bits(want))
    assert np.abs(pw - p64).max() <= 2e-6 * N * scale.max()
    return float(err.max())


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
