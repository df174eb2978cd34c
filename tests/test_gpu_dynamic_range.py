"""GPU tests over the dynamic range of the input: K1 and every eigen-stage route at power-of-two scales of the data.

The reference's eig_sym (LAPACK cheevd) rescales its input, so it gives the same projector for R and 2^s R over the whole
float range; K1 (sums of products, a 1/K and optional gain and FB factors) commutes exactly with a power-of-two scale as
long as nothing is subnormal or overflows.  What is pinned here:
  * K1: streams x 2^k give R x 4^k bit for bit on every K1 route, and every element is within 2e-6 sqrt(P_a P_b) of the
    fp64 value (P_a = channel a's power in that window), across channels 2^+-20 apart in power and windows 2^10 apart;
  * the eigen stage: every launch branch of launch_music_evd, at both precisions, on items replicated at 2^s for
    s = -100 ... 127 (the top float binade) and interleaved so that every wave mixes scales: the projector and spectrum
    bounds of test_gpu_music.py against fp64 eigh of the base item, P_N / Q / spectrum bit-identical to the s = 0 copy
    (every route pre-scales by an exact power of two, or -- the one-lane double Jacobi -- runs in double throughout),
    and the same fall-back count as the unscaled batch;
  * Root-MUSIC and calibrate_lin_array on the same scales; the two pipelines end to end.
Out of range on purpose: subnormal-only items, and K1 sums above FLT_MAX (which overflow in the reference too).
"""
import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle

pytestmark = pytest.mark.gpu

_C64 = np.complex64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize % 8 == 0 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------------------------------
# (K, overlap, N, FB, fused gain, 8-byte-aligned device pointers): one shape per route of launch_autocorrelate
K1_ROUTES = {
    **{f"wave_vec2_n{N}": (128, 0, N, N % 2, False, False) for N in range(1, 9)},   # cov_wave_kernel<N, true>
    "wave_odd_s": (129, 0, 5, 1, False, False),                                      # cov_wave_kernel<N, false>: odd S
    "wave_unaligned": (256, 64, 4, 1, False, True),                                  # ... 8-byte-aligned streams
    "piece_combine": (1024, 512, 4, 1, False, False),                                # cov_piece_kernel + cov_combine_kernel
    "piece_combine_r": (1000, 700, 7, 0, False, False),                              # K = 3 S + 100: pieces A_j and B_j
    "mfma_vec2": (128, 0, 12, 0, False, False),                                      # cov_mfma_kernel<true>
    "mfma_odd_s": (129, 0, 9, 0, False, False),                                      # cov_mfma_kernel<false>
    "mfma_fb": (256, 32, 16, 1, False, False),                                       # cov_mfma_kernel<true> + cov_fb_kernel
    "gain_wave": (256, 0, 4, 0, True, False),
    "gain_piece": (1024, 512, 5, 1, True, False),
    "gain_mfma": (128, 0, 10, 1, True, False),
}


def _gains(N, seed):
    rng = np.random.default_rng(seed)
    return (10 ** (rng.uniform(-12, 12, N) / 20) * np.exp(2j * np.pi * rng.uniform(0, 1, N))).astype(_C64)


def _run_k1(route, x, n, gains=None):
    K, ovl, N, fb, _, unaligned = route
    blk = doa.autocorrelate(N, K, ovl, fb)
    if gains is not None:
        blk.fuse_antenna_correction(gains)
    if not unaligned:
        out = np.empty((n, N * N), _C64)
        produced, _ = blk.general_work(n, [x[k] for k in range(N)], [out])
        assert produced == n
        return out
    # device streams one complex sample past a 16-byte boundary: the scalar-load path of the wave kernel
    span = blk.input_span(n)
    dev = [torch.zeros(span + 1, dtype=torch.complex64, device="cuda") for _ in range(N)]
    for k in range(N):
        dev[k][1:] = torch.from_numpy(np.ascontiguousarray(x[k][:span]))
    ptrs = [t[1:].data_ptr() for t in dev]
    assert all(p % 16 == 8 for p in ptrs)
    out = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    blk.work_dev(n, ptrs, out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(K1_ROUTES))
def test_k1_exact_power_of_two_scaling(name):
    route = K1_ROUTES[name]
    K, ovl, N, fb, gain, _ = route
    n, S = 6, K - ovl
    rng = np.random.default_rng(sum(map(ord, name)))
    # every component of magnitude in [0.5, 2): no product of two samples is subnormal even at 2^-40 per sample
    v = rng.uniform(0.5, 2.0, (2, N, (n - 1) * S + K)) * rng.choice([-1.0, 1.0], (2, N, (n - 1) * S + K))
    x = (v[0] + 1j * v[1]).astype(_C64)
    g = _gains(N, 5) if gain else None
    base = _run_k1(route, x, n, g)
    nz = np.abs(np.concatenate([base.real.ravel(), base.imag.ravel()]))
    assert nz[nz > 0].min() >= 2.0 ** -40                      # 4^-40 base stays normal
    for k in (-40, -13, 1, 7, 30):
        got = _run_k1(route, (x * np.float32(2.0 ** k)).astype(_C64), n, g)
        want = (base * np.float32(4.0 ** k)).astype(_C64)
        assert _same_bits(got, want), (name, k, np.abs(got - want).max())


def _k1_f64(x, K, S, n, fb):
    N = x.shape[0]
    J = np.fliplr(np.eye(N))
    R, P = np.empty((n, N, N), np.complex128), np.empty((n, N))
    for i in range(n):
        w = x[:, i * S:i * S + K].astype(np.complex128)
        Ri = w @ w.conj().T / K
        R[i] = 0.5 * Ri + (0.5 / K) * J @ np.conj(Ri) @ J if fb else Ri
        P[i] = np.mean(np.abs(w) ** 2, axis=1)
    return R, P


@pytest.mark.parametrize("name", list(K1_ROUTES))
def test_k1_per_element_bound_across_channel_and_window_power(name):
    route = K1_ROUTES[name]
    K, ovl, N, fb, gain, _ = route
    n, S = 12, K - ovl
    T = (n - 1) * S + K
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    x = rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T))
    chan = 2.0 ** rng.uniform(-10, 10, N)                       # per-antenna power spread up to 2^+-20
    chan[0], chan[-1] = 2.0 ** -10, 2.0 ** 10
    env = 2.0 ** (5.0 * np.array([0, 1, 0, -1])[np.arange(T // S + 1) % 4])     # consecutive S-blocks 2^10 apart in power
    x = (x * chan[:, None] * env[None, np.arange(T) // S]).astype(_C64)
    g = _gains(N, 6) if gain else None
    got = _run_k1(route, x, n, g).reshape(n, N, N).transpose(0, 2, 1)           # column-major items -> [a, b]
    xt = x.astype(np.complex128) * (g.astype(np.complex128)[:, None] if gain else 1.0)
    R64, P = _k1_f64(xt, K, S, n, fb)
    sq = np.sqrt(P[:, :, None] * P[:, None, :])
    bound = 0.5 * sq + (0.5 / K) * sq[:, ::-1, ::-1] if fb else sq               # each FB term by its own channels
    err = np.abs(got - R64)
    assert np.all(err <= 2e-6 * bound), (name, (err / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# eigen stage
# ---------------------------------------------------------------------------------------------------------------------
# s of 2^s on a base item whose largest component is in [1, 2): 127 puts it in the top float binade.  Index 0 is the
# unscaled copy the others are compared with.
SCALES = [0, -100, -61, -1, 1, 37, 64, 100, 127]
P_LEN = 256

# (precision, N, M): every launch branch of launch_music_evd at least once
EVD_CASES = [
    (64, 2, 1), (64, 3, 1), (64, 4, 1),          # one-lane subspace iteration, one-lane classic Jacobi fall-back
    (64, 3, 2), (64, 4, 3),                      # one-lane classic Jacobi
    (64, 4, 2),                                  # quad, group<4> fall-back
    (64, 5, 2), (64, 8, 4),                      # subspace G = 8, block16 fall-back
    (64, 9, 3), (64, 16, 4),                     # subspace G = 16, block16 fall-back
    (64, 6, 4), (64, 8, 5),                      # group<8>
    (64, 12, 7), (64, 16, 5),                    # block16
    (32, 2, 1), (32, 4, 1), (32, 4, 2), (32, 4, 3),   # one-lane float Jacobi
    (32, 5, 2), (32, 8, 4),                      # group<8, float>
    (32, 9, 3), (32, 16, 3),                     # block16<float>
]


def _array_cov(rng, N, M, snr_db, K, fb=False, gains=None):
    th = np.sort(rng.uniform(15.0, 165.0, M)) + 6.0 * np.arange(M)
    A = np.exp(-2j * np.pi * 0.5 * np.cos(np.deg2rad(th))[None, :] * np.arange(N)[:, None])
    s = (rng.standard_normal((M, K)) + 1j * rng.standard_normal((M, K))) / np.sqrt(2)
    w = (rng.standard_normal((N, K)) + 1j * rng.standard_normal((N, K))) / np.sqrt(2) * 10 ** (-snr_db / 20)
    x = A @ s + w
    if gains is not None:
        x = gains[:, None] * x
    R = x @ x.conj().T / K
    if fb:
        J = np.fliplr(np.eye(N))
        R = 0.5 * R + 0.5 * J @ R.conj() @ J
    return R


def _near_equal(rng, N, M, ratio):
    # lambda_M / lambda_{M+1} = ratio: the subspace iterations give up and take their Jacobi fall-back
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
    lam = np.concatenate([2.0 + 0.1 * np.arange(M - 1, 0, -1), [ratio], 1.0 - 1e-3 * np.arange(N - M)])
    return (Q * lam) @ Q.conj().T


def _normalise(A):
    """complex64 column-major item, exact power-of-two scale to a largest component in [1, 2), components below 2^-20
    of it set to zero (so that no component of a copy at 2^-100 is subnormal)."""
    it = np.asarray(A, np.complex64).reshape(-1, order="F")
    re, im = it.real.copy(), it.imag.copy()
    m = max(np.abs(re).max(), np.abs(im).max())
    e = int(np.floor(np.log2(m)))
    re, im = re * np.float32(2.0 ** -e), im * np.float32(2.0 ** -e)
    m = max(np.abs(re).max(), np.abs(im).max())
    assert 1.0 <= m < 2.0
    re[np.abs(re) < 2.0 ** -20] = 0
    im[np.abs(im) < 2.0 ** -20] = 0
    return (re + 1j * im).astype(_C64)


def _base_items(N, M, seed):
    """(items [n, N*N] complex64, well-conditioned flag per item, forward-backward flag per item)"""
    rng = np.random.default_rng(seed)
    mats = [_array_cov(rng, N, M, snr, K) for snr, K in ((20.0, 1024), (10.0, 512), (3.0, 256)) for _ in range(2)]
    mats += [_array_cov(rng, N, M, 10.0, 256, fb=True) for _ in range(2)]
    mats += [_array_cov(rng, N, M, 15.0, 512, gains=10 ** (rng.uniform(-12, 12, N) / 20)) for _ in range(2)]
    good = [True] * len(mats)
    mats += [_near_equal(rng, N, M, 1.001), _near_equal(rng, N, M, 1.003)]
    good += [False, False]
    fb = np.zeros(len(mats), bool)
    fb[6:8] = True
    return np.stack([_normalise(A) for A in mats]), np.array(good), fb


def _replicate(base, scales):
    """base item b at scale scales[j] -> row b * len(scales) + j: consecutive items of a wave carry different scales"""
    out = np.stack([(base * np.float32(2.0 ** s)).astype(_C64) for s in scales], axis=1)
    return np.ascontiguousarray(out.reshape(-1, base.shape[1]))


def _herm(it, N):
    A = it.reshape(N, N, order="F").astype(np.complex128)
    A = np.triu(A) + np.triu(A, 1).conj().T                      # uplo = 'U'
    A[np.diag_indices(N)] = A.diagonal().real
    return A


def _pn64(items, N, M):
    out = []
    for it in items:
        _, V = np.linalg.eigh(_herm(it, N))
        out.append(V[:, : N - M] @ V[:, : N - M].conj().T)
    return np.stack(out)


def _per_copy(a, n_scales):
    return a.reshape(-1, n_scales, *a.shape[1:])


@pytest.mark.parametrize("bits,N,M", EVD_CASES)
def test_eigen_stage_across_scales(bits, N, M):
    base, good, fb = _base_items(N, M, seed=100 * N + M + bits)
    nb, ns = base.shape[0], len(SCALES)
    mixed = _replicate(base, SCALES)
    flat = _replicate(base, [0] * ns)                            # the mixed batch's layout, every copy unscaled
    blk = doa.MUSIC_lin_array(0.5, M, N, P_LEN)
    blk.set_internal_precision(bits)

    def run(items):
        doa.evd_fallback_count(reset=True)
        pn, q = blk.debug(items)
        n_fb = doa.evd_fallback_count(reset=True)
        spec = np.empty((items.shape[0], P_LEN), np.float32)
        assert blk.work(items.shape[0], [items], [spec]) == items.shape[0]
        return pn, q, spec, n_fb

    *_, fb_base = run(base)
    *flat_out, fb_flat = run(flat)
    pn, q, spec, fb_mixed = run(mixed)

    # (3) scaling changes no output bit: every item against its unscaled copy at the same batch position (same wave
    # mates), and -- where the path is chosen per item -- every copy against the s = 0 copy.  The quad kernel decides
    # its fall-back for a whole wave at once, and the 9 copies of an item straddle its 16-item waves.
    per_item = (bits, N, M) != (64, 4, 2)
    for name, a, a0 in (("P_N", pn, flat_out[0]), ("Q", q, flat_out[1]), ("spectrum", spec, flat_out[2])):
        bad = np.nonzero(np.any(_bits(a) != _bits(a0), axis=1))[0]
        assert bad.size == 0, (name, bits, N, M, [SCALES[i % ns] for i in bad[:8]])
        c = _per_copy(a, ns)
        for j in range(1, ns if per_item else 1):
            assert _same_bits(c[:, j], c[:, 0]), (name, bits, N, M, SCALES[j], np.abs(c[:, j] - c[:, 0]).max())
    # (4) no scale sends an item (or its wave) to a different path
    assert fb_mixed == fb_flat, (bits, N, M, fb_mixed, fb_flat)
    if per_item:
        assert fb_mixed == ns * fb_base, (bits, N, M, fb_mixed, fb_base)

    # (1), (2) against fp64 eigh of the base item (the f32 oracle for the precision-32 bounds of test_gpu_music.py)
    s32, q32, p32 = oracle.music_lin_array(base, 0.5, M, N, P_LEN, "f32", return_parts=True)
    s64, q64, p64 = oracle.music_lin_array(base, 0.5, M, N, P_LEN, "f64", return_parts=True)
    want_pn = _pn64(base, N, M)
    pn_c, q_c, spec_c = _per_copy(pn, ns), _per_copy(q, ns), _per_copy(spec, ns)
    for b in range(nb):
        e_ref_p = np.abs(p32[b] - p64[b]).max()
        w = np.linalg.eigvalsh(_herm(base[b], N))
        gap = (w[N - M] - w[N - M - 1]) / w[-1]          # relative gap across the signal / noise boundary
        qt, mx = q64[b], q64[b].max()
        g1, g2 = qt >= 1e-1 * mx, qt >= 1e-2 * mx
        err_ref = np.abs(q32[b] - qt)
        for j, s in enumerate(SCALES):
            e_p = np.abs(pn_c[b, j].reshape(N, N, order="F") - want_pn[b]).max()
            if bits == 64:
                # near-equal eigenvalues: float input rounding over a relative gap of 1e-3 (test_gpu_evd_subspace.py)
                assert e_p <= (1e-7 if good[b] else 1e-6), (b, s, e_p)
            else:
                # test_gpu_music.py's bound, or N float roundings over the relative gap where that is larger (an
                # N = 16 item with +-12 dB antenna gains: 2.5e-6 at a gap of 0.24)
                assert e_p <= 4 * e_ref_p + max(1e-6, N * 2.0 ** -24 / gap), (b, s, e_p, e_ref_p, gap)
            if not good[b]:
                continue                       # an ill-conditioned projector: its spectrum is not a parity quantity
            err = np.abs(q_c[b, j] - qt)
            if bits == 64:                                                                          # (b)
                assert np.all(err <= 3e-7 * np.abs(qt) + 2e-13 * mx), (b, s, (err / np.abs(qt)).max())
            else:
                # test_gpu_music.py's bounds, or 4x the fp32 oracle's own error where that is larger (a 3 dB item
                # with three sources on four antennas: the LAPACK-fp32 oracle itself is 1.2e-5 off on g1)
                r1, r1_ref = (err[g1] / qt[g1]).max(), (err_ref[g1] / qt[g1]).max()
                r2, r2_ref = (err[g2] / qt[g2]).max(), (err_ref[g2] / qt[g2]).max()
                assert r1 <= max(6e-6, 4 * r1_ref), (b, s, r1, r1_ref)
                assert r2 <= max(4e-5, 4 * r2_ref), (b, s, r2, r2_ref)
                assert err.max() <= 4 * err_ref.max() + 1e-6 * mx, (b, s)
            sp = spec_c[b, j]
            assert sp.max() == 0.0                                                                  # (d)
            fin = np.isfinite(s64[b])
            diff = (sp.astype(np.float64) - s64[b])[fin]
            if bits == 64:
                assert np.all(np.abs(diff) <= 2e-5 + 2e-6 * np.abs(s64[b][fin])), (b, s, np.abs(diff).max())
            else:
                dg = (sp.astype(np.float64) - s64[b])[g2 & fin]
                assert dg.max() - dg.min() <= 8e-4, (b, s, dg.max() - dg.min())
            want = {int(np.argmax(s64[b]))} if bits == 64 else {int(np.argmax(s64[b])), int(np.argmax(s32[b]))}  # (e)
            assert int(np.argmax(sp)) in want, (b, s, int(np.argmax(sp)), want)


# ---------------------------------------------------------------------------------------------------------------------
# Root-MUSIC and calibrate_lin_array
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,N,M", EVD_CASES)
def test_root_music_across_scales(bits, N, M):
    base, good, fb = _base_items(N, M, seed=100 * N + M + bits)
    nb, ns = base.shape[0], len(SCALES)
    mixed = _replicate(base, SCALES)
    blk = doa.rootMUSIC_linear_array(0.5, M, N)
    blk.set_internal_precision(bits)
    ang, roots, status = blk.debug(mixed)
    # bit for bit against the unscaled batch of the same layout: the root finder iterates until every item of its
    # wave has converged, so its last bits depend on the wave mates and copies of one item are compared position-wise
    ang0, roots0, status0 = blk.debug(_replicate(base, [0] * ns))
    for name, a, a0 in (("angles", ang, ang0), ("roots", roots, roots0), ("status", status, status0)):
        bad = np.nonzero(np.any(_bits(a.reshape(a.shape[0], -1)) != _bits(a0.reshape(a.shape[0], -1)), axis=1))[0]
        assert bad.size == 0, (name, bits, N, M, [SCALES[i % ns] for i in bad[:8]])
    ang_c, st_c = _per_copy(ang, ns), _per_copy(status, ns)
    for b in range(nb):
        try:
            a64 = oracle.root_music(base[b:b + 1], 0.5, M, N, "f64")[0]
        except ValueError:                     # no root strictly inside the unit circle: the item's status word
            assert np.all(st_c[b] == 1), (b, st_c[b])
            continue
        assert np.all(st_c[b] == 0), (b, st_c[b])
        # precision 32 on forward-backward items: FB makes the polynomial's roots exact pairs z, 1/conj(z), and a float
        # projector can push both members of a pair inside the circle, where the selection then takes the pair (seen at
        # N = 4, M = 3: 114.124 and 114.128 deg picked instead of 52.8 and 114.126).  Scale invariance above still holds.
        if not good[b] or (bits == 32 and fb[b]):
            continue
        tol = 1e-3
        if bits == 32:                         # float projector: no further from fp64 than twice the fp32 reference is
            a32 = oracle.root_music(base[b:b + 1], 0.5, M, N, "f32")[0]
            tol = max(tol, 2 * float(np.abs(a32.astype(np.float64) - a64).max()))
        assert np.abs(ang_c[b] - a64[None, :]).max() <= tol, (b, ang_c[b], a64, tol)


def _pilot_covariances(N, d, pilot_deg, K, n, seed, snr_db=30.0):
    # as test_gpu_calibrate.py
    rng = np.random.default_rng(seed)
    gains = np.concatenate([[1.0], rng.uniform(0.3, 1.0, N - 1)])
    phases = np.concatenate([[1.0], np.exp(-1j * np.pi * rng.uniform(0, 1, N - 1))])
    x = doa.sim.make_streams(N, n * K, [pilot_deg], d, snr_db=None, seed=seed, freqs=[1.0 / 6.0])
    x = (gains * phases)[:, None] * x
    x = x + 10 ** (-snr_db / 20) * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) / np.sqrt(2)
    return oracle.autocorrelate(x.astype(np.complex64), K, 0, 0, n)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("N,d,pilot", [(2, 0.5, 45.0), (4, 0.3, 30.0), (5, 0.4, 100.0), (8, 0.5, 60.0), (16, 0.5, 75.0)])
def test_calibrate_across_scales(N, d, pilot, bits):
    R = _pilot_covariances(N, d, pilot, 1024, 6, seed=N)
    base = np.stack([_normalise(it.reshape(N, N, order="F")) for it in R])
    nb, ns = base.shape[0], len(SCALES)
    mixed = _replicate(base, SCALES)
    blk = doa.calibrate_lin_array(d, N, pilot)
    blk.set_internal_precision(bits)
    est = np.empty((nb * ns, N), np.complex64)
    assert blk.work(nb * ns, [mixed], [est]) == nb * ns
    est_c = _per_copy(est, ns)
    for j in range(1, ns):
        assert _same_bits(est_c[:, j], est_c[:, 0]), (N, bits, SCALES[j], np.abs(est_c[:, j] - est_c[:, 0]).max())
    e0 = est_c[:, 0]
    ref64 = oracle.calibrate_normalise(oracle.calibrate_lin_array(base, d, N, pilot, "f64"))
    ref32 = oracle.calibrate_normalise(oracle.calibrate_lin_array(base, d, N, pilot, "f32"))
    assert np.all(e0[:, 0].imag == 0) and np.all(e0[:, 0].real >= 0)
    assert np.abs(np.linalg.norm(e0, axis=1) - 1).max() <= 1e-6
    dev32 = np.abs(ref32 - ref64).max()
    assert np.abs(e0 - ref64).max() <= 2e-6 + 2 * dev32, (N, bits, np.abs(e0 - ref64).max(), dev32)
    assert np.abs(e0 - ref32).max() <= 2e-6 + 2 * dev32, (N, bits, np.abs(e0 - ref32).max(), dev32)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
# (N, M, P, K): the lean shape, the quad shape, two long scans
PIPE_CASES = [(4, 1, 1024, 256), (4, 2, 1024, 256), (8, 2, 2048, 128), (16, 3, 4096, 128)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("N,M,P,K", PIPE_CASES)
def test_pipelines_across_stream_scales(N, M, P, K, bits):
    n = 96
    th = [57.3, 101.0, 140.0][:M]
    x = doa.sim.make_streams(N, n * K, th, 0.5, snr_db=15.0, seed=N + M)
    # no component below 2^-20: no product of two samples is subnormal at 2^-40 per sample
    re, im = x.real.copy(), x.imag.copy()
    re[np.abs(re) < 2.0 ** -20] = 2.0 ** -20
    im[np.abs(im) < 2.0 ** -20] = 2.0 ** -20
    x = (re + 1j * im).astype(_C64)
    pipe = doa.music_pipeline(N, K, 0, 0, 0.5, M, P)
    root = doa.root_pipeline(N, K, 0, 0, 0.5, M)
    pipe.set_internal_precision(bits)
    root.set_internal_precision(bits)

    def run(xs):
        mx, am = np.empty((n, M), np.float32), np.empty((n, M), np.float32)
        cov, spec = np.empty((n, N * N), _C64), np.empty((n, P), np.float32)
        assert pipe.work(n, [xs[k] for k in range(N)], mx, am, cov, spec) == n
        ang, rcov = np.empty((n, M), np.float32), np.empty((n, N * N), _C64)
        assert root.work(n, [xs[k] for k in range(N)], ang, rcov) == n
        assert _same_bits(rcov, cov)
        return cov, spec, mx, am, ang

    base = run(x)
    assert np.all(base[1].max(axis=1) == 0.0)
    for k in (-40, 30):
        cov, spec, mx, am, ang = run((x * np.float32(2.0 ** k)).astype(_C64))
        assert _same_bits(cov, (base[0] * np.float32(4.0 ** k)).astype(_C64)), (N, M, bits, k)
        for name, got, want in (("spectrum", spec, base[1]), ("max", mx, base[2]), ("argmax", am, base[3]),
                                ("angles", ang, base[4])):
            assert _same_bits(got, want), (name, N, M, bits, k, np.abs(got - want).max())
