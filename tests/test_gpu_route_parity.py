"""Every kernel the launch plan can select (tests/route_census.py: 66 covariance, 47 eigen and 452 scan instantiations) run
through its recipe's public call and held to the bounds the project already holds that entry to.  One case is one (stage,
kernel family, compiled size, precision) group of instantiations.

Inputs: doa.sim.make_streams with the sources spread over 25 .. 155 degrees, SNR alternating 20 / 10 dB per item, seeded from
the kernel's name; covariance items from oracle.autocorrelate, so both sides see identical items.  Before the device is judged,
every item of the fp64 reference must have min Q >= 1e-6 max Q: the condition the dB bound is stated for.

The bounds, each from the file that already tests the entry:
  K1      |R - R_f64| <= 2e-6 max|R_f64|                             tests/test_gpu_autocorrelate.py:55,74,95; sc16 against the
          widened samples                                            tests/test_gpu_sc16_autocorrelate.py:225
          sc16 bit for bit the fc32 route of the same alignment class on the widened samples   tests/test_gpu_sc16_autocorrelate.py:80
  groups  cov, row and both ports bit for bit those of work_dev, one batch at a time   tests/test_gpu_pipeline_batches.py
  64 bits (a) |P - P_f64| <= 1e-7                                    tests/test_gpu_music.py:71
          (b) |Q - Q_f64| <= 3e-7 Q + 2e-13 max Q                    tests/test_gpu_music.py:72
          (d) max exactly 0 dB, |dB - dB_f64| <= 2e-5 + 2e-6 |dB|    tests/test_gpu_music.py:80,84
          (e) arg-max equal to fp64's                                tests/test_gpu_music.py:91,95
          counts: (d), (e) per item at its own M                     tests/test_gpu_music_counts.py:44-50
          ESPRIT: status 0, |angle - reference| <= 1e-3 degrees, on gamma, gap >= 1e-4   tests/test_gpu_esprit.py:85,92-94
          MUSIC_array: (a), (b), (d), arg-max                        tests/test_gpu_array_scan.py:97-104
          calibrate: |est - ref64| <= 2e-6 + 2 |ref32 - ref64|       tests/test_gpu_calibrate.py:37
          picks: both ports are oracle.find_local_max on the pipeline's own row, bit for bit   tests/fuzz_pipeline_shapes.py:47,75
          angles only: the ports of the stored run, bit for bit
  32 bits only the forms relative to the fp32 LAPACK oracle's own distance to fp64 on the same input:
          e_P <= 4 e_ref + 1e-6                                      tests/test_gpu_music.py:75
          max|dQ| <= 4 max|dQ_ref| + 1e-6 max Q                      tests/test_gpu_music.py:78
          dB spread over Q >= 1e-2 max Q within 2 * 4e-4             tests/test_gpu_music.py:86-88
          arg-max in {fp64's, the fp32 oracle's}                     tests/test_gpu_music.py:91
          calibrate: e <= 4 e_ref + 1e-6 (the projector form on the unit-norm estimate)

Every case prints its worst figure as a fraction of its bound before it asserts (run with -s).

MEASURED on an MI355X: the file takes 5 seconds (100 tests; the slowest case 0.24 s).  Worst figure per kernel family, as a
fraction of its bound (ESPRIT's 0 is literal: the device's angles are the reference's floats):
  K1     cov_wave_kernel 0.055   cov_piece_kernel 0.056   cov_combine_kernel 0.057   cov_mfma_kernel 0.20   cov_fb_kernel 0.17
         (R; the N = 12 and 16 items in front of the wide scan kernels reach 0.30)
  eigen  music_evd_kernel                 dB 0.063, dB spread (float) 0.064
         music_evd_quad_kernel            projector 0.29, Q 0.20, dB 0.052
         music_evd_subspace_kernel        projector 0.30, Q 0.20, dB 0.058
         music_evd_group_kernel           dB spread (float) 0.027, calibration 0.011, calibration (f32 form) 0.064
         music_evd_group_counts_kernel    dB 0.051, ESPRIT angle 0
         music_evd_group_record_kernel    ESPRIT angle 0
         music_evd_group_full_kernel      projector 5.3e-8 (the full record is double), Q 0.20, dB 0.068
         music_evd_block16_kernel         dB 0.050, projector (f32 form) 0.48, Q (f32 form) 0.50, calibration 0.027
         music_evd_block16_counts_kernel  dB 0.051
         music_evd_block16_record_kernel  ESPRIT angle 0
         music_evd_block16_full_kernel    projector 4.9e-8, Q 0.20, dB 0.046
  scan   music_scan_peak1_kernel          dB 0.086, dB spread (float) 0.14
         music_scan_kernel                Q 0.20, dB 0.061, Q (f32 form) 0.60, projector (f32 form) 0.77, dB spread (float) 0.14
         music_scan_generic_kernel        dB 0.050, dB spread (float) 0.10
         music_scan_peak_long_kernel      dB 0.073
         music_scan_stream_kernel         dB 0.082
"""
import collections
import zlib

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import array_ref
import esprit_ref
import route_census as rc
from doa.sim import from_sc16, to_sc16

pytestmark = pytest.mark.gpu

D = rc.D
K_ITEM = 64
SC16_LEVEL = 0.0625                  # sc16 streams: the sources and the noise at 1/16 of full scale (2**-15 per count)
GUARD = 64                           # sentinel elements behind every device output: nothing may write there
SENTINEL = -7.0


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def case_key(r):
    name, _, args = r["kernel"].partition("<")
    args = args.rstrip(">").split(",") if args else []
    prec = "float" if "float" in args else ("double" if "double" in args else "-")
    if name in ("cov_wave_kernel", "cov_piece_kernel"):
        size = args[1]
    elif name == "music_evd_quad_kernel":
        size = "4"
    elif name.startswith("music_evd_block16"):
        size = "16"
    elif name.startswith(("music_evd_", "music_scan_")):
        size = args[0]
    else:
        size = "-"
    return "%s-%s-%s-%s" % (rc.STAGES[r["stage"]], name, size, prec)


CASES = collections.defaultdict(list)
for _stage, _recipes in sorted(rc.RECIPES.items()):
    for _kernel in sorted(_recipes):
        CASES[case_key(_recipes[_kernel])].append(_recipes[_kernel])


def seed_of(r):
    return zlib.crc32(r["kernel"].encode()) & 0x3FFFFFFF


# ---- inputs and references (no device) ---------------------------------------------------------------------------------------------
def spread(M):
    return list(esprit_ref.spread_angles(M))


def block(N, M, samples, i, seed, fmt=0):
    """item i's block of samples as the device sees it: sources at spread(M), 20 dB for even i and 10 dB for odd"""
    x = doa.sim.make_streams(N, samples, spread(max(M, 1)), D, snr_db=(20.0, 10.0)[i % 2], seed=seed)
    # sc16 streams are quantised; the reference takes the widened samples
    return np.ascontiguousarray(from_sc16(to_sc16((x * SC16_LEVEL).astype(np.complex64)))) if fmt else x


def q_ratio(q):
    q = np.asarray(q)
    return q.min(axis=-1) / q.max(axis=-1)


def ula_accept(N, Ms, P):
    """items whose fp64 null spectrum at every source count of Ms keeps min Q >= 4e-6 max Q (the device's own covariance of a
    pipeline differs from the oracle's in the last bits: a margin of four on the condition asserted later)"""
    return lambda R: np.all([q_ratio(oracle.music_lin_array(R, D, M, N, P, "f64", return_parts=True)[1]) >= 4e-6 for M in Ms], axis=0)


def items(N, M, n, seed, K=K_ITEM, accept=None, fmt=0, avg=0):
    """(streams [N, n K], covariance items [n, N*N] complex64 from oracle.autocorrelate): item i from the seed (seed + i); an item
    the fp64 reference does not accept (accept(R) -> one bool per item) is drawn again with the next seed, 4096 further on.  An
    array with one noise eigenvector (M = N - 1) has its nulls exactly on the unit circle, so how deep Q goes on the grid is a
    matter of where the grid lies, not of the snapshot size; the choice is made on the reference alone, never on the device's
    result"""
    blocks = [block(N, M, K, i, seed + i, fmt) for i in range(n)]
    for attempt in range(1, 64):
        R = oracle.autocorrelate(np.concatenate(blocks, axis=1), K, 0, avg, n)
        bad = [] if accept is None else np.flatnonzero(~np.asarray(accept(R), bool))
        if not len(bad):
            return np.ascontiguousarray(np.concatenate(blocks, axis=1)), R
        for i in bad:
            blocks[i] = block(N, M, K, i, seed + i + 4096 * attempt, fmt)
    raise AssertionError(("no conforming item", N, M, K, seed))


def k1_streams(N, step, n, K, seed, fmt):
    """[N, (n - 1) step + K]: K1 alone has no condition; a block of `step` samples per item"""
    return np.ascontiguousarray(np.concatenate([block(N, 1, step, i, seed + i, fmt) for i in range(n - 1)] + [block(N, 1, K, n - 1, seed + n - 1, fmt)], axis=1))


def conforming(q64, what):
    """the condition the dB bound is stated for, on the fp64 reference"""
    ratio = float(q_ratio(q64).min())
    assert ratio >= 1e-6, (what, ratio)


class Report:
    def __init__(self):
        self.worst = {}

    def add(self, what, value, bound=1.0):
        f = float(value) / bound
        if not f <= self.worst.get(what, -1.0):         # (a NaN replaces anything)
            self.worst[what] = f

    def text(self):
        return ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items())) or "bit-for-bit checks only"

    def ok(self):
        return all(f <= 1.0 for f in self.worst.values())


def check_spectrum(rep, spec, R, N, M, P, bits, what):
    """bounds (d), (e) in double; the reference-relative forms in float; spec [n, P] float32 of the items R"""
    s64, q64, _ = oracle.music_lin_array(R, D, M, N, P, "f64", return_parts=True)
    conforming(q64, what)
    assert np.all(spec.max(axis=1) == 0.0), (what, "the maximum is not exactly 0 dB")
    if bits == 64:
        fin = np.isfinite(s64)
        rep.add("dB", (np.abs(spec.astype(np.float64) - s64)[fin] / (2e-5 + 2e-6 * np.abs(s64[fin]))).max())
        assert np.array_equal(np.argmax(spec, axis=1), np.argmax(s64, axis=1)), (what, "arg-max")
        return
    s32 = oracle.music_lin_array(R, D, M, N, P, "f32")
    for i in range(R.shape[0]):
        g2 = (q64[i] >= 1e-2 * q64[i].max()) & np.isfinite(s64[i])
        dg = (spec[i].astype(np.float64) - s64[i])[g2]
        rep.add("dB spread", dg.max() - dg.min(), 2 * 4e-4)
        assert int(np.argmax(spec[i])) in (int(np.argmax(s64[i])), int(np.argmax(s32[i]))), (what, i, "arg-max")


def check_projector_and_q(rep, pn, q, R, N, M, P, bits, what):
    """bounds (a), (b) in double; the reference-relative forms in float"""
    _, q64, p64 = oracle.music_lin_array(R, D, M, N, P, "f64", return_parts=True)
    conforming(q64, what)
    if bits == 32:
        _, q32, p32 = oracle.music_lin_array(R, D, M, N, P, "f32", return_parts=True)
    for i in range(R.shape[0]):
        e_p = np.abs(pn[i].reshape(N, N, order="F") - p64[i]).max()
        err = np.abs(q[i] - q64[i])
        mx = q64[i].max()
        if bits == 64:
            rep.add("projector", e_p, 1e-7)
            rep.add("Q", (err / (3e-7 * np.abs(q64[i]) + 2e-13 * mx)).max())
        else:
            rep.add("projector (f32 form)", e_p, 4 * np.abs(p32[i] - p64[i]).max() + 1e-6)
            rep.add("Q (f32 form)", err.max(), 4 * np.abs(q32[i] - q64[i]).max() + 1e-6 * mx)


def check_cov(rep, got, x, K, ovl, avg, n):
    ref = oracle.autocorrelate(x, K, ovl, avg, n, precision="f64")
    rep.add("R", np.abs(got - ref).max(), 2e-6 * np.abs(ref).max())


def check_peaks(spec, mx, am, M, P, what):
    v0, v1 = oracle.find_local_max(spec, M, P, 0.0, 180.0)
    assert same(mx, v0) and same(am, v1), (what, "the ports are not find_local_max of the pipeline's own row")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- device plumbing -------------------------------------------------------------------------------------------------------------
class Out:
    """a device output of `count` elements behind `offset` bytes, with sentinels in front of and behind it"""

    def __init__(self, count, dtype=torch.float32, offset=0):
        self.count, self.lead = count, GUARD
        self.esize = torch.empty(0, dtype=dtype).element_size()
        assert offset % self.esize == 0
        self.shift = offset // self.esize
        self.buf = torch.full((self.lead + self.shift + count + GUARD,), SENTINEL if dtype != torch.int32 else -7, dtype=dtype, device="cuda")
        self.ptr = self.buf.data_ptr() + (self.lead + self.shift) * self.esize

    def get(self, shape):
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        lo = self.lead + self.shift
        guard = np.concatenate([a[:lo], a[lo + self.count:]])
        assert np.all(guard == guard.dtype.type(SENTINEL)), "a write outside the output"
        return a[lo:lo + self.count].reshape(shape)


def stream_ptrs(x, fmt, off, keep):
    """device copies of the streams [N, T] (sc16: the int16 pairs), each `off` samples past a 256-byte boundary"""
    ptrs = []
    for row in (to_sc16(x) if fmt else x):
        raw = np.ascontiguousarray(row).view(np.uint8).reshape(-1)
        sb = 4 if fmt else 8
        buf = torch.zeros(raw.size + 512, dtype=torch.uint8, device="cuda")
        base = (-buf.data_ptr()) % 256 + off * sb
        buf[base:base + raw.size].copy_(torch.from_numpy(raw))
        ptrs.append(buf.data_ptr() + base)
        keep.append(buf)
    return ptrs


# ---- the entries -----------------------------------------------------------------------------------------------------------------
def run_autocorrelate(r, rep):
    a = r["args"]
    N, K, ovl, n = a["N"], a["K"], a["ovl"], a["n"]
    S = K - ovl
    x = k1_streams(N, S, n, K, seed_of(r), a["fmt"])
    keep = []
    blk = (doa.autocorrelate_sc16 if a["fmt"] else doa.autocorrelate)(N, K, ovl, a["avg"])
    out = Out(n * N * N * 2)
    assert blk.work_dev(n, stream_ptrs(x, a["fmt"], a["off"], keep), out.ptr, torch.cuda.current_stream()) == n
    got = out.get((n, N * N * 2)).view(np.complex64)
    check_cov(rep, got, x, K, ovl, a["avg"], n)
    blk.close()
    if a["fmt"]:        # the fc32 route of the same alignment class on the widened samples: the same bits (tests/test_gpu_sc16_autocorrelate.py:80)
        blk, out = doa.autocorrelate(N, K, ovl, a["avg"]), Out(n * N * N * 2)
        assert blk.work_dev(n, stream_ptrs(x, 0, a["off"], keep), out.ptr, torch.cuda.current_stream()) == n
        assert same(out.get((n, N * N * 2)).view(np.complex64), got), (r["kernel"], "sc16 differs from fc32 on the widened samples")
        blk.close()


def music_block(a):
    blk = doa.MUSIC_lin_array(D, a["M"], a["N"], a["P"])
    blk.set_internal_precision(a["bits"])
    return blk


def run_music_work_dev(r, rep):
    a = r["args"]
    N, M, P, n = a["N"], a["M"], a["P"], a["n"]
    _, R = items(N, M, n, seed_of(r), accept=ula_accept(N, [M], P))
    blk = music_block(a)
    dR = torch.from_numpy(np.array(R)).cuda()
    out = Out(n * P, offset=a["off"])
    assert blk.work_dev(n, dR.data_ptr(), out.ptr, torch.cuda.current_stream()) == n
    check_spectrum(rep, out.get((n, P)), R, N, M, P, a["bits"], r["kernel"])
    blk.close()


def run_music_debug(r, rep):
    a = r["args"]
    N, M, P, n = a["N"], a["M"], a["P"], a["n"]
    _, R = items(N, M, n, seed_of(r), accept=ula_accept(N, [M], P))
    blk = music_block(a)
    pn, q = blk.debug(np.array(R))
    check_projector_and_q(rep, pn, q, R, N, M, P, a["bits"], r["kernel"])
    blk.close()


def run_music_counts(r, rep):
    """a count per item, cycling over 1 .. the number of sources; every item against the oracle at its own count"""
    a = r["args"]
    N, P, n = a["N"], a["P"], a["n"]
    M_true = min(2, N - 1)
    _, R = items(N, M_true, n, seed_of(r), accept=ula_accept(N, range(1, M_true + 1), P))
    counts = (1 + np.arange(n) % M_true).astype(np.int32)
    blk = music_block(a)
    dR, dc = torch.from_numpy(np.array(R)).cuda(), torch.from_numpy(counts).cuda()
    out = Out(n * P)
    assert blk.work_dev_counts(n, dR.data_ptr(), dc.data_ptr(), out.ptr, torch.cuda.current_stream()) == n
    spec = out.get((n, P))
    for m in range(1, M_true + 1):
        check_spectrum(rep, spec[counts == m], R[counts == m], N, m, P, a["bits"], (r["kernel"], m))
    blk.close()


def run_root_esprit_auto(r, rep):
    a = r["args"]
    N, M, K, n = a["N"], a["M"], a["K"], a["n"]
    def accept(R):
        ok = np.ones(R.shape[0], bool)
        for m in range(1, M + 1):
            _, st_ref, gamma, gap = esprit_ref.esprit(R, D, m, N)
            ok &= (st_ref == 0) & (gamma >= 4e-4) & (gap >= 4e-4)
        return ok
    x, _ = items(N, M, n, seed_of(r), K, accept)
    keep = []
    pipe = doa.root_pipeline(N, K, 0, 0, D, M, max_batch=n)
    pipe.set_estimator("esprit")
    ang, cnt, cov, st = Out(n * M), Out(n, torch.int32), Out(n * N * N * 2), Out(n, torch.int32)
    assert pipe.work_dev_auto(n, stream_ptrs(x, 0, 0, keep), ang.ptr, cnt.ptr, "mdl", cov.ptr, None, st.ptr, torch.cuda.current_stream()) == n
    R = cov.get((n, N * N * 2)).view(np.complex64)
    check_cov(rep, R, x, K, 0, 0, n)
    counts, angles, status = cnt.get((n,)), ang.get((n, M)), st.get((n,))
    assert counts.min() >= 0 and counts.max() <= M and (counts > 0).any(), counts
    for m in range(1, M + 1):
        sel = counts == m
        if not sel.any():
            continue
        a_ref, st_ref, gamma, gap = esprit_ref.esprit(R[sel], D, m, N)
        assert np.all(st_ref == 0) and gamma.min() >= 1e-4 and gap.min() >= 1e-4, (r["kernel"], m, gamma.min(), gap.min())
        assert np.all(status[sel] == 0) and np.all(np.isnan(angles[sel][:, m:]))
        rep.add("ESPRIT angle", np.abs(angles[sel][:, :m].astype(np.float64) - a_ref).max(), 1e-3)
    assert np.all(np.isnan(angles[counts == 0]))
    pipe.close()


def run_esprit(r, rep):
    a = r["args"]
    N, M, n = a["N"], a["M"], a["n"]
    def accept(R):
        _, st_ref, gamma, gap = esprit_ref.esprit(R, D, M, N)
        return (st_ref == 0) & (gamma >= 1e-4) & (gap >= 1e-4)
    _, R = items(N, M, n, seed_of(r), accept=accept)
    a_ref, st_ref, gamma, gap = esprit_ref.esprit(R, D, M, N)
    assert np.all(st_ref == 0) and gamma.min() >= 1e-4 and gap.min() >= 1e-4, (r["kernel"], gamma.min(), gap.min())
    blk = doa.esprit_linear_array(D, M, N)
    dR = torch.from_numpy(np.array(R)).cuda()
    ang, st = Out(n * M), Out(n, torch.int32)
    assert blk.work_dev(n, dR.data_ptr(), ang.ptr, st.ptr, torch.cuda.current_stream()) == n
    got = ang.get((n, M))
    assert np.all(st.get((n,)) == 0) and not np.isnan(got).any()
    rep.add("ESPRIT angle", np.abs(got.astype(np.float64) - a_ref).max(), 1e-3)
    blk.close()


def run_music_array(r, rep):
    """the steering table of the same uniform linear array on a 96-direction grid: the definition is tests/array_ref.py's"""
    a = r["args"]
    N, M, n, P = a["N"], a["M"], a["n"], 96
    table = np.ascontiguousarray(doa.sim.manifold(D, N, np.arange(P) * 180.0 / P).T)
    _, R = items(N, M, n, seed_of(r), accept=lambda R: q_ratio(array_ref.music(R, table, M)[1]) >= 1e-6)
    s_ref, q_ref, X_ref = array_ref.music(R, table, M)
    conforming(q_ref, r["kernel"])
    blk = doa.MUSIC_array(M, table)
    dR = torch.from_numpy(np.array(R)).cuda()
    out = Out(n * P)
    assert blk.work_dev(n, dR.data_ptr(), out.ptr, torch.cuda.current_stream()) == n
    spec = out.get((n, P))
    X, q = blk.debug(np.array(R))
    for i in range(n):
        rep.add("projector", np.abs(X[i].reshape(N, N, order="F") - X_ref[i]).max(), 1e-7)
        rep.add("Q", (np.abs(q[i] - q_ref[i]) / (3e-7 * np.abs(q_ref[i]) + 2e-13 * q_ref[i].max())).max())
        rep.add("dB", (np.abs(spec[i] - s_ref[i]) / (2e-5 + 2e-6 * np.abs(s_ref[i]))).max())
    assert np.all(spec.max(axis=1) == 0.0)
    assert np.array_equal(np.argmax(spec, axis=1), np.argmax(s_ref, axis=1))
    blk.close()


def run_calibrate(r, rep):
    from test_gpu_calibrate import _pilot_covariances
    a = r["args"]
    N, n, pilot = a["N"], a["n"], 60.0
    _, R = _pilot_covariances(N, D, pilot, 1024, n, seed=seed_of(r))
    blk = doa.calibrate_lin_array(D, N, pilot)
    blk.set_internal_precision(a["bits"])
    dR = torch.from_numpy(np.ascontiguousarray(R)).cuda()
    out = Out(n * N * 2)
    assert blk.work_dev(n, dR.data_ptr(), out.ptr, torch.cuda.current_stream()) == n
    est = out.get((n, N * 2)).view(np.complex64)
    ref64 = oracle.calibrate_normalise(oracle.calibrate_lin_array(R, D, N, pilot, "f64"))
    ref32 = oracle.calibrate_normalise(oracle.calibrate_lin_array(R, D, N, pilot, "f32"))
    dev32 = np.abs(ref32 - ref64).max()
    if a["bits"] == 64:
        rep.add("calibration", np.abs(est - ref64).max(), 2e-6 + 2 * dev32)
    else:
        rep.add("calibration (f32 form)", np.abs(est - ref64).max(), 4 * dev32 + 1e-6)
    blk.close()


def pipeline_outputs(pipe, n, ptrs, N, M, P, store):
    cov, spec, mx, am = Out(n * N * N * 2), Out(n * P) if store else None, Out(n * M), Out(n * M)
    assert pipe.work_dev(n, ptrs, cov.ptr, spec.ptr if store else None, mx.ptr, am.ptr, torch.cuda.current_stream()) == n
    return cov.get((n, N * N * 2)).view(np.complex64), spec.get((n, P)) if store else None, mx.get((n, M)), am.get((n, M))


def run_pipeline(r, rep):
    a = r["args"]
    N, M, P, K, n, bits = a["N"], a["M"], a["P"], a["K"], a["n"], a["bits"]
    x, _ = items(N, M, n, seed_of(r), K, ula_accept(N, [M], P))
    keep = []
    ptrs = stream_ptrs(x, 0, 0, keep)
    pipe = doa.music_pipeline(N, K, 0, 0, D, M, P, max_batch=n)
    pipe.set_internal_precision(bits)
    cov, spec, mx, am = pipeline_outputs(pipe, n, ptrs, N, M, P, True)
    check_cov(rep, cov, x, K, 0, 0, n)
    check_spectrum(rep, spec, cov, N, M, P, bits, r["kernel"])
    check_peaks(spec, mx, am, M, P, r["kernel"])
    if not a["store"]:              # angles only: the stored run's ports
        cov2, _, mx2, am2 = pipeline_outputs(pipe, n, ptrs, N, M, P, False)
        assert same(cov2, cov) and same(mx2, mx) and same(am2, am), (r["kernel"], "angles only differs from the stored run")
    pipe.close()


def run_batches(r, rep):
    """a group of batches against the same batches through work_dev one at a time, bit for bit; those against the oracle"""
    a = r["args"]
    N, M, P, K, n, nb, fmt, store = a["N"], a["M"], a["P"], a["K"], a["n"], a["nb"], a["fmt"], a["store"]
    x, _ = items(N, M, nb * n, seed_of(r), K, ula_accept(N, [M], P), fmt, a["avg"])
    keep = []
    base = stream_ptrs(x, fmt, a["off"], keep)
    sb = 4 if fmt else 8
    ins = [[p + b * n * K * sb for p in base] for b in range(nb)]
    make = doa.music_pipeline_sc16 if fmt else doa.music_pipeline
    pipe = make(N, K, 0, a["avg"], D, M, P, max_batch=n)
    pipe.set_lanes(1)
    cov, spec = [Out(n * N * N * 2) for _ in range(nb)], [Out(n * P) for _ in range(nb)] if store else None
    mx, am = [Out(n * M) for _ in range(nb)], [Out(n * M) for _ in range(nb)]
    pipe.work_dev_batches(n, ins, [o.ptr for o in cov], [o.ptr for o in spec] if store else None, [o.ptr for o in mx], [o.ptr for o in am])
    pipe.synchronize()
    one = make(N, K, 0, a["avg"], D, M, P, max_batch=n)
    for b in range(nb):
        w_cov, w_spec, w_mx, w_am = pipeline_outputs(one, n, ins[b], N, M, P, True)
        xb = x[:, b * n * K:(b + 1) * n * K]
        check_cov(rep, w_cov, xb, K, 0, a["avg"], n)
        check_spectrum(rep, w_spec, w_cov, N, M, P, 64, r["kernel"])
        check_peaks(w_spec, w_mx, w_am, M, P, r["kernel"])
        assert same(cov[b].get((n, N * N * 2)).view(np.complex64), w_cov), (r["kernel"], b, "covariance")
        assert same(mx[b].get((n, M)), w_mx) and same(am[b].get((n, M)), w_am), (r["kernel"], b, "ports")
        if store:
            assert same(spec[b].get((n, P)), w_spec), (r["kernel"], b, "row")
    pipe.close()
    one.close()


RUN = {"autocorrelate.work_dev": run_autocorrelate, "MUSIC_lin_array.work_dev": run_music_work_dev, "MUSIC_lin_array.debug": run_music_debug,
       "MUSIC_lin_array.work_dev_counts": run_music_counts, "root_pipeline[esprit].work_dev_auto": run_root_esprit_auto,
       "esprit_linear_array.work_dev": run_esprit, "MUSIC_array.work_dev": run_music_array, "calibrate_lin_array.work_dev": run_calibrate,
       "music_pipeline.work_dev": run_pipeline, "music_pipeline.work_dev_batches": run_batches}


def test_every_census_kernel_is_in_a_case():
    assert sum(len(v) for v in CASES.values()) == 565
    assert {r["kernel"] for v in CASES.values() for r in v} == {k for kernels in rc.census().values() for k in kernels}
    assert all(r["entry"] in RUN for v in CASES.values() for r in v)


@pytest.mark.parametrize("key", sorted(CASES))
def test_route_parity(key):
    torch.cuda.set_device(0)
    total = Report()
    done = set()
    for r in CASES[key]:
        call = (r["entry"], tuple(sorted(r["args"].items())))
        if call in done:                # (two kernels of one call: the piece kernel and its combine pass)
            continue
        done.add(call)
        rep = Report()
        RUN[r["entry"]](r, rep)
        print("%s  <- %s %s: %s" % (r["kernel"], r["entry"], r["args"], rep.text()))
        assert rep.ok(), (r["kernel"], r["entry"], r["args"], rep.worst)
        for what, f in rep.worst.items():
            total.add(what, f)
    print("%s: worst fractions of the bounds: %s" % (key, total.text()))
