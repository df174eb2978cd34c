"""The cases behind tests/golden/gridfree_refusals.json and tests/golden/gridfree_chain_bits.npz, shared by the scripts that
record them (tests/golden/make_gridfree_golden.py) and the tests that replay them (test_cpu_gridfree_refusals.py,
test_gpu_gridfree_refusals.py, test_gpu_gridfree_chain.py): the grid-free estimators' entries (rootMUSIC_linear_array,
esprit_linear_array, root_pipeline) and the seven thin entries that music_pipeline shares with root_pipeline.

Refusals: every case is a call that an entry refuses before it touches the device, recorded as (return code, doa_last_error()
text).  Bits: seeded inputs through every form of the three handles, outputs kept as raw 32-bit words."""
import ctypes as C

import numpy as np

from doa import _lib

MDL, AIC = 0, 1
ROOT_MUSIC, ESPRIT = 0, 1

# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
_HOST = (C.c_char * 4096)()                     # a pointer that is not NULL; a refused call never follows it
P = C.addressof(_HOST)
Z = None
H = "H"                                         # replaced by the case's handle


def _pp(*ptrs):
    return _lib.ptr_array([p or 0 for p in ptrs])


PP = _pp(*[P] * 16)

# kind -> (create, destroy); a kind's options are applied in this order: the process precision at create, the handle's
# precision, the estimator
_KINDS = {
    "root": (lambda K: _lib.lib.doa_rootMUSIC_linear_array_create(0.5, 2, 4), "doa_rootMUSIC_linear_array_destroy"),
    "esprit": (lambda K: _lib.lib.doa_esprit_linear_array_create(0.5, 2, 4), "doa_esprit_linear_array_destroy"),
    "rootpipe": (lambda K: _lib.lib.doa_root_pipeline_create(4, K, 0, 0, 0.5, 2, 8), "doa_root_pipeline_destroy"),
    "musicpipe": (lambda K: _lib.lib.doa_music_pipeline_create(4, K, 0, 0, 0.5, 1, 64, 8), "doa_music_pipeline_destroy"),
}
_SET_BITS = {"root": "doa_rootMUSIC_linear_array_set_internal_precision", "rootpipe": "doa_root_pipeline_set_internal_precision"}


def _refusal_table():
    """[(name, kind or None, options, entry, args)]; kind None: no handle, no device"""
    t = []

    def add(name, kind, fn, *args, **opt):
        t.append((name, kind, opt, fn, args))

    R = "doa_rootMUSIC_linear_array_"
    for kind, h in ((None, Z), ("root", H)):
        tag = "null" if h is Z else "h"
        q = P if h is Z else Z                              # with a handle, each case takes one pointer away
        add(f"root.work.{tag}", kind, R + "work", h, 1, q, P)
        add(f"root.work_dev.{tag}", kind, R + "work_dev", h, 1, q, P, Z)
        add(f"root.work_counts.{tag}", kind, R + "work_counts", h, 1, P, q, P)
        add(f"root.work_dev_counts.{tag}", kind, R + "work_dev_counts", h, 1, P, q, P, Z, Z)
        add(f"root.debug.{tag}", kind, R + "debug", h, 1, q, P, P, P)
        add(f"root.select_debug.{tag}", kind, R + "select_debug", h, 1, q, P, P)
        add(f"root.select_counts_debug.{tag}", kind, R + "select_counts_debug", h, 1, P, q, P, P)
        add(f"root.set_internal_precision.{tag}", kind, R + "set_internal_precision", h, 64 if h is Z else 16)
    add("root.work.no_out", "root", R + "work", H, 1, P, Z)
    add("root.work_dev.no_out", "root", R + "work_dev", H, 1, P, Z, Z)
    add("root.work_dev.negative", "root", R + "work_dev", H, -1, P, P, Z)
    add("root.work_dev_counts.no_out", "root", R + "work_dev_counts", H, 1, P, P, Z, Z, Z)
    add("root.debug.no_items", "root", R + "debug", H, 0, P, P, P, P)
    add("root.work_counts.bits32", "root", R + "work_counts", H, 1, P, P, P, bits=32)
    add("root.work_dev_counts.bits32", "root", R + "work_dev_counts", H, 1, P, P, P, Z, Z, bits=32)
    add("root.work_dev_counts.bits32+no_out", "root", R + "work_dev_counts", H, 1, P, P, Z, Z, Z, bits=32)
    add("root.work_dev_counts.bits32+no_counts", "root", R + "work_dev_counts", H, 1, P, Z, P, Z, Z, bits=32)
    add("root.work_counts.bits32+negative", "root", R + "work_counts", H, -1, P, P, P, bits=32)
    add("root.work_counts.bits32+no_items", "root", R + "work_counts", H, 0, Z, Z, Z, bits=32)

    E = "doa_esprit_linear_array_"
    for kind, h in ((None, Z), ("esprit", H)):
        tag = "null" if h is Z else "h"
        q = P if h is Z else Z
        add(f"esprit.work.{tag}", kind, E + "work", h, 1, q, P, Z)
        add(f"esprit.work_dev.{tag}", kind, E + "work_dev", h, 1, q, P, Z, Z)
        add(f"esprit.work_counts.{tag}", kind, E + "work_counts", h, 1, P, q, P, Z)
        add(f"esprit.work_dev_counts.{tag}", kind, E + "work_dev_counts", h, 1, P, q, P, Z, Z)
        add(f"esprit.record_debug.{tag}", kind, E + "record_debug", h, 1, P, q, Z, P, P)
    add("esprit.work.no_out", "esprit", E + "work", H, 1, P, Z, Z)
    add("esprit.work_dev.no_out", "esprit", E + "work_dev", H, 1, P, Z, Z, Z)
    add("esprit.record_debug.no_items", "esprit", E + "record_debug", H, 0, P, P, Z, P, P)
    add("esprit.work.bits32", "esprit", E + "work", H, 1, P, P, Z, create_bits=32)
    add("esprit.work_dev.bits32", "esprit", E + "work_dev", H, 1, P, P, Z, Z, create_bits=32)
    add("esprit.work_counts.bits32", "esprit", E + "work_counts", H, 1, P, P, P, Z, create_bits=32)
    add("esprit.work_dev_counts.bits32", "esprit", E + "work_dev_counts", H, 1, P, P, P, Z, Z, create_bits=32)
    add("esprit.record_debug.bits32", "esprit", E + "record_debug", H, 1, P, P, Z, P, P, create_bits=32)
    add("esprit.work.bits32+no_out", "esprit", E + "work", H, 1, P, Z, Z, create_bits=32)
    add("esprit.work_dev.bits32+no_out", "esprit", E + "work_dev", H, 1, P, Z, Z, Z, create_bits=32)
    add("esprit.work_counts.bits32+no_counts", "esprit", E + "work_counts", H, 1, P, Z, P, Z, create_bits=32)
    add("esprit.work_dev.bits32+no_items", "esprit", E + "work_dev", H, 0, Z, Z, Z, Z, create_bits=32)
    add("esprit.record_debug.bits32+no_items", "esprit", E + "record_debug", H, 0, P, P, Z, P, P, create_bits=32)

    # the seven entries the two pipeline handles share
    for pre, kind in (("music_pipeline", "musicpipe"), ("root_pipeline", "rootpipe")):
        D = f"doa_{pre}_"
        add(f"{pre}.fuse_antenna_correction.null", None, D + "fuse_antenna_correction", Z, P)
        add(f"{pre}.set_input_format.null", None, D + "set_input_format", Z, 0, 1.0)
        add(f"{pre}.set_lanes.null", None, D + "set_lanes", Z, 2)
        add(f"{pre}.set_lane_streams.null", None, D + "set_lane_streams", Z, 2, PP)
        add(f"{pre}.synchronize.null", None, D + "synchronize", Z)
        add(f"{pre}.inject_failure.null", None, D + "inject_failure", Z, 0)
        add(f"{pre}.lanes_idle.null", None, D + "lanes_idle", Z)
        add(f"{pre}.set_input_format.null+format", None, D + "set_input_format", Z, 7, -1.0)
        add(f"{pre}.set_lanes.null+count", None, D + "set_lanes", Z, 0)
        add(f"{pre}.set_lane_streams.null+count+streams", None, D + "set_lane_streams", Z, 0, Z)
        add(f"{pre}.inject_failure.null+index", None, D + "inject_failure", Z, -2)
        add(f"{pre}.set_input_format.format", kind, D + "set_input_format", H, 7, 1.0)
        add(f"{pre}.set_input_format.scale", kind, D + "set_input_format", H, 1, -1.0)
        add(f"{pre}.set_lanes.zero", kind, D + "set_lanes", H, 0)
        add(f"{pre}.set_lanes.many", kind, D + "set_lanes", H, 99)
        add(f"{pre}.set_lane_streams.zero", kind, D + "set_lane_streams", H, 0, PP)
        add(f"{pre}.set_lane_streams.no_streams", kind, D + "set_lane_streams", H, 1, Z)
        add(f"{pre}.set_lane_streams.many+no_streams", kind, D + "set_lane_streams", H, 99, Z)
        add(f"{pre}.inject_failure.index", kind, D + "inject_failure", H, -2)

    Q = "doa_root_pipeline_"
    add("root_pipeline.set_spatial_smoothing.null", None, Q + "set_spatial_smoothing", Z, 0, 0)
    add("root_pipeline.set_estimator.null", None, Q + "set_estimator", Z, ROOT_MUSIC)
    add("root_pipeline.work_dev.null", None, Q + "work_dev", Z, 1, PP, Z, P, Z, Z)
    add("root_pipeline.work_dev_auto.null", None, Q + "work_dev_auto", Z, 1, PP, MDL, Z, P, P, Z, Z, Z)
    add("root_pipeline.work_dev_batches.null", None, Q + "work_dev_batches", Z, 1, 1, PP, Z, PP, Z, Z)
    add("root_pipeline.work.null", None, Q + "work", Z, 1, PP, Z, P)
    add("root_pipeline.set_internal_precision.null", None, Q + "set_internal_precision", Z, 64)
    k = "rootpipe"
    add("root_pipeline.set_spatial_smoothing.one", k, Q + "set_spatial_smoothing", H, 1, 0)
    add("root_pipeline.set_spatial_smoothing.small", k, Q + "set_spatial_smoothing", H, 2, 1)
    add("root_pipeline.set_estimator.unknown", k, Q + "set_estimator", H, 5)
    add("root_pipeline.set_internal_precision.bits16", k, Q + "set_internal_precision", H, 16)
    add("root_pipeline.work_dev.no_in", k, Q + "work_dev", H, 1, Z, Z, P, Z, Z)
    add("root_pipeline.work_dev.no_out", k, Q + "work_dev", H, 1, PP, Z, Z, Z, Z)
    add("root_pipeline.work_dev.negative", k, Q + "work_dev", H, -1, PP, Z, P, Z, Z)
    add("root_pipeline.work_dev_auto.no_in", k, Q + "work_dev_auto", H, 1, Z, MDL, Z, P, P, Z, Z, Z)
    add("root_pipeline.work_dev_auto.no_out", k, Q + "work_dev_auto", H, 1, PP, MDL, Z, Z, P, Z, Z, Z)
    add("root_pipeline.work_dev_auto.no_counts", k, Q + "work_dev_auto", H, 1, PP, AIC, Z, P, Z, Z, Z, Z)
    add("root_pipeline.work_dev_auto.method", k, Q + "work_dev_auto", H, 1, PP, 2, Z, P, P, Z, Z, Z)
    add("root_pipeline.work_dev_batches.no_in", k, Q + "work_dev_batches", H, 1, 1, Z, Z, PP, Z, Z)
    add("root_pipeline.work_dev_batches.no_out", k, Q + "work_dev_batches", H, 1, 1, PP, Z, Z, Z, Z)
    add("root_pipeline.work_dev_batches.batch_no_out", k, Q + "work_dev_batches", H, 2, 1, PP, Z, _pp(P, Z), Z, Z)
    add("root_pipeline.work.no_in", k, Q + "work", H, 1, Z, Z, P)
    add("root_pipeline.work.no_out", k, Q + "work", H, 1, PP, Z, Z)
    add("root_pipeline.work.stream_null", k, Q + "work", H, 1, _pp(P, Z, P, P), Z, P)
    # noutput_items > max_batch
    add("root_pipeline.work_dev.over", k, Q + "work_dev", H, 9, PP, Z, P, Z, Z)
    add("root_pipeline.work_dev_auto.over", k, Q + "work_dev_auto", H, 9, PP, MDL, Z, P, P, Z, Z, Z)
    add("root_pipeline.work_dev_batches.over", k, Q + "work_dev_batches", H, 1, 9, PP, Z, PP, Z, Z)
    add("root_pipeline.work.over", k, Q + "work", H, 9, PP, Z, P)
    # ESPRIT mode at 32 bits; the counted entry at 32 bits
    e32 = dict(bits=32, estimator=ESPRIT)
    add("root_pipeline.work_dev.esprit32", k, Q + "work_dev", H, 1, PP, Z, P, Z, Z, **e32)
    add("root_pipeline.work_dev_batches.esprit32", k, Q + "work_dev_batches", H, 1, 1, PP, Z, PP, Z, Z, **e32)
    add("root_pipeline.work.esprit32", k, Q + "work", H, 1, PP, Z, P, **e32)
    add("root_pipeline.work_dev_auto.esprit32", k, Q + "work_dev_auto", H, 1, PP, MDL, Z, P, P, Z, Z, Z, **e32)
    add("root_pipeline.work_dev_auto.bits32", k, Q + "work_dev_auto", H, 1, PP, MDL, Z, P, P, Z, Z, Z, bits=32)
    add("root_pipeline.work_dev_auto.snapshot1", k, Q + "work_dev_auto", H, 1, PP, MDL, Z, P, P, Z, Z, Z, K=1)
    add("root_pipeline.work_dev_auto.esprit+snapshot1", k, Q + "work_dev_auto", H, 1, PP, AIC, Z, P, P, Z, Z, Z, K=1, estimator=ESPRIT)
    # two rules broken at once: which one is reported
    add("root_pipeline.work_dev.over+esprit32", k, Q + "work_dev", H, 9, PP, Z, P, Z, Z, **e32)
    add("root_pipeline.work_dev.no_out+esprit32", k, Q + "work_dev", H, 1, PP, Z, Z, Z, Z, **e32)
    add("root_pipeline.work_dev.no_items+esprit32", k, Q + "work_dev", H, 0, PP, Z, Z, Z, Z, **e32)
    add("root_pipeline.work_dev_batches.over+esprit32", k, Q + "work_dev_batches", H, 1, 9, PP, Z, PP, Z, Z, **e32)
    add("root_pipeline.work_dev_batches.batch_no_out+esprit32", k, Q + "work_dev_batches", H, 2, 1, PP, Z, _pp(P, Z), Z, Z, **e32)
    add("root_pipeline.work_dev_batches.no_batches+esprit32", k, Q + "work_dev_batches", H, 0, 1, PP, Z, PP, Z, Z, **e32)
    add("root_pipeline.work.over+esprit32", k, Q + "work", H, 9, PP, Z, P, **e32)
    add("root_pipeline.work.no_items+esprit32", k, Q + "work", H, 0, PP, Z, Z, **e32)
    add("root_pipeline.work_dev_auto.no_out+bits32", k, Q + "work_dev_auto", H, 1, PP, MDL, Z, Z, P, Z, Z, Z, bits=32)
    add("root_pipeline.work_dev_auto.method+over", k, Q + "work_dev_auto", H, 9, PP, 2, Z, P, P, Z, Z, Z)
    add("root_pipeline.work_dev_auto.over+bits32", k, Q + "work_dev_auto", H, 9, PP, MDL, Z, P, P, Z, Z, Z, bits=32)
    add("root_pipeline.work_dev_auto.bits32+snapshot1", k, Q + "work_dev_auto", H, 1, PP, MDL, Z, P, P, Z, Z, Z, bits=32, K=1)
    add("root_pipeline.work_dev_auto.snapshot1+no_items", k, Q + "work_dev_auto", H, 0, PP, MDL, Z, Z, Z, Z, Z, Z, K=1)
    assert len({c[0] for c in t}) == len(t)
    return t


REFUSALS = _refusal_table()
REFUSALS_CPU = [c[0] for c in REFUSALS if c[1] is None]
REFUSALS_GPU = [c[0] for c in REFUSALS if c[1] is not None]


def run_refusal(name):
    """-> [return code, doa_last_error() text] of the case; every case must be refused"""
    _, kind, opt, fn, args = next(c for c in REFUSALS if c[0] == name)
    lib = _lib.lib
    h = None
    if kind:
        create, destroy = _KINDS[kind]
        if "create_bits" in opt: assert lib.doa_set_internal_precision(opt["create_bits"]) == 0
        try:
            h = create(opt.get("K", 16))
        finally:
            if "create_bits" in opt: assert lib.doa_set_internal_precision(64) == 0
        assert h, _lib.last_error()
    try:
        if "bits" in opt: assert getattr(lib, _SET_BITS[kind])(h, opt["bits"]) == 0
        if "estimator" in opt: assert lib.doa_root_pipeline_set_estimator(h, opt["estimator"]) == 0, _lib.last_error()
        rc = getattr(lib, fn)(*[h if a is H else a for a in args])
        text = _lib.last_error()
    finally:
        if h: getattr(lib, destroy)(h)
    assert rc < 0, (name, rc)
    return [rc, text]


# ---------------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------------
SIZES = (2, 3, 4, 5, 8, 9, 16)          # the one-lane, 8-lane and block eigen kernels; root degrees 2, 4, 6, 8, 14, 16, 30
N_ITEMS, ZERO_ITEM, NAN_ITEM = 19, 7, 11
K_SNAP = 24                             # samples per snapshot (no overlap): at least the largest array, so items have full rank
SPACING = 0.5
SMOOTHED = (8, 5, 1, 2)                 # N, subarray size, forward-backward, num_targets
SHAPES = [(N, M) for N in SIZES for M in sorted({1, min(N - 1, 3)})]


def make_inputs(seed=20250611):
    """{x<N>: int16 [N, (N_ITEMS + 1) K_SNAP, 2] samples (value = (re + j im) 2^-10), R<N>: complex64 [N_ITEMS, N N] items}:
    two sources and noise rounded to integers, snapshot ZERO_ITEM all zeros; the items are the snapshots' sample covariances
    formed in integers (so they do not depend on a BLAS), with item NAN_ITEM all NaN (in the streams: one NaN sample)."""
    rng = np.random.default_rng(seed)
    out = {}
    for N in SIZES:
        T = (N_ITEMS + 1) * K_SNAP
        th = np.deg2rad([52.0, 101.0][: max(1, min(2, N - 1))])
        a = np.exp(-2j * np.pi * SPACING * np.cos(th)[None, :] * np.arange(N)[:, None])
        s = (rng.standard_normal((len(th), T)) + 1j * rng.standard_normal((len(th), T))) * np.array([300.0, 200.0])[: len(th), None]
        x = a @ s + 40.0 * (rng.standard_normal((N, T)) + 1j * rng.standard_normal((N, T)))
        q = np.stack([np.rint(x.real), np.rint(x.imag)], axis=-1).astype(np.int16)
        q[:, ZERO_ITEM * K_SNAP:(ZERO_ITEM + 1) * K_SNAP] = 0
        out[f"x{N}"] = q
        R = np.empty((N_ITEMS, N * N), np.complex64)
        for i in range(N_ITEMS):
            w = q[:, i * K_SNAP:(i + 1) * K_SNAP].astype(np.int64)
            re, im = w[..., 0], w[..., 1]
            rr = re @ re.T + im @ im.T                       # x x^H, exact
            ii = im @ re.T - re @ im.T
            Ri = (rr.astype(np.float64) + 1j * ii.astype(np.float64)) / float(K_SNAP << 20)
            R[i] = Ri.T.reshape(-1).astype(np.complex64)     # column-major
        R[NAN_ITEM] = complex(np.nan, np.nan)
        out[f"R{N}"] = R
    return out


def streams(inputs, N):
    """complex64 [N, T] with the NaN sample of snapshot NAN_ITEM"""
    q = inputs[f"x{N}"].astype(np.float32)
    x = np.ascontiguousarray((q[..., 0] + 1j * q[..., 1]) * np.float32(2.0 ** -10)).astype(np.complex64)
    x[N // 2, NAN_ITEM * K_SNAP + 5] = complex(np.nan, 1.0)
    return x


def counts_for(M):
    """0..M in turn, and one value out of range"""
    c = (np.arange(N_ITEMS) % (M + 1)).astype(np.int32)
    c[5] = M + 1
    return c


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1).copy()


def _text(rc, text):
    return np.frombuffer(f"{rc}|{text}".encode(), np.uint8).copy()


def run_bits(inputs, N, M, smoothing=None):
    """Every form at one shape -> {name: uint32 words, or uint8 text "rc|error text" for the host entries}.  The pipeline's
    angles are also checked against the chained blocks' here (block entries: `chain.*`, never stored)."""
    import torch

    import doa

    n, d, K = N_ITEMS, SPACING, K_SNAP
    st = torch.cuda.current_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    new = lambda shape, dt: torch.full(shape, -7, dtype=dt, device="cuda")
    host = lambda t: t.cpu().numpy()
    f32, i32 = torch.float32, torch.int32
    out = {}
    x = streams(inputs, N)
    slab = doa.sim.stream_slab_torch([dev(a) for a in x])
    ptrs = [t.data_ptr() for t in slab]
    ptrs1 = [p + K * 8 for p in ptrs]                         # the second batch: one snapshot further on
    Ne = smoothing[0] if smoothing else N                     # the elements the estimator sees

    def host_call(fn):
        try:
            return _text(fn(), "")
        except doa.DoaError as e:
            return _text(e.status, _lib.last_error())

    if not smoothing:
        R = inputs[f"R{N}"]
        dR = dev(R)
        cnt = counts_for(M)
        dcnt = dev(cnt)
        for bits in (64, 32):
            root = doa.rootMUSIC_linear_array(d, M, N)
            root.set_internal_precision(bits)
            ang = new((n, M), f32)
            assert root.work_dev(n, dR.data_ptr(), ang.data_ptr(), st) == n
            out[f"root.work_dev.{bits}"] = words(host(ang))
        root = doa.rootMUSIC_linear_array(d, M, N)
        esp = doa.esprit_linear_array(d, M, N)
        ang, sta = new((n, M), f32), new((n,), i32)
        assert esp.work_dev(n, dR.data_ptr(), ang.data_ptr(), sta.data_ptr(), st) == n
        out["esprit.work_dev.angles"], out["esprit.work_dev.status"] = words(host(ang)), words(host(sta))
        for name, blk in (("root", root), ("esprit", esp)):
            ang, sta = new((n, M), f32), new((n,), i32)
            assert blk.work_dev_counts(n, dR.data_ptr(), dcnt.data_ptr(), ang.data_ptr(), sta.data_ptr(), st) == n
            out[f"{name}.work_dev_counts.angles"], out[f"{name}.work_dev_counts.status"] = words(host(ang)), words(host(sta))
        ang, roots, sta = root.debug(R)
        out["root.debug.angles"], out["root.debug.roots"], out["root.debug.status"] = words(ang), words(roots), words(sta)
        ang = np.full((n, M), -7, np.float32)
        out["root.work.rc"] = host_call(lambda: root.work(n, [R], [ang]))
        out["root.work.angles"] = words(ang)
        ang = np.full((n, M), -7, np.float32)
        out["root.work_counts.rc"] = host_call(lambda: root.work_counts(n, [R], cnt, [ang]))
        out["root.work_counts.angles"] = words(ang)
        ang, sta = np.full((n, M), -7, np.float32), np.full(n, -7, np.int32)
        out["esprit.work.rc"] = host_call(lambda: esp.work(n, [R], [ang, sta]))
        out["esprit.work.angles"], out["esprit.work.status"] = words(ang), words(sta)

    def pipe(estimator, bits=64, lanes=0):
        p = doa.root_pipeline(N, K, 0, 0, d, M, max_batch=n)
        if smoothing: p.set_spatial_smoothing(smoothing[0], smoothing[1])
        if estimator == "esprit": p.set_estimator("esprit")
        if bits != 64: p.set_internal_precision(bits)
        if lanes: p.set_lanes(lanes)
        return p

    # the blocks chained by hand on the pipeline's streams
    cov = new((n, N * N), torch.complex64)
    assert doa.autocorrelate(N, K, 0, 0).work_dev(n, ptrs, cov.data_ptr(), st) == n
    ecov = cov
    if smoothing:
        ecov = new((n, Ne * Ne), torch.complex64)
        assert doa.spatial_smooth(N, smoothing[0], bool(smoothing[1])).work_dev(n, cov.data_ptr(), ecov.data_ptr(), st) == n
    chain = {}
    ang = new((n, M), f32)
    assert doa.rootMUSIC_linear_array(d, M, Ne).work_dev(n, ecov.data_ptr(), ang.data_ptr(), st) == n
    chain["root_music"] = words(host(ang))
    ang = new((n, M), f32)
    assert doa.esprit_linear_array(d, M, Ne).work_dev(n, ecov.data_ptr(), ang.data_ptr(), None, st) == n
    chain["esprit"] = words(host(ang))

    for est in ("root_music", "esprit"):
        p = pipe(est)
        ang, sta = new((n, M), f32), new((n,), i32)
        assert p.work_dev(n, ptrs, None, ang.data_ptr(), sta.data_ptr(), st) == n
        out[f"pipe.{est}.work_dev.angles"], out[f"pipe.{est}.work_dev.status"] = words(host(ang)), words(host(sta))
        assert np.array_equal(out[f"pipe.{est}.work_dev.angles"], chain[est]), ("pipeline != chained blocks", N, M, est)
        for method in ("mdl", "aic"):
            ang, sta, cnt_o, eig = new((n, M), f32), new((n,), i32), new((n,), i32), new((n, Ne), f32)
            assert p.work_dev_auto(n, ptrs, ang.data_ptr(), cnt_o.data_ptr(), method, None, eig.data_ptr(), sta.data_ptr(), st) == n
            for key, t in (("angles", ang), ("status", sta), ("counts", cnt_o), ("eig", eig)):
                out[f"pipe.{est}.auto_{method}.{key}"] = words(host(t))
        if smoothing: continue
        for lanes in (1, 2):
            pl = pipe(est, lanes=lanes)
            a2, s2 = [new((n, M), f32) for _ in range(2)], [new((n,), i32) for _ in range(2)]
            assert pl.work_dev_batches(n, [ptrs, ptrs1], None, [t.data_ptr() for t in a2], [t.data_ptr() for t in s2], st) == 2 * n
            torch.cuda.synchronize()
            out[f"pipe.{est}.batches_{lanes}.angles"] = np.concatenate([words(host(t)) for t in a2])
            out[f"pipe.{est}.batches_{lanes}.status"] = np.concatenate([words(host(t)) for t in s2])
        ang = np.full((n, M), -7, np.float32)
        out[f"pipe.{est}.work.rc"] = host_call(lambda: p.work(n, list(x), ang))
        out[f"pipe.{est}.work.angles"] = words(ang)
    if not smoothing:
        p = pipe("root_music", bits=32)
        ang, sta = new((n, M), f32), new((n,), i32)
        assert p.work_dev(n, ptrs, None, ang.data_ptr(), sta.data_ptr(), st) == n
        out["pipe.root_music.work_dev_32.angles"], out["pipe.root_music.work_dev_32.status"] = words(host(ang)), words(host(sta))
    torch.cuda.synchronize()
    return out


def shape_key(N, M, smoothing=None):
    return f"n{N}m{M}" + (f"s{smoothing[0]}fb{smoothing[1]}" if smoothing else "")


ALL_SHAPES = [(N, M, None) for N, M in SHAPES] + [(SMOOTHED[0], SMOOTHED[3], (SMOOTHED[1], SMOOTHED[2]))]


def run_all_bits(inputs):
    """{shape key + "/" + name: array} over every shape"""
    out = {}
    for N, M, sm in ALL_SHAPES:
        for name, a in run_bits(inputs, N, M, sm).items():
            out[f"{shape_key(N, M, sm)}/{name}"] = a
    return out
