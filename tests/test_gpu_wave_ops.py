"""GPU tests of gr-doa_amd/csrc/wave_ops.hpp, the moves and reductions between the lanes of a wave, through
doa_hip_wave_ops_debug (include/doa_hip_test.h): one workgroup of 256 threads applies one primitive to in[t] and every thread stores
what it holds afterwards.

The expectation is computed here in numpy from the lane maps and the orders of addition that the header states, step by step in
the arithmetic of the element type, and compared bit for bit: there is no tolerance.  Small integers held as float or double
give the same bits in every order of addition; the values of mixed magnitude do not, and pin the order."""
import ctypes as C

import numpy as np
import pytest

from doa import _lib

pytestmark = pytest.mark.gpu

T, WAVE = 256, 64
LANE = np.arange(T) % WAVE
BASE = np.arange(T) - LANE                       # first thread of the thread's wave
INT_MAX = np.int32(2**31 - 1)
PAIR = np.dtype([("v", np.float32), ("i", np.int32)])


def run(op, arr):
    arr = np.ascontiguousarray(arr)
    out = np.zeros(T, arr.dtype)
    rc = _lib.lib.doa_hip_wave_ops_debug(op, arr.size, arr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == T, _lib.last_error()
    return out


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    bad = np.flatnonzero(got.view(np.uint8).reshape(T, -1) != want.view(np.uint8).reshape(T, -1)).size
    assert bad == 0, f"{what}: got {got}, want {want}"


def small(dtype, seed):
    """small integers in the element type: every order of addition is exact"""
    return np.random.default_rng(seed).integers(-8, 9, T).astype(dtype)


def mixed(dtype, seed):
    """values of mixed magnitude and sign: the sum depends on the order of the additions"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 6, T)).astype(dtype)


# ---- the lane maps of the header's comment block: source thread of every thread, -1 where a lane has no source ----------------
def src_xor(m):
    return BASE + (LANE ^ m)


def src_row(kind, n):
    r = LANE % 16
    if kind == "shl":
        return np.where(r + n < 16, np.arange(T) + n, -1)
    if kind == "shr":
        return np.where(r >= n, np.arange(T) - n, -1)
    if kind == "ror":
        return np.arange(T) - r + (r - n) % 16
    if kind == "bcast15":
        return np.where(LANE >= 16, BASE + 16 * (LANE // 16) - 1, -1)
    if kind == "bcast31":
        return np.where(LANE >= 32, BASE + 31, -1)
    raise ValueError(kind)


def moved(v, old, src, row_mask=0xF, bank_mask=0xF):
    """dpp<control, row_mask, bank_mask>(old, v): a lane without a source or outside either mask receives old"""
    written = (src >= 0) & (((row_mask >> (LANE // 16)) & 1) == 1) & (((bank_mask >> ((LANE // 4) % 4)) & 1) == 1)
    return np.where(written, v[np.maximum(src, 0)], old)


# c of op 1000 + 100 t + c -> (source map, row mask, bank mask)
# (the two broadcasts with the row masks they are used with: the header promises nothing for an unmasked row without a source)
CONTROLS = {0: (src_xor(1), 0xF, 0xF), 1: (src_xor(2), 0xF, 0xF), 2: (src_row("shl", 2), 0xF, 0xF), 3: (src_row("shr", 2), 0xF, 0xF),
            4: (src_row("shr", 2), 0xF, 0x1), 5: (src_row("bcast15", 0), 0xA, 0xF), 6: (src_row("bcast31", 0), 0xC, 0xF),
            7: (src_xor(1), 0x5, 0x6)}
CONTROLS.update({10 + k: (src_row("ror", k), 0xF, 0xF) for k in range(1, 16)})


@pytest.mark.parametrize("t,dtype", [(0, np.int32), (1, np.float32), (2, np.float64)])
def test_dpp_move(t, dtype):
    """every named control the kernels use, on the three element types; v and old are all different, so a lane that took the
    wrong source, or the wrong half of a double, shows"""
    rng = np.random.default_rng(10 + t)
    if dtype is np.int32:
        both = rng.permutation(2 * T).astype(np.int32) * 65537 - 2**24
    else:
        both = (rng.permutation(2 * T) + rng.uniform(0.1, 0.9, 2 * T)).astype(dtype) * dtype(1.0 / 3.0)
    v, old = both[:T], both[T:]
    for c, (src, rm, bm) in sorted(CONTROLS.items()):
        want = moved(v, old, src, rm, bm)
        if (rm, bm) != (0xF, 0xF) or (src < 0).any():
            assert (want == old).any() and (want != old).any()          # some lanes stay on old, some move
        same_bits(run(1000 + 100 * t + c, both), want, f"control {c}")


def test_wave_index():
    same_bits(run(0, np.zeros(T, np.int32)), (np.arange(T) // WAVE).astype(np.int32))


def butterfly(v, width, op):
    for m in [1 << k for k in range(width.bit_length() - 1)]:
        v = op(v, v[src_xor(m)])
    return v


@pytest.mark.parametrize("g,G", [(0, 4), (1, 8), (2, 16)])
def test_group_reductions(g, G):
    add = lambda a, b: a + b
    for inp in (small, mixed):
        for op, dtype in ((10 + g, np.float64), (20 + g, np.float32)):
            x = inp(dtype, 100 + op)
            want = butterfly(x, G, add)
            assert want.dtype == dtype
            same_bits(run(op, x), want, f"group_sum<{G}> {dtype.__name__} {inp.__name__}")
            if inp is small:                                             # and it is the sum of the group, in every lane
                same_bits(want, x.reshape(-1, G).sum(axis=1).repeat(G))
    x = mixed(np.float64, 30 + g)
    x[[3, 77, 78, 200]] = np.nan                                         # fmax drops a NaN lane
    x[128:128 + G] = np.nan                                              # ... unless the whole group is NaN
    want = butterfly(x, G, np.fmax)
    same_bits(run(30 + g, x), want, f"group_max<{G}>")
    same_bits(want, np.fmax.reduce(x.reshape(-1, G), axis=1).repeat(G))
    b = np.zeros(T, np.int32)
    b[[5, 64 + 15, 64 + 16, 255]] = [1, 4, 2, 8]                         # most groups hold no flag at all
    same_bits(run(40 + g, b), np.bitwise_or.reduce(b.reshape(-1, G), axis=1).repeat(G).astype(np.int32), f"group_or<{G}>")


def test_quad_and_row():
    for inp in (small, mixed):
        x = inp(np.float64, 50)
        for s in (1, 2, 3):
            same_bits(run(50 + s, x), x[np.arange(T) - LANE % 4 + (LANE % 4 + s) % 4], f"quad_rot<{s}>")
        q = butterfly(x, 4, lambda a, b: a + b)
        same_bits(run(54, x), q, "quad_sum")
        # row_sum16: the quad sums, then + row_ror:4, then + row_ror:8 (old = 0 is never taken: every lane has a source)
        r = q + q[src_row("ror", 4)]
        r = r + r[src_row("ror", 8)]
        same_bits(run(55, x), r, "row_sum16")
        if inp is small:
            same_bits(r, x.reshape(-1, 16).sum(axis=1).repeat(16))


def six_steps(v, step):
    """the schedule of the DPP all-reduces; step(v, src, row_mask) is one combine.  Lane 63 of each wave holds the result."""
    for src, rm in ((src_xor(1), 0xF), (src_xor(2), 0xF), (src_row("ror", 4), 0xF), (src_row("ror", 8), 0xF),
                    (src_row("bcast15", 0), 0xA), (src_row("bcast31", 0), 0xC)):
        v = step(v, src, rm)
    return v[BASE + 63]


def test_wave_allreduce_sum_max_min():
    sum_step = lambda v, src, rm: v + moved(v, np.zeros_like(v), src, rm)            # old = 0
    for inp in (small, mixed):
        x = inp(np.float32, 60)
        want = six_steps(x, sum_step)
        assert want.dtype == np.float32
        same_bits(run(60, x), want, f"wave_allreduce_sum float {inp.__name__}")
    same_bits(six_steps(small(np.float32, 60), sum_step), small(np.float32, 60).reshape(4, WAVE).sum(axis=1).repeat(WAVE))
    n = np.random.default_rng(61).integers(-2**20, 2**20, T).astype(np.int32)
    same_bits(run(61, n), n.reshape(4, WAVE).sum(axis=1).repeat(WAVE).astype(np.int32), "wave_allreduce_sum int")
    same_bits(six_steps(n, sum_step), n.reshape(4, WAVE).sum(axis=1).repeat(WAVE).astype(np.int32))

    x = mixed(np.float32, 62)
    x[[9, 64 + 63, 128]] = np.nan                                        # fmaxf and v_min_f32 drop a NaN lane
    same_bits(run(62, x), six_steps(x, lambda v, src, rm: np.fmax(v, moved(v, v, src, rm))), "wave_allreduce_max")
    same_bits(run(62, x), np.fmax.reduce(x.reshape(4, WAVE), axis=1).repeat(WAVE))
    same_bits(run(63, x), np.fmin.reduce(x.reshape(4, WAVE), axis=1).repeat(WAVE), "wave_allreduce_min with a NaN lane")
    m = np.random.default_rng(64).integers(-2**30, 2**30, T).astype(np.int32)
    m[64:128] = INT_MAX                                                   # "no position" in every lane of a wave
    same_bits(run(64, m), m.reshape(4, WAVE).min(axis=1).repeat(WAVE), "wave_allreduce_min_int")


def cand_better(v, i, bv, bi):
    return (i != INT_MAX) & ((bi == INT_MAX) | (v > bv) | ((v == bv) & (i < bi)))


def argbest(x):
    def step(p, src, rm):
        ov, oi = moved(p["v"], p["v"], src, rm), moved(p["i"], p["i"], src, rm)
        take = cand_better(ov, oi, p["v"], p["i"])
        out = p.copy()
        out["v"], out["i"] = np.where(take, ov, p["v"]), np.where(take, oi, p["i"])
        return out
    return six_steps(x, step)


def test_wave_argbest():
    rng = np.random.default_rng(65)
    x = np.zeros(T, PAIR)
    x["v"] = rng.integers(0, 4, T).astype(np.float32)
    # wave 0: the maximum 9 in several rows, indices not in lane order: the lowest index wins
    x["i"][:64] = rng.permutation(64) + 1000
    x["v"][[2, 17, 18, 40, 63]] = 9.0
    # wave 1: every index INT_MAX: no candidate, whatever the values
    x["i"][64:128] = INT_MAX
    # wave 2: a single candidate in lane 63; wave 3: a single candidate in lane 0 (with the smallest value of its wave)
    x["i"][128:256] = INT_MAX
    x["i"][128 + 63], x["v"][128 + 63] = 7, -3.0
    x["i"][192], x["v"][192] = 5, -1.0
    got, want = run(65, x), argbest(x)
    same_bits(got, want, "wave_argbest")
    assert (got["i"][:64] == x["i"][[2, 17, 18, 40, 63]].min()).all() and (got["v"][:64] == 9.0).all()
    assert (got["i"][64:128] == INT_MAX).all()
    assert (got["i"][128:192] == 7).all() and (got["v"][128:192] == -3.0).all()
    assert (got["i"][192:] == 5).all() and (got["v"][192:] == -1.0).all()
    # and a wave of distinct random candidates against the definition
    y = np.zeros(T, PAIR)
    y["v"], y["i"] = mixed(np.float32, 66), rng.permutation(T).astype(np.int32)
    got = run(65, y)
    same_bits(got, argbest(y), "wave_argbest, random")
    for w in range(4):
        k = 64 * w + int(np.argmax(y["v"][64 * w:64 * w + 64]))
        assert (got["v"][64 * w:64 * w + 64] == y["v"][k]).all() and (got["i"][64 * w:64 * w + 64] == y["i"][k]).all()


def test_wave_butterflies():
    add = lambda a, b: a + b
    for inp in (small, mixed):
        for op, dtype in ((70, np.float32), (71, np.float64), (72, np.float64)):
            x = inp(dtype, op)
            want = butterfly(x, WAVE, add)
            assert want.dtype == dtype
            same_bits(run(op, x), want, f"op {op} {inp.__name__}")
            if inp is small:
                same_bits(want, x.reshape(4, WAVE).sum(axis=1).repeat(WAVE))
    x = mixed(np.float32, 73)
    x[[31, 128 + 63]] = np.nan                                           # nan_max: a NaN sticks (waves 0 and 2), else the maximum
    nan_max = lambda a, b: np.where((b > a) | (b != b), b, a)
    got = run(73, x)
    same_bits(got, butterfly(x, WAVE, nan_max), "wave_butterfly_nan_max")
    assert np.isnan(got[:64]).all() and np.isnan(got[128:192]).all()
    assert (got[64:128] == x[64:128].max()).all() and (got[192:] == x[192:].max()).all()


def test_bad_arguments():
    x = np.zeros(2 * T, np.float32)
    out = np.zeros(T, np.float32)
    f = _lib.lib.doa_hip_wave_ops_debug
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert f(60, 2 * T, p(x), p(out)) < 0 and f(1100, T, p(x), p(out)) < 0      # n is 256, and 512 for the move
    assert f(99, T, p(x), p(out)) < 0 and f(1126, 2 * T, p(x), p(out)) < 0 and "no op" in _lib.last_error()
    assert f(60, T, None, p(out)) < 0 and f(60, T, p(x), None) < 0
