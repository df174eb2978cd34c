// wave_ops.hpp — the moves and reductions between the 64 lanes of a wave, one copy of each, device side only.  wave_ops_debug.hip
// applies each to a known input and tests/test_gpu_wave_ops.py checks the lane maps and orders of addition stated here, bit for bit.
#pragma once

#include "common.hpp"
#include <climits>

namespace doa {

// ---- DPP controls (gfx9 encodings) ---------------------------------------------------------------------------------------------
// A DPP move lets lane i read a register of another lane of its ROW (16 consecutive lanes) without LDS; the control names the source:
//   quad_perm [s0,s1,s2,s3] = s0 | s1 << 2 | s2 << 4 | s3 << 6   lane 4 q + j reads lane 4 q + s_j
//   row_shl:n = 0x100 + n    lane i reads lane i + n of its row; the last n lanes of the row have no source
//   row_shr:n = 0x110 + n    lane i reads lane i - n of its row; the first n lanes of the row have no source
//   row_ror:n = 0x120 + n    lane i reads lane (i - n) mod 16 of its row
//   row_bcast:15 = 0x142     every lane of rows 1..3 reads lane 15 of the row before its own
//   row_bcast:31 = 0x143     every lane of rows 2 and 3 reads lane 31
// A lane whose shift has no source, a lane whose row (lane >> 4) is not in the row mask and a lane whose bank ((lane >> 2) & 3)
// is not in the bank mask receive `old`.  The two broadcasts are used with row masks 0xA and 0xC only, which keep the rows
// they do not serve on `old`; unmasked, those rows were seen to receive their own v on gfx950, and nothing relies on it.
constexpr int quad_pattern(int s0, int s1, int s2, int s3) { return s0 | (s1 << 2) | (s2 << 4) | (s3 << 6); }
constexpr int kQuadXor1 = quad_pattern(1, 0, 3, 2);     // lane i reads lane i ^ 1
constexpr int kQuadXor2 = quad_pattern(2, 3, 0, 1);     // lane i reads lane i ^ 2
template <int N> constexpr int row_shl = 0x100 + N;
template <int N> constexpr int row_shr = 0x110 + N;
template <int N> constexpr int row_ror = 0x120 + N;
constexpr int kRowBcast15 = 0x142, kRowBcast31 = 0x143;

// The one move.  `old` is an operand of the instruction, not a detail: callers pass 0, v or a named value on purpose.
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF> __device__ __forceinline__ int dpp(int old, int v)
{
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, BANK_MASK, false);
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF> __device__ __forceinline__ float dpp(float old, float v)
{
    return __int_as_float(dpp<CTRL, ROW_MASK, BANK_MASK>(__float_as_int(old), __float_as_int(v)));
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF> __device__ __forceinline__ double dpp(double old, double v)
{
    const long long o = __double_as_longlong(old), x = __double_as_longlong(v);
    const int lo = dpp<CTRL, ROW_MASK, BANK_MASK>((int)(o & 0xFFFFFFFFll), (int)(x & 0xFFFFFFFFll));
    const int hi = dpp<CTRL, ROW_MASK, BANK_MASK>((int)(o >> 32), (int)(x >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The one fetch: v of lane src_lane (any lane of the wave, run-time index; a ds_bpermute round trip).
template <typename T> __device__ __forceinline__ T lane_fetch(T v, int src_lane) { return __shfl(v, src_lane, kWave); }

// The wave's index in the grid, in a scalar register (one-dimensional blocks of a multiple of 64 threads).
__device__ __forceinline__ int wave_index()
{
    return __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave);
}

// ---- reductions over an aligned group of G lanes (G = 4, 8, 16, ...; `lane` = the caller's lane in the wave) ---------------------
// xor butterfly: step m = 1, 2, .., G/2 is v[i] = v[i] op v[i ^ m].  Every lane of the group holds the result; for a sum it is the
// balanced tree ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) ..., the same bits in every lane (a + b == b + a).
template <int G, typename T> __device__ __forceinline__ T group_sum(T v, int lane)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += lane_fetch<T>(v, lane ^ m);
    return v;
}
// fmax over the group (a NaN lane is dropped unless all are NaN), in every lane
template <int G, typename T> __device__ __forceinline__ T group_max(T v, int lane)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v = fmax(v, lane_fetch<T>(v, lane ^ m));
    return v;
}
// bitwise OR over the group, in every lane
template <int G> __device__ __forceinline__ int group_or(int v, int lane)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v |= lane_fetch<int>(v, lane ^ m);
    return v;
}

// ---- reductions over a quad and over a DPP row, on DPP moves (old = v or 0 as written) --------------------------------------------
template <int S> __device__ __forceinline__ double quad_rot(double v)      // lane r takes the value of quad lane (r + S) mod 4
{
    return dpp<quad_pattern(S & 3, (1 + S) & 3, (2 + S) & 3, (3 + S) & 3)>(v, v);
}
// (x[i] + x[i^1]) + (x[i^2] + x[i^3]) in lane i of the quad: the same bits in the four lanes (a + b == b + a)
__device__ __forceinline__ double quad_sum(double v)
{
    v += dpp<kQuadXor1>(v, v);
    v += dpp<kQuadXor2>(v, v);
    return v;
}
// Sum over the 16 lanes of a DPP row, in every lane of the row: q = the quad sums as in quad_sum, then lane i of quad k holds
// (q[k] + q[k-1]) + (q[k-2] + q[k-3]), quad indices mod 4 -- the four lanes of a quad agree, the four quads in general do not.
__device__ __forceinline__ double row_sum16(double v)
{
    v += dpp<kQuadXor1>(0.0, v);
    v += dpp<kQuadXor2>(0.0, v);
    v += dpp<row_ror<4>>(0.0, v);
    v += dpp<row_ror<8>>(0.0, v);
    return v;
}

// ---- reductions over the wave on DPP moves, result wave-uniform ----------------------------------------------------------------
// One schedule of six steps, then lane 63 is read: i ^ 1, i ^ 2 (quads), row_ror:4, row_ror:8 (every lane: its row of 16, ordered
// as in row_sum16), row_bcast:15 into rows 1 and 3 (row mask 0xA: r1 += r0, r3 += r2), row_bcast:31 into rows 2 and 3 (row
// mask 0xC).  Lane 63 ends with (r3 + r2) + (r1 + r0), r_k = row k's result as its lane 15 holds it; the other lanes hold
// partial results.  Step::run<CTRL, ROW_MASK>(v) combines a lane's value with that of its source lane.
__device__ __forceinline__ int lane63(int v) { return __builtin_amdgcn_readlane(v, 63); }
__device__ __forceinline__ float lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
template <class Step, class T> __device__ __forceinline__ T wave_six_steps(T v)
{
    Step::template run<kQuadXor1, 0xF>(v);
    Step::template run<kQuadXor2, 0xF>(v);
    Step::template run<row_ror<4>, 0xF>(v);
    Step::template run<row_ror<8>, 0xF>(v);
    Step::template run<kRowBcast15, 0xA>(v);
    Step::template run<kRowBcast31, 0xC>(v);
    return lane63(v);
}
struct WaveSumStep {        // old = 0: a lane the step does not write adds 0
    template <int CTRL, int ROW_MASK, class T> static __device__ __forceinline__ void run(T &v) { v += dpp<CTRL, ROW_MASK>(T(0), v); }
};
struct WaveMaxStep {        // old = v: a lane the step does not write meets its own value
    template <int CTRL, int ROW_MASK> static __device__ __forceinline__ void run(float &v) { v = fmaxf(v, dpp<CTRL, ROW_MASK>(v, v)); }
};
struct WaveMinIntStep {     // old = v
    template <int CTRL, int ROW_MASK> static __device__ __forceinline__ void run(int &v) { v = min(v, dpp<CTRL, ROW_MASK>(v, v)); }
};
// sum (in the order of the schedule), fmaxf (a NaN lane is dropped) and integer minimum over the 64 lanes
__device__ __forceinline__ float wave_allreduce_sum(float v) { return wave_six_steps<WaveSumStep>(v); }
__device__ __forceinline__ int wave_allreduce_sum(int v) { return wave_six_steps<WaveSumStep>(v); }
__device__ __forceinline__ float wave_allreduce_max(float v) { return wave_six_steps<WaveMaxStep>(v); }
__device__ __forceinline__ int wave_allreduce_min_int(int v) { return wave_six_steps<WaveMinIntStep>(v); }
// The minimum of the 64 lanes, a NaN lane dropped like fminf does.
// (six v_min_f32 with the DPP control on the instruction itself: written with update_dpp + fminf the compiler issues a move,
// a canonicalising max and the min per step.  v_min_f32 returns the other operand for a NaN one, like fminf.  A DPP read of
// a VGPR the previous VALU instruction wrote needs two wait states, which nothing inserts inside inline asm.)
__device__ __forceinline__ float wave_allreduce_min(float v)
{
    asm volatile("s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                 "s_nop 1"
                 : "+v"(v));
    return lane63(v);
}

// (value, index) ordering used for ranking: larger value first, then lower index; idx == INT_MAX marks "no candidate".
__device__ __forceinline__ bool cand_better(float v, int i, float bv, int bi)
{
    if (i == INT_MAX) return false;
    if (bi == INT_MAX) return true;
    return (v > bv) || (v == bv && i < bi);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ void argbest_step(float &v, int &i)
{
    // lanes of rows masked off receive their own (v, i) back, which never beats itself
    const float ov = dpp<CTRL, ROW_MASK>(v, v);
    const int oi = dpp<CTRL, ROW_MASK>(i, i);
    if (cand_better(ov, oi, v, i)) { v = ov; i = oi; }
}
// wave-wide best (value, index) pair by cand_better, returned wave-uniform; DPP only (no LDS traffic).  The schedule of
// wave_six_steps written out: through the template the compiler orders the operands of the pick's scalar ORs differently,
// and this header's condition is that no kernel's instructions change (tools/compare_device_code.py).
__device__ __forceinline__ void wave_argbest(float &v, int &i)
{
    argbest_step<kQuadXor1, 0xF>(v, i);
    argbest_step<kQuadXor2, 0xF>(v, i);
    argbest_step<row_ror<4>, 0xF>(v, i);
    argbest_step<row_ror<8>, 0xF>(v, i);
    argbest_step<kRowBcast15, 0xA>(v, i);
    argbest_step<kRowBcast31, 0xC>(v, i);
    v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    i = __builtin_amdgcn_readlane(i, 63);
}

// ---- reductions over the wave on the xor butterfly: the result in every lane ---------------------------------------------------
// step m = 1, 2, .., 32 is v[i] = v[i] + v[i ^ m]: the balanced tree over lanes 0..63, the same bits in every lane.  Two spellings,
// side by side because a kernel's instructions depend on which it was written with: _fetch reads lane (threadIdx.x & 63) ^ m, _xor is __shfl_xor.
template <typename T> __device__ __forceinline__ T wave_butterfly_sum_fetch(T v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += lane_fetch<T>(v, (int)((threadIdx.x & (kWave - 1)) ^ m));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_butterfly_sum_xor(T v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
// maximum as numpy.amax takes it: a NaN sticks
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float wave_butterfly_nan_max(float v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v = nan_max(v, __shfl_xor(v, m, kWave));
    return v;
}

}  // namespace doa
