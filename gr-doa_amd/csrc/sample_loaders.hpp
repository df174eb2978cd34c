// sample_loaders.hpp — how the streaming kernels (K1 in autocorrelate.hip, the phase-offset estimator in
// phase_offset_est.hip) read one stream in either input sample format.
#pragma once
#include "common.hpp"

namespace doa {

// Sample loaders.  A kernel asks for sample i of a stream (one) or for samples i and i+1 as (re_i, im_i, re_i+1, im_i+1)
// (pair, one load); which samples a lane takes, which accumulator they meet and in what order is the kernel's business and
// the same for every loader, so the sc16 and fc32 instantiations sum the same floats in the same order.
//   fc32: gr_complex, 8 B per sample, pair = one 16-byte load.
//   sc16: complex int16 (real first, 4 B per sample; one `int` here), pair = one 8-byte load, widened in registers as
//         __fmul_rn((float)q, scale) per component -- one rounding, no contraction into the accumulating FMAs, so the
//         kernel sees exactly the floats np.float32(q) * np.float32(scale) of an fc32 caller.
// Both loaders run at the same unroll depth UN (as many load instructions in flight, half the bytes for sc16).  Twice the
// sc16 depth, to keep as many BYTES in flight as fc32, measured worse on MI355X: the widened pairs raise the wave kernel
// at N = 4 from 116 to 180 VGPRs, which halves its occupancy (K1 at the benchmark shape 16.0 against 12.6 us, at K = 2048 /
// overlap 512 38.4 against 24.6 us, N = 8 37.5 against 34.9, N = 16 on the matrix cores unchanged; profiles/sc16_k1.txt).
struct Fc32Samples {
    typedef float2 sample_t;
    template <bool NT> __device__ static __forceinline__ float4 pair(const sample_t *p, float)
    {
        return load_f4<NT>(reinterpret_cast<const float4 *>(p));
    }
    __device__ static __forceinline__ float2 one(const sample_t *p, float) { return *p; }
};
struct Sc16Samples {
    typedef int sample_t;                  // low half = re, high half = im (little-endian int16 pair)
    __device__ static __forceinline__ float2 widen(int w, float s)
    {
        return make_float2(__fmul_rn((float)(short)(w & 0xffff), s), __fmul_rn((float)(w >> 16), s));
    }
    template <bool NT> __device__ static __forceinline__ float4 pair(const sample_t *p, float s)
    {
        typedef int i32x2 __attribute__((ext_vector_type(2)));
        i32x2 v;
        if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const i32x2 *>(p));
        else v = *reinterpret_cast<const i32x2 *>(p);
        const float2 a = widen(v.x, s), b = widen(v.y, s);
        return make_float4(a.x, a.y, b.x, b.y);
    }
    __device__ static __forceinline__ float2 one(const sample_t *p, float s) { return widen(*p, s); }
};

}  // namespace doa
