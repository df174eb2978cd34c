// item_tile.hpp — a tile of consecutive covariance items on its way from global memory to LDS, shared by the kernels that
// take a 256-thread workgroup over kItemTileBytes of items at a time (spatial_smooth.hip, coarray_covariance.hip).
#pragma once
#include "common.hpp"

namespace doa {

constexpr int kItemTileBytes = 8192;
constexpr int kItemTileThreads = 256;

// The loads of the NEXT tile are issued before the current one is worked on and wait in these registers
// (kItemTileBytes / 256 threads = 32 B per thread), so a workgroup has two tiles in flight with one
// tile of LDS.  (Native vector members: as HIP float4 members the compiler kept the struct in memory and moved it to LDS.)
// V16: 16-byte loads (src and tile 16-byte aligned); otherwise 8-byte ones.  n_in: gr_complex of the tile.
static_assert(kItemTileBytes == 2 * (int)sizeof(float4) * kItemTileThreads, "ItemTileStage holds two 16-byte loads per thread");
template <bool V16> struct ItemTileStage {
    doa_f32x4 v0, v1;
    float tail_re, tail_im;
    __device__ __forceinline__ void load(const float2 *src, int n_in)
    {
        const int q = threadIdx.x;
        if constexpr (V16) {
            const doa_f32x4 *src4 = reinterpret_cast<const doa_f32x4 *>(src);
            if (q < n_in / 2) v0 = src4[q];
            if (q + kItemTileThreads < n_in / 2) v1 = src4[q + kItemTileThreads];
            if ((n_in & 1) && q == 0) { tail_re = src[n_in - 1].x; tail_im = src[n_in - 1].y; }
        } else {
            if (q < n_in) { v0.x = src[q].x; v0.y = src[q].y; }
            if (q + kItemTileThreads < n_in) { v0.z = src[q + kItemTileThreads].x; v0.w = src[q + kItemTileThreads].y; }
            if (q + 2 * kItemTileThreads < n_in) { v1.x = src[q + 2 * kItemTileThreads].x; v1.y = src[q + 2 * kItemTileThreads].y; }
            if (q + 3 * kItemTileThreads < n_in) { v1.z = src[q + 3 * kItemTileThreads].x; v1.w = src[q + 3 * kItemTileThreads].y; }
        }
    }
    __device__ __forceinline__ void put(float2 *tile, int n_in) const
    {
        const int q = threadIdx.x;
        if constexpr (V16) {
            doa_f32x4 *tile4 = reinterpret_cast<doa_f32x4 *>(tile);
            if (q < n_in / 2) tile4[q] = v0;
            if (q + kItemTileThreads < n_in / 2) tile4[q + kItemTileThreads] = v1;
            if ((n_in & 1) && q == 0) tile[n_in - 1] = make_float2(tail_re, tail_im);
        } else {
            if (q < n_in) tile[q] = make_float2(v0.x, v0.y);
            if (q + kItemTileThreads < n_in) tile[q + kItemTileThreads] = make_float2(v0.z, v0.w);
            if (q + 2 * kItemTileThreads < n_in) tile[q + 2 * kItemTileThreads] = make_float2(v1.x, v1.y);
            if (q + 3 * kItemTileThreads < n_in) tile[q + 3 * kItemTileThreads] = make_float2(v1.z, v1.w);
        }
    }
};

// items of one tile: as many as kItemTileBytes hold, an even number so that every tile starts on a 16-byte boundary
inline int item_tile_items(int item_complex) { return (kItemTileBytes / (int)sizeof(float2) / item_complex) & ~1; }

}  // namespace doa
