// spatial_smooth.hip — spatial smoothing of covariance items (Shan-Wax-Kailath; forward-backward: Pillai-Kwon): kernel + C ABI.
//
// Not a block of the reference.  For coherent sources (a source and its multipath echo, emitters on one oscillator) the
// signal part of the covariance has rank one and MUSIC, Root-MUSIC and the source count all fail; for a uniform linear array
// the N x N covariance is replaced by the average of its L = N - S + 1 overlapping S x S diagonal blocks (and, forward-backward,
// of their persymmetric images), which restores the rank.  The definition -- one for every entry -- is in include/doa_hip.h;
// the kernel does its operations in its order, so its outputs are bit-identical to the numpy statement of the tests.
//
// Shape: items are 32 B (N = 2) to 2 KiB (N = 16), and an output element needs L (2 L forward-backward) upper-triangle
// elements of its item along one diagonal -- about one double addition per byte moved, so the kernel is traffic-bound.  A
// 256-thread workgroup takes a TILE of consecutive items (at most kTileBytes of input, an even number of items so that every
// tile starts on a 16-byte boundary), stages it in LDS with coalesced 16-byte loads (the next tile's loads are already in
// flight: ItemTileStage, item_tile.hpp), and each thread then produces PAIRS of consecutive elements of the tile's contiguous output range
// (items * S^2 gr_complex): one 16-byte store per pair.  A lower-triangle element is computed as its mirror and conjugated, so
// nothing is exchanged between threads after the staging.
// Grid-stride over tiles.  The 8-byte form (either base pointer not 16-byte aligned) differs in the width of the global
// loads and stores only.
#include "kernels.hpp"
#include "item_tile.hpp"

namespace doa {

constexpr int kSmoothTileBytes = kItemTileBytes;
constexpr int kSmoothThreads = kItemTileThreads;

struct SmoothArgs {
    const float2 *in;
    float2 *out;
    int N, S, L, fb, n_items, tile_items;
    GroupSplit by_ss, by_s;     // element of the tile's output range -> (item, rest), rest -> (column, row)
    double inv_l;               // 1.0 / L
};

// f[i,j] = sum_l H[i+l, j+l] (i <= j: upper triangle only), l ascending, re and im separately; diagonal: real parts only
__device__ __forceinline__ void smooth_diag_sum(const float2 *H, int N, int L, int i, int j, double &re, double &im)
{
    const float2 *p = H + i + j * N;
    double sr = 0.0, si = 0.0;
    if (i == j) {
        for (int l = 0; l < L; l++, p += N + 1) sr += (double)p->x;
    } else {
        for (int l = 0; l < L; l++, p += N + 1) {
            const float2 v = *p;
            sr += (double)v.x;
            si += (double)v.y;
        }
    }
    re = sr; im = si;
}

__device__ __forceinline__ float2 smooth_element(const float2 *tile, const SmoothArgs &a, unsigned e)
{
    unsigned item, rest, col, row;
    a.by_ss(e, item, rest);
    a.by_s(rest, col, row);
    const int i = (int)(row < col ? row : col), j = (int)(row < col ? col : row);
    const float2 *H = tile + item * (unsigned)(a.N * a.N);
    double sr, si;
    smooth_diag_sum(H, a.N, a.L, i, j, sr, si);
    if (a.fb) {
        double br, bi;
        smooth_diag_sum(H, a.N, a.L, a.S - 1 - j, a.S - 1 - i, br, bi);
        sr = 0.5 * (sr + br);
        si = 0.5 * (si + bi);
    }
    const float re = (float)(sr * a.inv_l), im = (float)(si * a.inv_l);
    return make_float2(re, row > col ? -im : im);
}

template <bool V16>
__global__ __launch_bounds__(kSmoothThreads) void spatial_smooth_kernel(SmoothArgs a)
{
    __shared__ float4 tile4[kSmoothTileBytes / sizeof(float4)];
    float2 *tile = reinterpret_cast<float2 *>(tile4);
    const int nn = a.N * a.N, ss = a.S * a.S;
    const int n_tiles = (a.n_items + a.tile_items - 1) / a.tile_items;
    auto items_of = [&](int tb) { const int left = a.n_items - tb * a.tile_items; return left < a.tile_items ? left : a.tile_items; };
    // (tile tb starts at item tb * tile_items, an even number: 16-byte aligned in both arrays when their bases are)
    ItemTileStage<V16> stage;
    int tb = blockIdx.x;
    if (tb < n_tiles) stage.load(a.in + (size_t)tb * a.tile_items * nn, items_of(tb) * nn);
    for (; tb < n_tiles; tb += gridDim.x) {
        const int items = items_of(tb);
        const int n_out = items * ss;                            // gr_complex of the tile: <= kSmoothTileBytes / 8
        stage.put(tile, items * nn);
        __syncthreads();
        if (const int nx = tb + gridDim.x; nx < n_tiles) stage.load(a.in + (size_t)nx * a.tile_items * nn, items_of(nx) * nn);
        float2 *dst = a.out + (size_t)tb * a.tile_items * ss;
        for (int q = threadIdx.x; 2 * q < n_out; q += kSmoothThreads) {
            const float2 v0 = smooth_element(tile, a, 2u * q);
            if (2 * q + 1 < n_out) {
                const float2 v1 = smooth_element(tile, a, 2u * q + 1);
                if constexpr (V16) {
                    reinterpret_cast<float4 *>(dst)[q] = make_float4(v0.x, v0.y, v1.x, v1.y);
                } else {
                    dst[2 * q] = v0;
                    dst[2 * q + 1] = v1;
                }
            } else {
                dst[2 * q] = v0;
            }
        }
        __syncthreads();                                         // the tile is overwritten by the next round's stage.put
    }
}

// d_Rs must not overlap d_R (not checked): a workgroup reads its tile after other workgroups have stored theirs
int launch_spatial_smooth(int N, int S, int fb, int n_items, const void *d_R, void *d_Rs, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    if (S < 2 || S > N || N > DOA_MAX_ANT_ELE || (fb != 0 && fb != 1)) {
        set_error("spatial_smooth: need 2 <= subarray_size <= num_ant_ele <= %d, forward_backward 0 or 1 (got %d, %d, %d)",
                  DOA_MAX_ANT_ELE, S, N, fb);
        return DOA_ERR_INVALID_ARG;
    }
    SmoothArgs a;
    a.in = static_cast<const float2 *>(d_R); a.out = static_cast<float2 *>(d_Rs);
    a.N = N; a.S = S; a.L = N - S + 1; a.fb = fb; a.n_items = n_items;
    a.tile_items = item_tile_items(N * N);                       // 4 (N = 16) .. 256 (N = 2), even
    a.by_ss = GroupSplit::make(S * S); a.by_s = GroupSplit::make(S);
    a.inv_l = 1.0 / a.L;
    int blocks = (n_items + a.tile_items - 1) / a.tile_items;
    if (blocks > cu_count() * 4) blocks = cu_count() * 4;        // four 8 KiB tiles per CU, grid-stride beyond
    const bool v16 = ((reinterpret_cast<uintptr_t>(d_R) | reinterpret_cast<uintptr_t>(d_Rs)) & 15) == 0;
    if (v16) hipLaunchKernelGGL(spatial_smooth_kernel<true>, dim3(blocks), dim3(kSmoothThreads), 0, st, a);
    else     hipLaunchKernelGGL(spatial_smooth_kernel<false>, dim3(blocks), dim3(kSmoothThreads), 0, st, a);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

#include "block_host.hpp"

struct doa_spatial_smooth : doa::BlockBase {
    int N = 0, S = 0, fb = 0;
    doa::DevBuf d_in, d_out;
};

extern "C" {

doa_spatial_smooth_t *doa_spatial_smooth_create(int num_ant_ele, int subarray_size, int forward_backward)
{
    doa::clear_error();
    if (subarray_size < 2 || subarray_size > num_ant_ele || (forward_backward != 0 && forward_backward != 1)) {
        doa::set_error("spatial_smooth: need 2 <= subarray_size <= num_ant_ele, forward_backward 0 or 1 (got %d, %d, %d)",
                       subarray_size, num_ant_ele, forward_backward);
        return nullptr;
    }
    if (num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("spatial_smooth: num_ant_ele=%d exceeds DOA_MAX_ANT_ELE=%d", num_ant_ele, DOA_MAX_ANT_ELE);
        return nullptr;
    }
    return doa::create_block<doa_spatial_smooth>("spatial_smooth", [&](doa_spatial_smooth &h) {
        h.N = num_ant_ele; h.S = subarray_size; h.fb = forward_backward;
        return DOA_OK;
    });
}

void doa_spatial_smooth_destroy(doa_spatial_smooth_t *h) { doa::destroy_block(h); }

int doa_spatial_smooth_work_dev(doa_spatial_smooth_t *h, int noutput_items, const void *d_cov_items, void *d_smoothed_items,
                                void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("spatial_smooth_work_dev", h, noutput_items, {d_cov_items, d_smoothed_items}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int rc = doa::launch_spatial_smooth(h->N, h->S, h->fb, noutput_items, d_cov_items, d_smoothed_items,
                                              static_cast<hipStream_t>(hip_stream));
    return rc == DOA_OK ? noutput_items : rc;
}

int doa_spatial_smooth_work(doa_spatial_smooth_t *h, int noutput_items, const void *cov_items, void *smoothed_items)
{
    doa::clear_error();
    if (int rc = doa::work_args("spatial_smooth_work", h, noutput_items, {cov_items, smoothed_items}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, (size_t)noutput_items * h->N * h->N * sizeof(float2));
    io.out(h->d_out, smoothed_items, (size_t)noutput_items * h->S * h->S * sizeof(float2));
    int rc = io.status();
    if (rc == DOA_OK) rc = doa_spatial_smooth_work_dev(h, noutput_items, h->d_in.p, h->d_out.p, h->stream);
    return io.finish(rc);
}

}  // extern "C"
