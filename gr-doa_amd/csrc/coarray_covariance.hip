// coarray_covariance.hip — the difference co-array of a sparse linear array (Pal-Vaidyanathan; T^2 / Lv: Liu-Vaidyanathan):
// kernel + C ABI.
//
// Not a block of the reference.  The N x N covariance of N elements at integer positions holds every lag 0 .. Lv-1 of a
// virtual Lv-element uniform array (Lv up to N (N - 1) / 2 + 1, capped at 16); the entries of equal lag are averaged into
// r[0 .. Lv-1], and the output item is the Hermitian Toeplitz matrix T of r (TOEPLITZ) or T T^H / Lv (SMOOTHED), which
// MUSIC_lin_array, rootMUSIC_linear_array and esprit_linear_array created for Lv elements read as a covariance item: more
// sources than antennas.  The definition -- one for every entry -- is in include/doa_hip.h; in TOEPLITZ mode the kernel does
// its operations in its order, so its outputs are bit-identical to the numpy statement of the tests.
//
// Shape: per item up to 2 KiB in and 2 KiB out, at most 136 additions for r and at Lv = 16 4096 complex multiply-adds for T^2
// -- less time in the fp64 pipe than the traffic takes, so the kernel is traffic- and latency-bound, and spatial_smooth.hip
// is its template: a 256-thread workgroup takes a TILE of consecutive items (item_tile.hpp: at most 8 KiB of input, an even
// number of items so that every tile starts on a 16-byte boundary in both arrays; fewer where full tiles would leave compute
// units idle: coarray_tile_items), stages it in LDS with coalesced 16-byte loads while the next tile's loads are already in
// flight, and then
//   1. one thread per (item, lag) sums the lag's entries from the tile in the order of the host-built pair list (in LDS)
//      and leaves r[lag] and its conjugate in LDS as the item's t(-(Lv-1)) .. t(Lv-1), t(m) = T[i,i-m], 16 bytes each;
//   2. each thread produces PAIRS of consecutive elements of the tile's contiguous output range (items * Lv^2 gr_complex)
//      from t alone, one 16-byte store per pair.  A lower-triangle element is computed as its mirror and conjugated, so
//      nothing else is exchanged between threads.
// t is read as 16-byte words, a row of T backwards through it: neighbouring lanes are neighbouring rows of one column, so
// T[i,k] comes from neighbouring 16-byte slots and conj(T[j,k]) is one address for the lanes of a column.  Grid-stride over
// tiles.  The 8-byte form (either base pointer not 16-byte aligned) differs in the width of the global loads and stores
// only.  No atomics, no scratch, no cross-lane sums.
#include <algorithm>

#include "kernels.hpp"
#include "item_tile.hpp"

namespace doa {

// t entries of one tile: tile items * (2 Lv - 1).  A full tile never needs more: 1024 / N^2 items, and 2 Lv - 1 <= N^2 - N + 1
constexpr int kCoarrayLagSlots = 1024;

// What CoarrayTables::build uploads and every workgroup copies to LDS once.
struct CoarrayList {
    double inv_c[DOA_MAX_ANT_ELE];                 // 1.0 / c_l
    unsigned short start[DOA_MAX_ANT_ELE + 2];     // (+ 1 pad: the struct is a whole number of 8-byte words)
    unsigned short pair[kCoarrayMaxPairs];
};
static_assert(sizeof(CoarrayList) % sizeof(double) == 0 && sizeof(CoarrayList) / sizeof(double) <= kItemTileThreads,
              "one 8-byte word per thread copies the list");

struct CoarrayArgs {
    const float2 *in;
    float2 *out;
    const CoarrayList *list;
    int N, Lv, n_items, tile_items;
    GroupSplit by_ll, by_l;     // element of the tile's output range -> (item, rest), rest -> (column, row); by_l also task -> (item, lag)
    double inv_lv;              // 1.0 / Lv
};

// r[l] of one item: the sum over the lag's pairs in list order, re and im separately, times 1.0 / c_l; l = 0: real parts only
__device__ __forceinline__ double2 coarray_lag_mean(const float2 *H, const CoarrayList &list, int l)
{
    double sr = 0.0, si = 0.0;
    const int k1 = list.start[l + 1];
    if (l == 0) {
        for (int k = list.start[0]; k < k1; k++) sr += (double)H[list.pair[k]].x;
    } else {
        for (int k = list.start[l]; k < k1; k++) {
            const unsigned e = list.pair[k];
            const float2 v = H[e & (kCoarrayConj - 1u)];
            sr += (double)v.x;
            si += (e & kCoarrayConj) ? -(double)v.y : (double)v.y;
        }
    }
    const double inv = list.inv_c[l];
    return make_double2(sr * inv, si * inv);
}

// element e of the tile's output range from the tile's t: per item the 2 Lv - 1 values t(m) = r[m] (m >= 0), conj(r[-m]) (m < 0),
// m ascending, so that T[i,k] = t(i-k) is read without a branch on the sign
template <int MODE>
__device__ __forceinline__ float2 coarray_element(const double2 *t, const CoarrayArgs &a, unsigned e)
{
    unsigned item, rest, col, row;
    a.by_ll(e, item, rest);
    a.by_l(rest, col, row);
    const int i = (int)(row < col ? row : col), j = (int)(row < col ? col : row);      // the element computed: (row i, column j), i <= j
    const double2 *t0 = t + item * (unsigned)(2 * a.Lv - 1) + (a.Lv - 1);               // the item's t(0)
    float re, im;
    if constexpr (MODE == DOA_COARRAY_TOEPLITZ) {
        const double2 v = t0[i - j];                              // T[i,j] = t(i-j) = conj(r[j-i])
        re = (float)v.x;
        im = i == j ? 0.f : (float)v.y;
    } else {
        // sum_k T[i,k] conj(T[j,k]) = sum_k t(i-k) conj(t(j-k)):  (x + iy)(u - iv) = xu + yv + i (yu - xv); two rows of T walked
        // backwards through t, 16 bytes a step
        const double2 *p = t0 + i, *q = t0 + j;
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < a.Lv; k++, p--, q--) {
            const double2 u = *p, v = *q;
            sr += u.x * v.x + u.y * v.y;
            si += u.y * v.x - u.x * v.y;
        }
        re = (float)(sr * a.inv_lv);
        im = i == j ? 0.f : (float)(si * a.inv_lv);
    }
    return make_float2(re, row > col ? -im : im);
}

template <bool V16, int MODE>
__global__ __launch_bounds__(kItemTileThreads) void coarray_covariance_kernel(CoarrayArgs a)
{
    __shared__ float4 tile4[kItemTileBytes / sizeof(float4)];
    __shared__ double2 t[kCoarrayLagSlots];
    __shared__ CoarrayList list;
    float2 *tile = reinterpret_cast<float2 *>(tile4);
    const int nn = a.N * a.N, ll = a.Lv * a.Lv;
    const int n_tiles = (a.n_items + a.tile_items - 1) / a.tile_items;
    auto items_of = [&](int tb) { const int left = a.n_items - tb * a.tile_items; return left < a.tile_items ? left : a.tile_items; };
    // (tile tb starts at item tb * tile_items, an even number: 16-byte aligned in both arrays when their bases are)
    ItemTileStage<V16> stage;
    int tb = blockIdx.x;
    if (tb < n_tiles) stage.load(a.in + (size_t)tb * a.tile_items * nn, items_of(tb) * nn);
    if (threadIdx.x < sizeof(CoarrayList) / sizeof(double))
        reinterpret_cast<double *>(&list)[threadIdx.x] = reinterpret_cast<const double *>(a.list)[threadIdx.x];
    for (; tb < n_tiles; tb += gridDim.x) {
        const int items = items_of(tb);
        stage.put(tile, items * nn);
        __syncthreads();                                         // the tile (and, the first time, the list) is in LDS
        if (const int nx = tb + gridDim.x; nx < n_tiles) stage.load(a.in + (size_t)nx * a.tile_items * nn, items_of(nx) * nn);
        for (unsigned task = threadIdx.x; task < (unsigned)(items * a.Lv); task += kItemTileThreads) {
            unsigned item, l;
            a.by_l(task, item, l);
            const double2 m = coarray_lag_mean(tile + item * (unsigned)nn, list, (int)l);
            double2 *t0 = t + item * (unsigned)(2 * a.Lv - 1) + (a.Lv - 1);             // < items (2 Lv - 1) <= kCoarrayLagSlots
            t0[l] = m;
            if (l) t0[-(int)l] = make_double2(m.x, -m.y);
        }
        __syncthreads();
        const int n_out = items * ll;                            // gr_complex of the tile's output
        float2 *dst = a.out + (size_t)tb * a.tile_items * ll;
        for (int q = threadIdx.x; 2 * q < n_out; q += kItemTileThreads) {
            const float2 v0 = coarray_element<MODE>(t, a, 2u * q);
            if (2 * q + 1 < n_out) {
                const float2 v1 = coarray_element<MODE>(t, a, 2u * q + 1);
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
        // (the next round's stage.put overwrites the tile, which was last read before the second barrier above; its lag sums
        // overwrite t only after the next round's first barrier, which every thread reaches after its reads of t here)
    }
}

// The layout checks shared by doa_coarray_lags and create: n distinct integers with a span of at most 255.  On success
// *contiguous_size = Lc and count[l] = c_l for every lag 0 .. 255 (0 beyond the span).
static int coarray_layout(const char *who, const int *positions, int n, int min_n, int *contiguous_size, int (&count)[256])
{
    if (!positions) { set_error("%s: positions is NULL", who); return DOA_ERR_INVALID_ARG; }
    if (n < min_n || n > DOA_MAX_ANT_ELE) {
        set_error("%s: need %d <= num_ant_ele <= %d positions (got %d)", who, min_n, DOA_MAX_ANT_ELE, n);
        return DOA_ERR_INVALID_ARG;
    }
    const long long lo = *std::min_element(positions, positions + n), hi = *std::max_element(positions, positions + n);
    if (hi - lo > 255) {
        set_error("%s: the positions span %lld element spacings, more than 255", who, hi - lo);
        return DOA_ERR_INVALID_ARG;
    }
    std::fill(count, count + 256, 0);
    for (int a = 0; a < n; a++) {
        for (int b = 0; b < n; b++) {
            if (a != b && positions[a] == positions[b]) {
                set_error("%s: positions %d and %d are both %d; the positions must be distinct", who, std::min(a, b), std::max(a, b),
                          positions[a]);
                return DOA_ERR_INVALID_ARG;
            }
            if (positions[a] >= positions[b]) count[positions[a] - positions[b]]++;
        }
    }
    int lc = 0;
    while (lc < 256 && count[lc]) lc++;
    *contiguous_size = lc;
    return DOA_OK;
}

// positions and virtual_size as create has validated them
int CoarrayTables::build(const int *positions, int num_ant_ele, int virtual_size, int mode_)
{
    N = num_ant_ele; Lv = virtual_size; mode = mode_;
    CoarrayList list = {};
    int k = 0;
    for (int l = 0; l < Lv; l++) {
        list.start[l] = (unsigned short)k;
        for (int b = 0; b < N; b++)                               // ascending column b, then ascending row a
            for (int a = 0; a < N; a++)
                if (positions[a] - positions[b] == l && k < kCoarrayMaxPairs)
                    list.pair[k++] = a <= b ? (unsigned short)(a + b * N) : (unsigned short)((b + a * N) | kCoarrayConj);
        list.inv_c[l] = 1.0 / (k - list.start[l]);
    }
    for (int l = Lv; l < DOA_MAX_ANT_ELE + 2; l++) list.start[l] = (unsigned short)k;
    if (int rc = d_pairs.reserve(sizeof list); rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_pairs.p, &list, sizeof list, hipMemcpyHostToDevice));
    return DOA_OK;
}

// Items of one tile, an even number.  At most what the tile's LDS holds (kItemTileBytes of input, kCoarrayLagSlots entries of t);
// at least what gives every thread a pair of output elements; between the two, what spreads n_items over four tiles per
// compute unit: a sparse array's items are small (4 antennas: 64 to a full tile), so full tiles would leave most of the
// device without a workgroup at the batch sizes of a flowgraph.  An item's bits do not depend on the tile it falls into.
static int coarray_tile_items(int N, int Lv, int n_items, int cus)
{
    const int most = std::min(item_tile_items(N * N), (kCoarrayLagSlots / (2 * Lv - 1)) & ~1);          // 4 (N = 16) .. 256 (N = 2)
    const int least = std::min(most, ((2 * kItemTileThreads + Lv * Lv - 1) / (Lv * Lv) + 1) & ~1);
    const int spread = (int)std::min<long long>(most, (((long long)n_items + 4LL * cus - 1) / (4LL * cus) + 1) & ~1LL);
    return std::max(least, spread);
}

// d_out must not overlap d_R (not checked): a workgroup reads its tile after other workgroups have stored theirs
int launch_coarray_covariance(const CoarrayTables &t, int n_items, const void *d_R, void *d_out, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    const uintptr_t both = reinterpret_cast<uintptr_t>(d_R) | reinterpret_cast<uintptr_t>(d_out);
    if (t.N < 2 || t.N > DOA_MAX_ANT_ELE || t.Lv < 2 || t.Lv > DOA_MAX_ANT_ELE || !t.d_pairs.p || !d_R || !d_out ||
        both % sizeof(float2)) {
        set_error("coarray_covariance: bad arguments (N=%d, virtual size %d, or items not 8-byte aligned)", t.N, t.Lv);
        return DOA_ERR_INVALID_ARG;
    }
    CoarrayArgs a;
    a.in = static_cast<const float2 *>(d_R); a.out = static_cast<float2 *>(d_out);
    a.list = t.d_pairs.as<CoarrayList>();
    a.N = t.N; a.Lv = t.Lv; a.n_items = n_items;
    a.tile_items = coarray_tile_items(t.N, t.Lv, n_items, cu_count());
    a.by_ll = GroupSplit::make(t.Lv * t.Lv); a.by_l = GroupSplit::make(t.Lv);
    a.inv_lv = 1.0 / t.Lv;
    int blocks = (n_items + a.tile_items - 1) / a.tile_items;
    if (blocks > cu_count() * 4) blocks = cu_count() * 4;        // four tiles per CU, grid-stride beyond
    const bool v16 = (both & 15) == 0;
    const dim3 grid(blocks), block(kItemTileThreads);
    if (t.mode == DOA_COARRAY_TOEPLITZ) {
        if (v16) hipLaunchKernelGGL((coarray_covariance_kernel<true, DOA_COARRAY_TOEPLITZ>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((coarray_covariance_kernel<false, DOA_COARRAY_TOEPLITZ>), grid, block, 0, st, a);
    } else {
        if (v16) hipLaunchKernelGGL((coarray_covariance_kernel<true, DOA_COARRAY_SMOOTHED>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((coarray_covariance_kernel<false, DOA_COARRAY_SMOOTHED>), grid, block, 0, st, a);
    }
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

#include "block_host.hpp"

struct doa_coarray_covariance : doa::BlockBase {
    doa::CoarrayTables tables;
    doa::DevBuf d_in, d_out;
};

extern "C" {

int doa_coarray_lags(const int *positions, int n, int *contiguous_size, int *counts)
{
    doa::clear_error();
    if (!contiguous_size) { doa::set_error("coarray_lags: contiguous_size is NULL"); return DOA_ERR_INVALID_ARG; }
    int count[256];
    if (int rc = doa::coarray_layout("coarray_lags", positions, n, 1, contiguous_size, count); rc != DOA_OK) return rc;
    if (counts) std::copy(count, count + *contiguous_size, counts);
    return DOA_OK;
}

doa_coarray_covariance_t *doa_coarray_covariance_create(const int *positions, int num_ant_ele, int virtual_size, int mode)
{
    doa::clear_error();
    int lc = 0, count[256];
    if (doa::coarray_layout("coarray_covariance", positions, num_ant_ele, 2, &lc, count) != DOA_OK) return nullptr;
    if (lc < 2) {
        doa::set_error("coarray_covariance: no pair of elements is one spacing apart (contiguous size %d): nothing to build a "
                       "virtual array from", lc);
        return nullptr;
    }
    const int most = std::min(lc, DOA_MAX_ANT_ELE);
    if (virtual_size != 0 && (virtual_size < 2 || virtual_size > most)) {
        doa::set_error("coarray_covariance: need virtual_size 0 or 2 .. %d (the contiguous size of these positions is %d, "
                       "DOA_MAX_ANT_ELE %d; got %d)", most, lc, DOA_MAX_ANT_ELE, virtual_size);
        return nullptr;
    }
    if (mode != DOA_COARRAY_SMOOTHED && mode != DOA_COARRAY_TOEPLITZ) {
        doa::set_error("coarray_covariance: mode must be DOA_COARRAY_SMOOTHED (0) or DOA_COARRAY_TOEPLITZ (1), got %d", mode);
        return nullptr;
    }
    return doa::create_block<doa_coarray_covariance>("coarray_covariance", [&](doa_coarray_covariance &h) {
        return h.tables.build(positions, num_ant_ele, virtual_size ? virtual_size : most, mode);
    });
}

void doa_coarray_covariance_destroy(doa_coarray_covariance_t *h) { doa::destroy_block(h); }

int doa_coarray_covariance_virtual_size(const doa_coarray_covariance_t *h) { return h ? h->tables.Lv : 0; }

int doa_coarray_covariance_work_dev(doa_coarray_covariance_t *h, int noutput_items, const void *d_cov_items, void *d_output_items,
                                    void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("coarray_covariance_work_dev", h, noutput_items, {d_cov_items, d_output_items}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int rc = doa::launch_coarray_covariance(h->tables, noutput_items, d_cov_items, d_output_items,
                                                  static_cast<hipStream_t>(hip_stream));
    return rc == DOA_OK ? noutput_items : rc;
}

int doa_coarray_covariance_work(doa_coarray_covariance_t *h, int noutput_items, const void *cov_items, void *output_items)
{
    doa::clear_error();
    if (int rc = doa::work_args("coarray_covariance_work", h, noutput_items, {cov_items, output_items}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, (size_t)noutput_items * h->tables.N * h->tables.N * sizeof(float2));
    io.out(h->d_out, output_items, (size_t)noutput_items * h->tables.Lv * h->tables.Lv * sizeof(float2));
    int rc = io.status();
    if (rc == DOA_OK) rc = doa_coarray_covariance_work_dev(h, noutput_items, h->d_in.p, h->d_out.p, h->stream);
    return io.finish(rc);
}

}  // extern "C"
