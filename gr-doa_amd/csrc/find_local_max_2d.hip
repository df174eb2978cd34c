// find_local_max_2d.hip — the top-M local maxima of an azimuth x elevation grid, each reported as a pair (azimuth, elevation).
//
// Not a block of the reference.  The rule (8-neighbourhood, optional wrap of the azimuth index, NaN neighbours skipped, ties
// to the lowest flat index, outputs paired and NaN-filled) is stated once in include/doa_hip.h and restated in numpy in
// tests/peaks2d_ref.py.  Compare and integer logic only: the result is bit-exact and depends on the item alone, not on the
// launch geometry, the batch size or the item's neighbours in the batch.
//
// Kernel shape: one workgroup of four waves per item.
//   staged form (n_az * n_el <= 16384): the row is read from HBM once into LDS; every cell's peak test runs on the LDS row
//     (cell base + lane, so the eight neighbour reads of a wave are to consecutive words), and a ballot turns the 64 results
//     into one flag word in LDS -- P bits, whatever the row holds: no candidate list, nothing that can overflow, and no
//     atomic whose order could show in the result.  Thread t then owns flag word t, and the top M are M rounds of a workgroup
//     arg-max over the flagged cells with the key (value descending, index ascending), each round strictly after the
//     previous round's key (peak_device.hpp: cand_better, wave_argbest; the four wave results meet in LDS).
//   global form (any larger grid, up to 2^24 cells): P flag bits no longer fit in LDS, so nothing is kept: each round walks
//     the row in global memory, eight loads in flight per thread, and tests a cell's neighbours (global reads, cache hits) only
//     if the cell is after the previous key AND beats the thread's best so far -- a handful of tests per thread and round on
//     a spectrum, at worst one per cell -- leaving a test at the first neighbour row that rules the cell out.  The row is
//     read M times; the form exists so that the entry is total, not to be fast.
// No scratch memory (the Makefile checks the compiler's resource report).  Measurements: profiles/peak_pick_2d.txt, DESIGN.md
// section 3 ("Two-dimensional peak pick").
#include "kernels.hpp"
#include "peak_device.hpp"

#include <cmath>
#include <vector>

namespace doa {

namespace {

constexpr int kPeaks2dStagedMax = 16384;     // floats of LDS row: 64 KiB, two workgroups per CU
constexpr int kLoads = 8;                    // the global form: values a thread fetches before it looks at any

// PMAX > 0: the staged form for grids of up to PMAX cells (a multiple of 64, at most 64 * 256); PMAX == 0: the global form
template <int PMAX>
__global__ __launch_bounds__(kPeaks2dThreads) void find_local_max_2d_kernel(const float *__restrict__ in, const float *__restrict__ az,
                                                                            const float *__restrict__ el, float *__restrict__ out_val,
                                                                            float *__restrict__ out_az, float *__restrict__ out_el,
                                                                            Grid2d g, int M, int vec4, int stride)
{
    constexpr bool kStaged = PMAX > 0;
    static_assert(PMAX % 64 == 0 && PMAX <= 64 * kPeaks2dThreads, "one flag word per thread");
    __shared__ __attribute__((aligned(16))) float row[kStaged ? PMAX : 4];
    __shared__ unsigned long long flags[kStaged ? PMAX / 64 : 1];
    __shared__ float sv[2][4];
    __shared__ int si[2][4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const size_t item = blockIdx.x;
    const int P = g.P;
    const float *v_in = in + item * (size_t)P;

    // only the global form takes an output stride (its one caller with one is the grid mode's two-launch route, which starts
    // where the staged forms end); the staged forms write M floats per item and pay nothing for it
    const Peaks2dOut o{az, el, out_val, out_az, out_el, M, kStaged ? M : stride};
    const auto best = [&](float &v, int &i, int round) { block_argbest(v, i, sv, si, round); };
    if constexpr (kStaged) {
        if (vec4) {                          // P % 4 == 0 and 16-byte aligned rows
            for (int q = tid; q < (P >> 2); q += kPeaks2dThreads)
                reinterpret_cast<float4 *>(row)[q] = load_f4<true>(reinterpret_cast<const float4 *>(v_in) + q);
        } else {
            for (int p = tid; p < P; p += kPeaks2dThreads) row[p] = __builtin_nontemporal_load(v_in + p);
        }
        __syncthreads();
        const auto lds = [&](int j) { return row[j]; };
        for (int base = tid - lane; base < P; base += kPeaks2dThreads) {      // wave-uniform: 64 consecutive cells per step
            const int i = base + lane;
            const bool pk = (i < P) && is_peak<false>(lds, g, i, row[i < P ? i : 0]);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pk);
            if (lane == 0) flags[base >> 6] = m;
        }
        __syncthreads();
        const unsigned long long mine = (64 * tid < P) ? flags[tid] : 0ull;      // the flags of cells 64 tid .. 64 tid + 63
        peaks2d_rounds(g, o, item, tid,
                       [&](bool first, float pv, int pi, float &bv, int &bi) { flagged_best(row, mine, tid, first, pv, pi, bv, bi); }, best);
    } else {
        const auto glb = [&](int j) { return v_in[j]; };
        peaks2d_rounds(g, o, item, tid, [&](bool first, float pv, int pi, float &bv, int &bi) {
            // kLoads values in flight per thread before any is looked at: the walk is a chain of load latencies otherwise
            for (int i0 = tid; i0 < P; i0 += kLoads * kPeaks2dThreads) {
                float c[kLoads];
#pragma unroll
                for (int u = 0; u < kLoads; u++) {
                    const int i = i0 + u * kPeaks2dThreads;
                    c[u] = v_in[i < P ? i : i0];
                }
#pragma unroll
                for (int u = 0; u < kLoads; u++) {
                    const int i = i0 + u * kPeaks2dThreads;
                    if (i < P && (first || key_after(c[u], i, pv, pi)) && cand_better(c[u], i, bv, bi) && is_peak<true>(glb, g, i, c[u])) {
                        bv = c[u]; bi = i;
                    }
                }
            }
        }, best);
    }
}

template <int PMAX>
void launch_form(const Peaks2dTables &t, const Grid2d &g, int n_items, const void *d_in, void *d_val, void *d_az, void *d_el,
                 int vec4, int stride, hipStream_t st)
{
    hipLaunchKernelGGL((find_local_max_2d_kernel<PMAX>), dim3(n_items), dim3(kPeaks2dThreads), 0, st, (const float *)d_in,
                       t.d_az.as<float>(), t.d_el.as<float>(), (float *)d_val, (float *)d_az, (float *)d_el, g, t.M, vec4, stride);
}

}  // namespace

bool peaks2d_args_ok(const char *who, int num_max_vals, int n_az, int n_el, double az_min, double az_max, double el_min,
                     double el_max)
{
    if (num_max_vals < 1 || num_max_vals > DOA_MAX_PEAKS) {
        set_error("%s: need 1 <= num_max_vals <= DOA_MAX_PEAKS = %d (got %d)", who, DOA_MAX_PEAKS, num_max_vals);
        return false;
    }
    if (n_az < 1 || n_el < 1 || (long long)n_az * n_el > kPeaks2dMaxCells) {
        set_error("%s: need n_az >= 1, n_el >= 1 and n_az * n_el <= %d (got %d, %d)", who, kPeaks2dMaxCells, n_az, n_el);
        return false;
    }
    if (!std::isfinite(az_min) || !std::isfinite(az_max) || !std::isfinite(el_min) || !std::isfinite(el_max) || !(az_max > az_min) ||
        !(el_max > el_min)) {
        set_error("%s: need finite limits with az_max > az_min and el_max > el_min (got %g, %g, %g, %g)", who, az_min, az_max, el_min,
                  el_max);
        return false;
    }
    return true;
}

int Peaks2dTables::build(int num_max_vals, int n_az_, int n_el_, float az_min, float az_max, float el_min, float el_max, int wrap_az)
{
    M = num_max_vals; n_az = n_az_; n_el = n_el_; wrap = wrap_az ? 1 : 0;
    // formed in double, the end point excluded: the formulas of doa_planar_steering_table / _grid
    const auto axis = [](double lo, double hi, int n) {
        std::vector<float> x((size_t)n);
        for (int k = 0; k < n; k++) x[k] = (float)(lo + (double)k * (hi - lo) / (double)n);
        return x;
    };
    const std::vector<float> a = axis(az_min, az_max, n_az), e = axis(el_min, el_max, n_el);
    int rc = d_az.reserve(a.size() * sizeof(float));
    if (rc == DOA_OK) rc = d_el.reserve(e.size() * sizeof(float));
    if (rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_az.p, a.data(), a.size() * sizeof(float), hipMemcpyHostToDevice));
    DOA_HIP_TRY(hipMemcpy(d_el.p, e.data(), e.size() * sizeof(float), hipMemcpyHostToDevice));
    return DOA_OK;
}

int launch_find_local_max_2d(const Peaks2dTables &t, int n_items, const void *d_in, void *d_val, void *d_az, void *d_el,
                             hipStream_t st, int stride_az_el)
{
    if (n_items <= 0) return DOA_OK;
    const long long cells = (long long)t.n_az * t.n_el;
    const bool stride_ok = stride_az_el <= 0 || stride_az_el == t.M || (stride_az_el > t.M && cells > kPeaks2dStagedMax);
    if (t.M < 1 || t.M > DOA_MAX_PEAKS || t.n_az < 1 || t.n_el < 1 || cells > kPeaks2dMaxCells || !stride_ok || !t.d_az.p ||
        !t.d_el.p || !d_in || !d_val || !d_az || !d_el) {
        set_error("find_local_max_2d: bad arguments of the launch (M=%d, grid %d x %d)", t.M, t.n_az, t.n_el);
        return DOA_ERR_INVALID_ARG;
    }
    const int P = (int)cells, stride = stride_az_el > 0 ? stride_az_el : t.M;
    const Grid2d g = make_grid2d(t.n_az, t.n_el, t.wrap);
    const int vec4 = (P % 4 == 0 && reinterpret_cast<uintptr_t>(d_in) % 16 == 0) ? 1 : 0;
    // two staged sizes, so that a small grid does not take a large grid's 64 KiB of LDS and its two workgroups per CU
    if (P <= 2048) launch_form<2048>(t, g, n_items, d_in, d_val, d_az, d_el, vec4, stride, st);
    else if (P <= kPeaks2dStagedMax) launch_form<kPeaks2dStagedMax>(t, g, n_items, d_in, d_val, d_az, d_el, vec4, stride, st);
    else launch_form<0>(t, g, n_items, d_in, d_val, d_az, d_el, 0, stride, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"

struct doa_find_local_max_2d : doa::BlockBase {
    doa::Peaks2dTables tab;
    doa::DevBuf d_in, d_out0, d_out1, d_out2;
};

extern "C" {

doa_find_local_max_2d_t *doa_find_local_max_2d_create(int num_max_vals, int n_az, int n_el, float az_min, float az_max,
                                                      float el_min, float el_max, int wrap_az)
{
    doa::clear_error();
    if (!doa::peaks2d_args_ok("find_local_max_2d", num_max_vals, n_az, n_el, az_min, az_max, el_min, el_max)) return nullptr;
    return doa::create_block<doa_find_local_max_2d>("find_local_max_2d", [&](doa_find_local_max_2d &h) {
        return h.tab.build(num_max_vals, n_az, n_el, az_min, az_max, el_min, el_max, wrap_az);
    });
}

void doa_find_local_max_2d_destroy(doa_find_local_max_2d_t *h) { doa::destroy_block(h); }

long long doa_find_local_max_2d_items_total(const doa_find_local_max_2d_t *h) { return h ? h->items_total : 0; }

int doa_find_local_max_2d_work_dev(doa_find_local_max_2d_t *h, int noutput_items, const void *d_input_items0, void *d_output_items0,
                                   void *d_output_items1, void *d_output_items2, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("find_local_max_2d_work_dev", h, noutput_items,
                                {d_input_items0, d_output_items0, d_output_items1, d_output_items2});
        rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int rc = doa::launch_find_local_max_2d(h->tab, noutput_items, d_input_items0, d_output_items0, d_output_items1,
                                                 d_output_items2, static_cast<hipStream_t>(hip_stream));
    if (rc != DOA_OK) return rc;
    h->items_total += noutput_items;
    return noutput_items;
}

int doa_find_local_max_2d_work(doa_find_local_max_2d_t *h, int noutput_items, const void *input_items0, void *output_items0,
                               void *output_items1, void *output_items2)
{
    doa::clear_error();
    if (int rc = doa::work_args("find_local_max_2d_work", h, noutput_items, {input_items0, output_items0, output_items1, output_items2});
        rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    const size_t out_bytes = (size_t)noutput_items * h->tab.M * sizeof(float);
    doa::HostCall io(*h);
    io.in(h->d_in, input_items0, (size_t)noutput_items * h->tab.cells() * sizeof(float));
    io.out(h->d_out0, output_items0, out_bytes);
    io.out(h->d_out1, output_items1, out_bytes);
    io.out(h->d_out2, output_items2, out_bytes);
    int rc = io.status();
    if (rc == DOA_OK) rc = doa_find_local_max_2d_work_dev(h, noutput_items, h->d_in.p, h->d_out0.p, h->d_out1.p, h->d_out2.p, h->stream);
    return io.finish(rc);
}

}  // extern "C"
