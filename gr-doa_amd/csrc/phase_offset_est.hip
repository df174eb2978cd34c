// phase_offset_est.hip — the constant phase offsets between N receiver channels, estimated on gfx950.
//
// Replaces the reference's hier block twinrx_phase_offset_est (python/twinrx_phase_offset_est.py:37-94: blocks.skiphead on
// every stream, blocks.complex_to_arg on every stream, blocks.sub_ff of stream 0 and stream p):
//   out_{p-1}[i] = atan2f(im x_0[i], re x_0[i]) - atan2f(im x_p[i], re x_p[i]),   p = 1 .. N-1,
// one float subtraction, NOT wrapped into any interval (the range (-2 pi, 2 pi) is what the reference's savers see), and
// -- fused with it -- the reductions its consumers take of those floats: numpy.amax (python/findmax_and_save.py:66-78),
// numpy.mean (python/average_and_save.py:68-80), plus the branch-free estimate arg(sum_i x_0[i] conj(x_p[i])).
//
// Streaming form (poe_stream_kernel): one sample per lane, N loads, N atan2f, N-1 stores.
// Fused form (poe_partial_kernel + poe_combine_kernel): the streams are read once and 3(N-1) floats are written.
//   The sample range is cut into chunks of kChunk samples, a function of `samples` alone.  One wave owns a chunk: lane l
//   takes the sample pairs l, l + 64, ... of the chunk in ascending order (16-byte non-temporal loads when every stream is
//   aligned to two samples, two one-sample loads otherwise: the same samples meet the same accumulators in the same order
//   either way), keeps per p a float maximum and three double sums in registers, the 64 lanes meet in a fixed xor
//   butterfly and lane 0 writes one 32-byte partial per (chunk, p).  poe_combine_kernel then folds the partials of each p
//   in a fixed order (thread t takes chunks t, t + 256, ...; fixed LDS tree).  No atomics; the result does not depend on
//   the grid, on the alignment route or on how a host caller's samples were staged.
// atan2f is the device library's (see DESIGN.md section 7 for the instruction count and where the kernel sits).
#include "block_host.hpp"
#include "kernels.hpp"
#include "sample_loaders.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace doa {

constexpr int kChunk = 4096;           // samples per partial (64 per lane)

struct PoePartial {                    // one per (chunk, p)
    double sum, re, im;
    float mx, pad;
};

struct PoeArgs {
    const void *in[DOA_MAX_ANT_ELE];   // N streams of the loader's sample type, at the first sample this launch reads
    float *out[DOA_MAX_ANT_ELE - 1];   // streaming form: N-1 float streams
    long long n;                       // samples this launch reads per stream
    PoePartial *part;                  // fused form: [chunks of the whole range][N-1]
    int chunk0;                        // fused form: index of this launch's first chunk in the whole range
    int n_chunks;                      // chunks of this launch
    int n_ch;                          // N
    int vec2;                          // every stream aligned to two samples: pair loads
    float scale;                       // sc16 widening factor
};

template <class L> __device__ __forceinline__ const typename L::sample_t *poe_stream(const PoeArgs &g, int k)
{
    return static_cast<const typename L::sample_t *>(g.in[k]);
}

// the one place the per-sample float is formed: both forms call it, so the fused maximum is a maximum of the very floats
// the streaming form writes
// A component that is not finite (NaN or Inf) gives NaN, not the limit atan2f defines for an infinite operand: such a
// sample is no measurement, and this way every reduction over it says so.
__device__ __forceinline__ float poe_arg(float2 x)
{
    const float a = atan2f(x.y, x.x);
    return (__builtin_isfinite(x.x) && __builtin_isfinite(x.y)) ? a : __builtin_nanf("");
}
__device__ __forceinline__ float poe_diff(float a0, float2 xp) { return __fsub_rn(a0, poe_arg(xp)); }

template <class L> __global__ __launch_bounds__(256) void poe_stream_kernel(PoeArgs g)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
        const float a0 = poe_arg(L::one(poe_stream<L>(g, 0) + i, g.scale));
        for (int p = 1; p < g.n_ch; p++) g.out[p - 1][i] = poe_diff(a0, L::one(poe_stream<L>(g, p) + i, g.scale));
    }
}

template <int TCAP> struct PoeAcc {
    float mx[TCAP - 1];
    double sum[TCAP - 1], re[TCAP - 1], im[TCAP - 1];
};

// samples 2q and 2q + 1 of the chunk that starts at `base` (cnt samples) as (re, im, re, im); the second is zero when the
// chunk ends on an odd sample (the caller does not take it)
template <class L, int TCAP>
__device__ __forceinline__ void poe_load(const PoeArgs &g, long long base, int q, int cnt, float4 (&v)[TCAP])
{
    const long long i = base + 2 * (long long)q;
    const bool full = 2 * q + 1 < cnt;
    if (g.vec2 && full) {
#pragma unroll
        for (int k = 0; k < TCAP; k++)
            if (k < g.n_ch) v[k] = L::template pair<true>(poe_stream<L>(g, k) + i, g.scale);
    } else {
#pragma unroll
        for (int k = 0; k < TCAP; k++)
            if (k < g.n_ch) {
                const float2 a = L::one(poe_stream<L>(g, k) + i, g.scale);
                const float2 b = full ? L::one(poe_stream<L>(g, k) + i + 1, g.scale) : make_float2(0.f, 0.f);
                v[k] = make_float4(a.x, a.y, b.x, b.y);
            }
    }
}

template <int TCAP> __device__ __forceinline__ void poe_sample(PoeAcc<TCAP> &acc, int n_ch, const float2 (&x)[TCAP])
{
    const float a0 = poe_arg(x[0]);
    const double x0r = x[0].x, x0i = x[0].y;
#pragma unroll
    for (int p = 1; p < TCAP; p++)
        if (p < n_ch) {
            const float d = poe_diff(a0, x[p]);
            acc.mx[p - 1] = nan_max(acc.mx[p - 1], d);
            acc.sum[p - 1] += (double)d;
            // x_0 conj(x_p); a product of two floats is exact in double, only the sum rounds
            const double pr = x[p].x, pi = x[p].y;
            acc.re[p - 1] = fma(x0r, pr, fma(x0i, pi, acc.re[p - 1]));
            acc.im[p - 1] = fma(x0i, pr, fma(-x0r, pi, acc.im[p - 1]));
        }
}

// TCAP: streams the kernel is unrolled for (n_ch <= TCAP; the unused ones are skipped by wave-uniform branches)
template <class L, int TCAP> __global__ __launch_bounds__(256) void poe_partial_kernel(PoeArgs g)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave0 = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const int n_waves = gridDim.x * (blockDim.x / kWave);
    for (int lc = wave0; lc < g.n_chunks; lc += n_waves) {
        const long long base = (long long)lc * kChunk;
        const int cnt = (g.n - base < kChunk) ? (int)(g.n - base) : kChunk;
        const int nq = (cnt + 1) >> 1;                 // pairs, the last one half empty when cnt is odd
        PoeAcc<TCAP> acc;
#pragma unroll
        for (int p = 0; p < TCAP - 1; p++) { acc.mx[p] = -INFINITY; acc.sum[p] = 0.0; acc.re[p] = 0.0; acc.im[p] = 0.0; }

        // one iteration of loads stays in flight under the arithmetic of the previous one
        float4 cur[TCAP], nxt[TCAP];
#pragma unroll
        for (int k = 0; k < TCAP; k++) cur[k] = nxt[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < nq) poe_load<L, TCAP>(g, base, lane, cnt, cur);
        for (int q = lane; q < nq; q += kWave) {
            if (q + kWave < nq) poe_load<L, TCAP>(g, base, q + kWave, cnt, nxt);
            float2 x0[TCAP], x1[TCAP];
#pragma unroll
            for (int k = 0; k < TCAP; k++) { x0[k] = make_float2(cur[k].x, cur[k].y); x1[k] = make_float2(cur[k].z, cur[k].w); }
            poe_sample<TCAP>(acc, g.n_ch, x0);
            if (2 * q + 1 < cnt) poe_sample<TCAP>(acc, g.n_ch, x1);
#pragma unroll
            for (int k = 0; k < TCAP; k++) cur[k] = nxt[k];
        }

        PoePartial *po = g.part + (size_t)(g.chunk0 + lc) * (g.n_ch - 1);
#pragma unroll
        for (int p = 0; p < TCAP - 1; p++)
            if (p < g.n_ch - 1) {
                PoePartial r;
                r.sum = wave_butterfly_sum_xor(acc.sum[p]);
                r.re = wave_butterfly_sum_xor(acc.re[p]);
                r.im = wave_butterfly_sum_xor(acc.im[p]);
                r.mx = wave_butterfly_nan_max(acc.mx[p]);
                r.pad = 0.f;
                if (lane == 0) po[p] = r;
            }
    }
}

// one block per p: folds the partials of all chunks (fixed order) and writes whichever results are wanted
__global__ __launch_bounds__(256) void poe_combine_kernel(const PoePartial *__restrict__ part, int n_chunks, int n_out,
                                                          long long samples, float *mean_out, float *max_out, float *circ_out)
{
    __shared__ double s_sum[256], s_re[256], s_im[256];
    __shared__ float s_mx[256];
    const int p = blockIdx.x, t = threadIdx.x;
    double sum = 0.0, re = 0.0, im = 0.0;
    float mx = -INFINITY;
#pragma unroll 8                                   // the loads of eight trips go out together; the sums keep their order
    for (int c = t; c < n_chunks; c += 256) {
        const PoePartial r = part[(size_t)c * n_out + p];
        sum += r.sum; re += r.re; im += r.im; mx = nan_max(mx, r.mx);
    }
    s_sum[t] = sum; s_re[t] = re; s_im[t] = im; s_mx[t] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            s_sum[t] += s_sum[t + s]; s_re[t] += s_re[t + s]; s_im[t] += s_im[t + s];
            s_mx[t] = nan_max(s_mx[t], s_mx[t + s]);
        }
        __syncthreads();
    }
    if (t == 0) {
        if (mean_out) mean_out[p] = (float)(s_sum[0] / (double)samples);
        if (max_out) max_out[p] = s_mx[0];
        if (circ_out) circ_out[p] = (float)atan2(s_im[0], s_re[0]);
    }
}

static bool poe_fill_streams(PoeArgs &g, const char *what, int N, const void *const *d_in, size_t skip_samples, size_t sb)
{
    bool pair_aligned;                  // judged after the skip, where the kernel starts to read
    if (check_streams(what, d_in, N, sb, &pair_aligned, -1, skip_samples * sb) != DOA_OK) return false;
    g.vec2 = pair_aligned;
    for (int k = 0; k < N; k++) g.in[k] = static_cast<const char *>(d_in[k]) + skip_samples * sb;
    for (int k = N; k < DOA_MAX_ANT_ELE; k++) g.in[k] = g.in[0];
    return true;
}

template <class L> static void poe_launch_partial(const PoeArgs &g, hipStream_t st)
{
    const int waves_per_block = 4;
    int blocks = (g.n_chunks + waves_per_block - 1) / waves_per_block;
    const int cap = cu_count() * 16 / waves_per_block;          // <= 16 waves per CU, grid-stride beyond
    if (blocks > cap) blocks = cap;
    const dim3 grid(blocks), block(waves_per_block * kWave);
    if (g.n_ch <= 4)      hipLaunchKernelGGL((poe_partial_kernel<L, 4>), grid, block, 0, st, g);
    else if (g.n_ch <= 8) hipLaunchKernelGGL((poe_partial_kernel<L, 8>), grid, block, 0, st, g);
    else                  hipLaunchKernelGGL((poe_partial_kernel<L, 16>), grid, block, 0, st, g);
}

static inline int poe_chunks(long long samples) { return (int)((samples + kChunk - 1) / kChunk); }

// partials of chunks chunk0 .. of the whole range from the n samples at d_in (+ skip_samples); d_part holds the whole range
static int launch_poe_partial(int N, int format, float scale, const void *const *d_in, size_t skip_samples, long long n,
                              int chunk0, void *d_part, hipStream_t st)
{
    PoeArgs g;
    memset(&g, 0, sizeof g);
    if (!poe_fill_streams(g, "phase_offset_est_estimate", N, d_in, skip_samples, sample_bytes(format))) return DOA_ERR_INVALID_ARG;
    g.n = n; g.n_ch = N; g.part = static_cast<PoePartial *>(d_part); g.chunk0 = chunk0; g.n_chunks = poe_chunks(n);
    g.scale = (format == DOA_SAMPLE_SC16) ? scale : 1.0f;
    if (format == DOA_SAMPLE_SC16) poe_launch_partial<Sc16Samples>(g, st);
    else                           poe_launch_partial<Fc32Samples>(g, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

static int launch_poe_combine(int N, long long samples, const void *d_part, float *d_mean, float *d_max, float *d_circ,
                              hipStream_t st)
{
    hipLaunchKernelGGL(poe_combine_kernel, dim3(N - 1), dim3(256), 0, st, static_cast<const PoePartial *>(d_part),
                       poe_chunks(samples), N - 1, samples, d_mean, d_max, d_circ);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

static int launch_poe_stream(int N, int format, float scale, const void *const *d_in, size_t skip_samples, long long n,
                             void *const *d_out, hipStream_t st)
{
    if (n <= 0) return DOA_OK;
    PoeArgs g;
    memset(&g, 0, sizeof g);
    if (!poe_fill_streams(g, "phase_offset_est_work", N, d_in, skip_samples, sample_bytes(format))) return DOA_ERR_INVALID_ARG;
    for (int p = 0; p < N - 1; p++) {
        if (!d_out[p]) { set_error("phase_offset_est_work: output stream %d is NULL", p); return DOA_ERR_INVALID_ARG; }
        g.out[p] = static_cast<float *>(d_out[p]);
    }
    g.n = n; g.n_ch = N;
    g.scale = (format == DOA_SAMPLE_SC16) ? scale : 1.0f;
    long long blocks = (n + 255) / 256;
    if (blocks > 8LL * cu_count()) blocks = 8LL * cu_count();
    if (format == DOA_SAMPLE_SC16) hipLaunchKernelGGL(poe_stream_kernel<Sc16Samples>, dim3((unsigned)blocks), dim3(256), 0, st, g);
    else                           hipLaunchKernelGGL(poe_stream_kernel<Fc32Samples>, dim3((unsigned)blocks), dim3(256), 0, st, g);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

// samples per stream the host entries stage per copy: ~32 MiB over the N streams, a whole number of chunks
static long long poe_stage_samples(int N, size_t sb)
{
    long long s = (long long)((32u << 20) / ((size_t)N * sb));
    s -= s % kChunk;
    return s < kChunk ? kChunk : s;
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct doa_phase_offset_est : doa::BlockBase {
    int N = 0;
    long long n_skip = 0;               // blocks.skiphead's argument
    long long skipped = 0;              // samples dropped so far (the skiphead state): moves only when a call has succeeded
    doa::InputFormat fmt;
    doa::DevBuf d_in, d_out, d_part, d_res[3];
    long long owed() const { return n_skip > skipped ? n_skip - skipped : 0; }
};

extern "C" {

doa_phase_offset_est_t *doa_phase_offset_est_create(int num_ports, int n_skip_ahead)
{
    doa::clear_error();
    if (num_ports < 2 || num_ports > DOA_MAX_ANT_ELE) {
        doa::set_error("phase_offset_est: num_ports=%d outside 2..%d", num_ports, DOA_MAX_ANT_ELE);
        return nullptr;
    }
    if (n_skip_ahead < 0) { doa::set_error("phase_offset_est: n_skip_ahead=%d is negative", n_skip_ahead); return nullptr; }
    return doa::create_block<doa_phase_offset_est>("phase_offset_est", [&](doa_phase_offset_est &h) {
        h.N = num_ports; h.n_skip = n_skip_ahead;
        return (int)DOA_OK;
    });
}

void doa_phase_offset_est_destroy(doa_phase_offset_est_t *h) { doa::destroy_block(h); }

int doa_phase_offset_est_reset(doa_phase_offset_est_t *h)
{
    doa::clear_error();
    if (!h) { doa::set_error("phase_offset_est_reset: bad arguments"); return DOA_ERR_INVALID_ARG; }
    h->skipped = 0;
    return DOA_OK;
}

int doa_phase_offset_est_set_input_format(doa_phase_offset_est_t *h, int format, float scale)
{
    doa::clear_error();
    return doa::set_input_format("phase_offset_est", h ? &h->fmt : nullptr, format, scale);
}

int doa_phase_offset_est_work_dev(doa_phase_offset_est_t *h, int n_items, const void *const *d_input_items,
                                  void *const *d_output_items, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("phase_offset_est_work_dev", h, n_items, {d_input_items, d_output_items}); rc != DOA_OK) return rc;
    if (n_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const long long drop = h->owed() < n_items ? h->owed() : n_items;
    const int produce = (int)(n_items - drop);
    const int rc = doa::launch_poe_stream(h->N, h->fmt.format, h->fmt.scale, d_input_items, (size_t)drop, produce, d_output_items,
                                          static_cast<hipStream_t>(hip_stream));
    if (rc != DOA_OK) return rc;
    h->skipped += drop;
    return produce;
}

int doa_phase_offset_est_work(doa_phase_offset_est_t *h, int n_items, const void *const *input_items,
                              void *const *output_items)
{
    doa::clear_error();
    if (int rc = doa::work_args("phase_offset_est_work", h, n_items, {input_items, output_items}); rc != DOA_OK) return rc;
    if (n_items == 0) return 0;
    const int N = h->N;
    for (int k = 0; k < N; k++)         // every port, also in a call the skip swallows whole
        if (!input_items[k] || (k < N - 1 && !output_items[k])) { doa::set_error("phase_offset_est_work: port %d is NULL", k); return DOA_ERR_INVALID_ARG; }
    const long long drop = h->owed() < n_items ? h->owed() : n_items;
    const long long produce = n_items - drop;
    const size_t sb = h->fmt.sample_bytes();
    const long long stage = doa::poe_stage_samples(N, sb);
    // one round trip per staged piece (the first is the largest, so the buffers grow once)
    for (long long s0 = 0; s0 < produce; s0 += stage) {
        const long long cnt = produce - s0 < stage ? produce - s0 : stage;
        doa::HostCall io(*h);
        const void *di[DOA_MAX_ANT_ELE];
        void *dout[DOA_MAX_ANT_ELE];
        io.in_streams("phase_offset_est_work", h->d_in, input_items, N, (size_t)cnt * sb, di, (size_t)(drop + s0) * sb);
        int rc = io.out_streams("phase_offset_est_work", h->d_out, output_items, N - 1, (size_t)cnt * sizeof(float),
                                ((size_t)cnt * sizeof(float) + 15) & ~(size_t)15, dout, (size_t)s0 * sizeof(float));
        if (rc == DOA_OK) rc = doa::launch_poe_stream(N, h->fmt.format, h->fmt.scale, di, 0, cnt, dout, h->stream);
        if (rc = io.finish(rc); rc != DOA_OK) return rc;
    }
    h->skipped += drop;
    return (int)produce;
}

// what both estimate entries check before they touch anything: *drop = samples the skip still takes from this call
static int poe_estimate_args(const char *what, doa_phase_offset_est_t *h, long long n_items, const void *const *inputs,
                             long long samples, long long *drop)
{
    if (!h || n_items < 0 || !inputs || samples <= 0) {
        doa::set_error("%s: bad arguments", what);
        return DOA_ERR_INVALID_ARG;
    }
    *drop = h->owed() < n_items ? h->owed() : n_items;
    if (n_items - *drop < samples) {
        doa::set_error("%s: %lld items given, %lld of them skipped, fewer than samples=%lld remain", what, n_items, *drop, samples);
        return DOA_ERR_INVALID_ARG;
    }
    return DOA_OK;
}

int doa_phase_offset_est_estimate_dev(doa_phase_offset_est_t *h, long long n_items, const void *const *d_input_items,
                                      long long samples, float *d_mean_out, float *d_max_out, float *d_circ_out,
                                      void *hip_stream)
{
    doa::clear_error();
    long long drop = 0;
    if (const int rc = poe_estimate_args("phase_offset_est_estimate_dev", h, n_items, d_input_items, samples, &drop); rc != DOA_OK) return rc;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // per-chunk partials (grow-only; growing frees the old buffer, which waits for the device)
    int rc = h->d_part.reserve((size_t)doa::poe_chunks(samples) * (h->N - 1) * sizeof(doa::PoePartial));
    if (rc != DOA_OK) return rc;
    rc = doa::launch_poe_partial(h->N, h->fmt.format, h->fmt.scale, d_input_items, (size_t)drop, samples, 0, h->d_part.p, st);
    if (rc == DOA_OK) rc = doa::launch_poe_combine(h->N, samples, h->d_part.p, d_mean_out, d_max_out, d_circ_out, st);
    if (rc != DOA_OK) return rc;
    h->skipped += drop;
    return DOA_OK;
}

int doa_phase_offset_est_estimate(doa_phase_offset_est_t *h, long long n_items, const void *const *input_items,
                                  long long samples, float *mean_out, float *max_out, float *circ_out)
{
    doa::clear_error();
    long long drop = 0;
    if (const int rc = poe_estimate_args("phase_offset_est_estimate", h, n_items, input_items, samples, &drop); rc != DOA_OK) return rc;
    const int N = h->N;
    const size_t sb = h->fmt.sample_bytes();
    const long long stage = doa::poe_stage_samples(N, sb);              // a whole number of chunks: the partition is that of
    doa::HostCall io(*h);                                               // the device entry, whatever the staging
    int rc = io.status();
    if (rc == DOA_OK) rc = h->d_part.reserve((size_t)doa::poe_chunks(samples) * (N - 1) * sizeof(doa::PoePartial));
    // (the pieces follow one another on the stream, so one staging buffer serves them all; the first is the largest)
    for (long long s0 = 0; s0 < samples && rc == DOA_OK; s0 += stage) {
        const long long cnt = samples - s0 < stage ? samples - s0 : stage;
        const void *di[DOA_MAX_ANT_ELE];
        rc = io.in_streams("phase_offset_est_estimate", h->d_in, input_items, N, (size_t)cnt * sb, di, (size_t)(drop + s0) * sb);
        if (rc == DOA_OK) rc = doa::launch_poe_partial(N, h->fmt.format, h->fmt.scale, di, 0, cnt, (int)(s0 / doa::kChunk), h->d_part.p, h->stream);
    }
    float *const host[3] = {mean_out, max_out, circ_out};
    for (int i = 0; i < 3 && rc == DOA_OK; i++) rc = io.out(h->d_res[i], host[i], (N - 1) * sizeof(float));
    if (rc == DOA_OK)
        rc = doa::launch_poe_combine(N, samples, h->d_part.p, h->d_res[0].as<float>(), h->d_res[1].as<float>(), h->d_res[2].as<float>(), h->stream);
    if (rc = io.finish(rc); rc != DOA_OK) return rc;
    h->skipped += drop;
    return DOA_OK;
}

}  // extern "C"
