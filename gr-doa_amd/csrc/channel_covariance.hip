// channel_covariance.hip — per-frequency-bin covariance (the Welch / Bartlett cross-spectral matrix) of N complex streams on
// gfx950: the front end for several narrowband emitters at different frequencies inside one captured band.
//
// Definition (include/doa_hip.h; tests/channel_covariance_ref.py restates it in numpy).  Snapshot i starts at sample
// s_i = i (K - overlap) and is cut into B = K / F blocks of F samples:
//     X[a,b,f]   = sum_t w[t] x_a[s_i + bF + t] exp(-2 pi i f t / F)
//     R_i,f[p,q] = 1 / (B W2) sum_b X[p,b,f] conj(X[q,b,f]),        W2 = sum_t w[t]^2
// Every (snapshot, bin) matrix is an ordinary column-major N x N covariance item.
//
// Kernel shape: one workgroup of four waves per snapshot.  A round takes 4 CB blocks (CB = 64 / F blocks side by side in
// one wave when F < 64, else 1): wave w loads its blocks' N F samples once from HBM (16-byte loads per lane on the pair
// route), multiplies by the window and lays them into its own rows of the LDS image; the F-point FFT runs in place there
// as radix-2 decimation-in-frequency stages, two fused per pass, and leaves the bins in bit-reversed positions.  A wave
// touches only its own rows until then, so its stages are ordered by the wave alone and a round has two workgroup barriers.
// The accumulators are distributed by bin, not by block: thread t owns position t mod F for all N antennas and keeps the
// upper triangle (N real + N(N-1)/2 complex sums) in registers, taking the blocks t / F, t / F + 256 / F, ... in
// increasing order.  The 256 / F partial sums of a bin meet in LDS in a fixed order, the scale is applied once, and the
// final store un-permutes the bins and mirrors the triangle (the lower one is the bitwise conjugate).  No atomics, no
// scratch; every product and sum is an explicit fmaf or an uncontracted operator, so the instantiations of a size (fc32 /
// sc16, pair / scalar loads) round identically and an item does not depend on how many snapshots the call has or where it
// sits in it.  Measurements: profiles/channel_covariance.txt (tools/profile_channel_covariance.py), DESIGN.md section 3.
#include "kernels.hpp"
#include "sample_loaders.hpp"
#include "block_host.hpp"

#include <cmath>
#include <cstdint>

namespace doa {

constexpr int kChanThreads = 256;          // four waves
constexpr int kChanMaxInputs = 8;          // the triangle of a wider array does not fit one lane
constexpr int kChanMaxFft = 256;

struct ChanCovArgs {
    const void *in[kChanMaxInputs];        // N streams of the loader's sample type
    float2 *out;                           // [n][num_bins][N*N]
    float *power;                          // [n][F] or nullptr
    const float2 *twiddle;                 // [F/2] exp(-2 pi i k / F), rounded from double
    const float *window;                   // [F]
    int K, S, F, lg_f, B;
    int first_bin, num_bins;
    float inv;                             // (float)(1 / (B W2))
    float scale;                           // sc16: the widening factor; unused for fc32
};

template <int TN> struct ChanTri {
    float d[TN];
    float re[TN * (TN - 1) / 2 > 0 ? TN * (TN - 1) / 2 : 1];
    float im[TN * (TN - 1) / 2 > 0 ? TN * (TN - 1) / 2 : 1];
};

// No floating-point contraction in this file: a product and a sum fuse only where fmaf says so.  (The __fmul_rn / __fadd_rn
// of the HIP headers are plain operators defined where contraction is on, and fuse with each other after inlining; the
// operators below carry no such permission, and the compiler needs it on both sides.)  That is what makes the power port
// the float sum of the stored diagonals and the four instantiations of a size bit-identical.
#pragma clang fp contract(off)
__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }

__device__ __forceinline__ float2 c_add(float2 a, float2 b) { return make_float2(f_add(a.x, b.x), f_add(a.y, b.y)); }
__device__ __forceinline__ float2 c_sub(float2 a, float2 b) { return make_float2(f_sub(a.x, b.x), f_sub(a.y, b.y)); }
__device__ __forceinline__ float2 c_mul(float2 a, float2 w)
{
    return make_float2(fmaf(a.x, w.x, -f_mul(a.y, w.y)), fmaf(a.x, w.y, f_mul(a.y, w.x)));
}

// stream a of the call, a < TN known only at run time: a select chain over the (scalar) kernel arguments, no indexed copy
template <class L, int TN> __device__ __forceinline__ const typename L::sample_t *chan_stream(const ChanCovArgs &g, int a)
{
    const typename L::sample_t *p = static_cast<const typename L::sample_t *>(g.in[0]);
#pragma unroll
    for (int k = 1; k < TN; k++)
        if (a == k) p = static_cast<const typename L::sample_t *>(g.in[k]);
    return p;
}

// Until the accumulation a wave works on its own rows of the image only, and a wave's LDS operations execute in the order
// they were issued: between its own stages it needs no workgroup barrier, only the compiler not to move them.
__device__ __forceinline__ void chan_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// LDS image: 4 waves x TN antennas x max(F, 64) points (float2), reused for the 256 TN^2 partial sums (float).  Two sizes,
// so that the short transforms leave room for more workgroups per compute unit: SMALL serves F <= 64.
constexpr int chan_image_points(int tn, bool small)
{
    return small ? (tn * 256 > tn * tn * 128 ? tn * 256 : tn * tn * 128) : tn * 1024;
}

template <class L, int TN, bool VEC2, bool SMALL>
__global__ __launch_bounds__(kChanThreads) void channel_covariance_kernel(ChanCovArgs g)
{
    __shared__ __attribute__((aligned(16))) float2 xs[chan_image_points(TN, SMALL)];
    __shared__ float2 s_tw[kChanMaxFft / 2];
    __shared__ float s_win[kChanMaxFft];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int F = g.F, lg = g.lg_f;
    const int lg_cb = lg < 6 ? 6 - lg : 0, CB = 1 << lg_cb;       // blocks side by side in one wave
    const int RB = 4 * CB;                                        // blocks per round
    const int G = kChanThreads >> lg;                             // threads per bin: RB is a multiple of it
    const int snap = blockIdx.x;
    const size_t base = (size_t)snap * (size_t)g.S;

    for (int i = tid; i < (F >> 1); i += kChanThreads) s_tw[i] = g.twiddle[i];
    for (int i = tid; i < F; i += kChanThreads) s_win[i] = g.window[i];
    __syncthreads();

    ChanTri<TN> acc;
#pragma unroll
    for (int a = 0; a < TN; a++) acc.d[a] = 0.f;
#pragma unroll
    for (int i = 0; i < TN * (TN - 1) / 2; i++) { acc.re[i] = 0.f; acc.im[i] = 0.f; }

    const int rows_w = TN << lg_cb;                               // rows of one wave: row = a * CB + cb
    float2 *xw = xs + (size_t)wave * (rows_w << lg);
    const int pos = tid & (F - 1), grp = tid >> lg;               // accumulation: this thread's bin position and block group

    for (int r0 = 0; r0 < g.B; r0 += RB) {
        const int wb0 = r0 + wave * CB;                           // this wave's first block of the round
        // ---- load, window, lay out: every sample of the snapshot is read once ----
        if constexpr (VEC2) {
            const int total = rows_w << (lg - 1);                 // sample pairs of the wave's rows
            for (int i0 = lane; i0 < total; i0 += 4 * kWave) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = i0 + u * kWave;
                    const int row = idx >> (lg - 1), pr = idx & ((F >> 1) - 1);
                    const int a = row >> lg_cb, b = wb0 + (row & (CB - 1));
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (idx < total && b < g.B)
                        v[u] = L::template pair<true>(chan_stream<L, TN>(g, a) + base + (size_t)b * F + 2 * pr, g.scale);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = i0 + u * kWave;
                    if (idx < total) {
                        const int pr = idx & ((F >> 1) - 1);
                        const float w0 = s_win[2 * pr], w1 = s_win[2 * pr + 1];
                        *reinterpret_cast<float4 *>(xw + 2 * idx) =
                            make_float4(f_mul(v[u].x, w0), f_mul(v[u].y, w0), f_mul(v[u].z, w1), f_mul(v[u].w, w1));
                    }
                }
            }
        } else {
            const int total = rows_w << lg;
            for (int i0 = lane; i0 < total; i0 += 4 * kWave) {
                float2 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = i0 + u * kWave;
                    const int row = idx >> lg, t = idx & (F - 1);
                    const int a = row >> lg_cb, b = wb0 + (row & (CB - 1));
                    v[u] = make_float2(0.f, 0.f);
                    if (idx < total && b < g.B) v[u] = L::one(chan_stream<L, TN>(g, a) + (base + (size_t)b * F + t), g.scale);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = i0 + u * kWave;
                    if (idx < total) {
                        const float w0 = s_win[idx & (F - 1)];
                        xw[idx] = make_float2(f_mul(v[u].x, w0), f_mul(v[u].y, w0));
                    }
                }
            }
        }
        chan_wave_sync();

        // ---- F-point FFT of every row, in place: radix-2 decimation in frequency, two stages per pass ----
        int lg_l = lg;                                            // log2 of the sub-transform length L
        const int n_bfly4 = rows_w << (lg - 2);
        while (lg_l >= 2) {
            const int lq = lg_l - 2, q4 = 1 << lq, ts = lg - lg_l;    // L/4; W_L^k = s_tw[k << ts]
            for (int j = lane; j < n_bfly4; j += kWave) {
                const int row = j >> (lg - 2), q = j & ((F >> 2) - 1);
                if (wb0 + (row & (CB - 1)) >= g.B) continue;
                const int i = q & (q4 - 1);
                float2 *x = xw + (row << lg) + ((q >> lq) << lg_l) + i;
                const float2 x0 = x[0], x1 = x[q4], x2 = x[2 * q4], x3 = x[3 * q4];
                const float2 wa = s_tw[i << ts], wb = s_tw[(i + q4) << ts], wc = s_tw[i << (ts + 1)];
                const float2 a1 = c_add(x0, x2), c1 = c_mul(c_sub(x0, x2), wa);       // stage L
                const float2 b1 = c_add(x1, x3), d1 = c_mul(c_sub(x1, x3), wb);
                x[0] = c_add(a1, b1);                                                 // stage L/2
                x[q4] = c_mul(c_sub(a1, b1), wc);
                x[2 * q4] = c_add(c1, d1);
                x[3 * q4] = c_mul(c_sub(c1, d1), wc);
            }
            lg_l -= 2;
            chan_wave_sync();
        }
        if (lg_l == 1) {                                          // the last stage of an odd log2 F: L = 2, twiddle 1
            const int n_bfly2 = rows_w << (lg - 1);
            for (int j = lane; j < n_bfly2; j += kWave) {
                const int row = j >> (lg - 1);
                if (wb0 + (row & (CB - 1)) >= g.B) continue;
                float2 *x = xw + 2 * j;
                const float2 x0 = x[0], x1 = x[1];
                x[0] = c_add(x0, x1);
                x[1] = c_sub(x0, x1);
            }
        }
        __syncthreads();                                          // every wave's transforms are in the image

        // ---- accumulate by bin: this thread's position, the blocks grp, grp + G, ... of the round ----
        for (int blk = grp; blk < RB; blk += G) {
            if (r0 + blk >= g.B) break;
            const int w = blk >> lg_cb, cb = blk & (CB - 1);
            const float2 *xb = xs + (size_t)w * (rows_w << lg) + (cb << lg) + pos;
            float2 x[TN];
#pragma unroll
            for (int a = 0; a < TN; a++) x[a] = xb[(a << lg_cb) << lg];
#pragma unroll
            for (int a = 0; a < TN; a++) {
                acc.d[a] = fmaf(x[a].x, x[a].x, fmaf(x[a].y, x[a].y, acc.d[a]));
#pragma unroll
                for (int b = a + 1; b < TN; b++) {                // x_a conj(x_b)
                    const int idx = a * TN - (a * (a + 1)) / 2 + (b - a - 1);
                    acc.re[idx] = fmaf(x[a].x, x[b].x, fmaf(x[a].y, x[b].y, acc.re[idx]));
                    acc.im[idx] = fmaf(x[a].y, x[b].x, fmaf(-x[a].x, x[b].y, acc.im[idx]));
                }
            }
        }
        __syncthreads();                                          // the image is overwritten by the next round's load
    }

    // ---- the partial sums of every thread, plane k of 256 floats: k = a (diagonal), TN + 2 idx (re), TN + 2 idx + 1 (im) ----
    float *ps = reinterpret_cast<float *>(xs);
#pragma unroll
    for (int a = 0; a < TN; a++) ps[a * kChanThreads + tid] = acc.d[a];
#pragma unroll
    for (int i = 0; i < TN * (TN - 1) / 2; i++) {
        ps[(TN + 2 * i) * kChanThreads + tid] = acc.re[i];
        ps[(TN + 2 * i + 1) * kChanThreads + tid] = acc.im[i];
    }
    __syncthreads();

    // sum k of the bin at position p over its G threads in thread order, scaled once
    auto bin_sum = [&](int k, int p) {
        const float *q = ps + k * kChanThreads + p;
        float s = q[0];
        for (int gg = 1; gg < G; gg++) s = f_add(s, q[gg << lg]);
        return f_mul(s, g.inv);
    };
    auto position_of = [&](int f) { return (int)(__brev((unsigned)f) >> (32 - lg)); };

    constexpr int nn = TN * TN;
    float2 *item0 = g.out + (size_t)snap * (size_t)g.num_bins * nn;
    const int total = g.num_bins * nn;
    for (int idx = tid; idx < total; idx += kChanThreads) {
        const int j = idx / nn, e = idx - j * nn;
        const int row = e % TN, col = e / TN;                     // column-major: R[row, col] at row + col N
        const int p = position_of((g.first_bin + j) & (F - 1));
        float2 r;
        if (row == col) {
            r = make_float2(bin_sum(row, p), 0.f);
        } else {
            const int a = row < col ? row : col, b = row < col ? col : row;
            const int t = a * TN - (a * (a + 1)) / 2 + (b - a - 1);
            const float im = bin_sum(TN + 2 * t + 1, p);
            r = make_float2(bin_sum(TN + 2 * t, p), row < col ? im : -im);
        }
        item0[idx] = r;
    }
    if (g.power) {
        for (int f = tid; f < F; f += kChanThreads) {
            const int p = position_of(f);
            float pw = bin_sum(0, p);
#pragma unroll
            for (int a = 1; a < TN; a++) pw = f_add(pw, bin_sum(a, p));
            g.power[(size_t)snap * F + f] = pw;
        }
    }
}

template <class L, int TN, bool SMALL> static void launch_chan_size(bool vec2, const ChanCovArgs &g, int n, hipStream_t st)
{
    if (vec2) hipLaunchKernelGGL((channel_covariance_kernel<L, TN, true, SMALL>), dim3(n), dim3(kChanThreads), 0, st, g);
    else      hipLaunchKernelGGL((channel_covariance_kernel<L, TN, false, SMALL>), dim3(n), dim3(kChanThreads), 0, st, g);
}
template <class L, int TN> static void launch_chan_tn(bool vec2, const ChanCovArgs &g, int n, hipStream_t st)
{
    if (g.F <= 64) launch_chan_size<L, TN, true>(vec2, g, n, st);
    else           launch_chan_size<L, TN, false>(vec2, g, n, st);
}

template <class L> static void launch_chan(int N, bool vec2, const ChanCovArgs &g, int n, hipStream_t st)
{
    switch (N) {
    case 1: launch_chan_tn<L, 1>(vec2, g, n, st); break;
    case 2: launch_chan_tn<L, 2>(vec2, g, n, st); break;
    case 3: launch_chan_tn<L, 3>(vec2, g, n, st); break;
    case 4: launch_chan_tn<L, 4>(vec2, g, n, st); break;
    case 5: launch_chan_tn<L, 5>(vec2, g, n, st); break;
    case 6: launch_chan_tn<L, 6>(vec2, g, n, st); break;
    case 7: launch_chan_tn<L, 7>(vec2, g, n, st); break;
    default: launch_chan_tn<L, 8>(vec2, g, n, st); break;
    }
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct doa_channel_covariance : doa::BlockBase {
    int N = 0, lg_f = 0;
    doa::StreamWindow win;
    doa::BinSelection sel;                 // sel.F: the transform size
    float inv = 0.f;                       // (float)(1 / (B W2))
    doa::InputFormat fmt;
    doa::DevBuf d_table;                   // [F/2] float2 twiddles, then [F] float window
    doa::DevBuf d_in, d_out, d_power;      // the host entry's buffers
};

extern "C" {

doa_channel_covariance_t *doa_channel_covariance_create(int inputs, int snapshot_size, int overlap_size, int fft_len,
                                                        const float *window)
{
    doa::clear_error();
    if (inputs > doa::kChanMaxInputs && inputs <= DOA_MAX_ANT_ELE) {
        doa::set_error("channel_covariance: inputs=%d is not built into this library (1..%d are)", inputs, doa::kChanMaxInputs);
        return nullptr;
    }
    const int lg_f = doa::fft_len_log2(fft_len);
    if (inputs < 1 || inputs > DOA_MAX_ANT_ELE || lg_f < 0) {
        doa::set_error("channel_covariance: invalid argument: need 1 <= inputs <= %d and fft_len 16, 32, 64, 128 or 256 "
                       "(got %d, %d)", doa::kChanMaxInputs, inputs, fft_len);
        return nullptr;
    }
    if (snapshot_size <= 0 || snapshot_size % fft_len || overlap_size < 0 || overlap_size >= snapshot_size) {
        doa::set_error("channel_covariance: invalid argument: need snapshot_size a positive multiple of fft_len and "
                       "0 <= overlap_size < snapshot_size (got %d, %d, fft_len %d)", snapshot_size, overlap_size, fft_len);
        return nullptr;
    }
    float win[doa::kChanMaxFft];
    double w2 = 0.0;
    for (int t = 0; t < fft_len; t++) {
        win[t] = window ? window[t] : 1.0f;
        if (!std::isfinite(win[t])) {
            doa::set_error("channel_covariance: invalid argument: window[%d] is not finite", t);
            return nullptr;
        }
        w2 += (double)win[t] * (double)win[t];
    }
    if (!(w2 > 0.0) || !std::isfinite(w2)) {
        doa::set_error("channel_covariance: invalid argument: the window's sum of squares must be finite and > 0");
        return nullptr;
    }
    return doa::create_block<doa_channel_covariance>("channel_covariance", [&](doa_channel_covariance &h) -> int {
        h.N = inputs; h.win.K = snapshot_size; h.win.overlap = overlap_size; h.lg_f = lg_f;
        h.sel = {fft_len, 0, fft_len};
        h.inv = (float)(1.0 / ((double)(snapshot_size / fft_len) * w2));
        // twiddles and window: built here in double, rounded once, read by every launch of the handle
        float table[doa::kChanMaxFft * 2];
        const double pi = 3.14159265358979323846;
        for (int k = 0; k < fft_len / 2; k++) {
            table[2 * k] = (float)std::cos(2.0 * pi * k / fft_len);
            table[2 * k + 1] = (float)(-std::sin(2.0 * pi * k / fft_len));
        }
        memcpy(table + fft_len, win, sizeof(float) * fft_len);
        if (int rc = h.d_table.reserve(sizeof(float) * 2 * fft_len); rc != DOA_OK) return rc;
        DOA_HIP_TRY(hipMemcpy(h.d_table.p, table, sizeof(float) * 2 * fft_len, hipMemcpyHostToDevice));
        return (int)DOA_OK;
    });
}

void doa_channel_covariance_destroy(doa_channel_covariance_t *h) { doa::destroy_block(h); }

int doa_channel_covariance_history(const doa_channel_covariance_t *h) { return h ? h->win.history() : DOA_ERR_INVALID_ARG; }

int doa_channel_covariance_forecast(const doa_channel_covariance_t *h, int noutput_items)
{
    return h && noutput_items >= 0 ? h->win.forecast(noutput_items) : DOA_ERR_INVALID_ARG;
}

long long doa_channel_covariance_input_span(const doa_channel_covariance_t *h, int noutput_items)
{
    return h ? h->win.input_span(noutput_items) : 0;
}

int doa_channel_covariance_set_input_format(doa_channel_covariance_t *h, int format, float scale)
{
    doa::clear_error();
    return doa::set_input_format("channel_covariance", h ? &h->fmt : nullptr, format, scale);
}

int doa_channel_covariance_set_bins(doa_channel_covariance_t *h, int first_bin, int num_bins)
{
    doa::clear_error();
    if (!h) { doa::set_error("channel_covariance_set_bins: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (int rc = doa::check_bin_selection("channel_covariance_set_bins", h->sel.F, first_bin, num_bins); rc != DOA_OK) return rc;
    h->sel.first = first_bin; h->sel.nb = num_bins;
    return DOA_OK;
}

int doa_channel_covariance_num_bins(const doa_channel_covariance_t *h) { return h ? h->sel.nb : DOA_ERR_INVALID_ARG; }

int doa_channel_covariance_work_dev(doa_channel_covariance_t *h, int noutput_items, const void *const *d_input_items,
                                    void *d_out_cov, void *d_out_power, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("channel_covariance_work_dev", h, noutput_items, {d_input_items, d_out_cov}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    bool pair_aligned = true;
    if (int rc = doa::check_streams("channel_covariance_work_dev", d_input_items, h->N, h->fmt.sample_bytes(), &pair_aligned); rc != DOA_OK) return rc;
    doa::ChanCovArgs g;
    memset(&g, 0, sizeof g);
    for (int k = 0; k < doa::kChanMaxInputs; k++) g.in[k] = d_input_items[k < h->N ? k : 0];
    g.out = static_cast<float2 *>(d_out_cov);
    g.power = static_cast<float *>(d_out_power);
    g.twiddle = h->d_table.as<float2>();
    g.window = h->d_table.as<float>() + h->sel.F;
    g.K = h->win.K; g.S = h->win.step(); g.F = h->sel.F; g.lg_f = h->lg_f; g.B = h->win.K / h->sel.F;
    g.first_bin = h->sel.first; g.num_bins = h->sel.nb;
    g.inv = h->inv;
    g.scale = h->fmt.kernel_scale();
    // pair loads: every block of every snapshot starts on a sample pair (F is even, so only the snapshot step matters)
    const bool vec2 = pair_aligned && (g.S % 2 == 0);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (h->fmt.format == DOA_SAMPLE_SC16) doa::launch_chan<doa::Sc16Samples>(h->N, vec2, g, noutput_items, st);
    else                              doa::launch_chan<doa::Fc32Samples>(h->N, vec2, g, noutput_items, st);
    DOA_HIP_TRY(hipGetLastError());
    return noutput_items;
}

int doa_channel_covariance_work(doa_channel_covariance_t *h, int noutput_items, const void *const *input_items, void *out_cov,
                                float *out_power)
{
    doa::clear_error();
    if (int rc = doa::work_args("channel_covariance_work", h, noutput_items, {input_items, out_cov}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    const int N = h->N;
    const size_t sb = h->fmt.sample_bytes();
    doa::HostCall io(*h);
    const void *d_ptrs[doa::kChanMaxInputs];
    // the device copy of a stream keeps the caller's offset inside 16 bytes, so the load route follows the caller's alignment
    io.in_streams("channel_covariance_work", h->d_in, input_items, N, (size_t)h->win.input_span(noutput_items) * sb, d_ptrs, 0, sb);
    io.out(h->d_out, out_cov, (size_t)noutput_items * h->sel.nb * N * N * sizeof(float2));
    if (out_power) io.out(h->d_power, out_power, (size_t)noutput_items * h->sel.F * sizeof(float));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = doa_channel_covariance_work_dev(h, noutput_items, d_ptrs, h->d_out.p, out_power ? h->d_power.p : nullptr, h->stream);
    return io.finish(rc);
}

}  // extern "C"
