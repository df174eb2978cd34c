// autocorrelate.hip — K1: sliding-window sample covariance of N complex streams on gfx950.
//
// Replaces gr::doa::autocorrelate (reference lib/autocorrelate_impl.cc:47-118):
//   R_i[a,b] = (1/K) * sum_{t<K} x_a[i*S + t] * conj(x_b[i*S + t]),   S = K - overlap,
//   optional forward-backward step R <- 0.5 R + (0.5/K) J conj(R) J   (:107-108, the second
//   term is divided by K a second time in the reference; reproduced).
// Output items are column-major N x N complex64 (:103).
//
// Kernel shape (HBM-bound, ~1 flop/B): one 64-lane wave owns one snapshot.  Each lane streams
// 16-byte (two-sample) loads from every channel — a wave instruction covers 1 KiB contiguous per
// channel — and keeps the Hermitian upper triangle (N real + N(N-1)/2 complex partial sums) in
// registers; partials meet in one DPP wave all-reduce and lanes 0..N^2-1 write the 8N^2-byte item
// as one contiguous segment.  No LDS, no atomics.  Overlapping windows take a read-once two-kernel
// path (cov_piece_kernel + cov_combine_kernel); 8 < N <= 16 runs on the matrix cores (cov_mfma_kernel).
// Every streaming kernel is templated on a sample loader (Fc32Samples / Sc16Samples): the sc16 form reads complex
// int16 and widens in registers, with the same lanes, accumulators and summation order as the fc32 form.
#include "block_host.hpp"
#include "kernels.hpp"
#include "launch_routes.hpp"
#include "sample_loaders.hpp"
#include "wave_ops.hpp"

#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace doa {

struct CovArgs {
    const void *in[DOA_MAX_ANT_ELE];   // N streams of the loader's sample type
    float2 *out;
    int n_ch;      // N
    int K;         // snapshot_size
    int S;         // snapshot_size - overlap_size
    int n_out;     // windows to produce
    int avg;       // 1 = forward-backward
    float inv_k;   // (float)(1.0/K)
    float fb_hk;   // (float)(0.5/K)
    const float2 *gain;   // optional [N*N] g_a conj(g_b) (fused antenna_correction), or nullptr
    // read-once path for overlapping windows (cov_piece_kernel + cov_combine_kernel)
    float2 *pieces;       // [n_steps][2][N*N] raw sums of the pieces A_j, B_j
    int q, r;             // K = q*S + r
    int n_steps;          // n_out + q
    float scale;          // sc16: the widening factor (Sc16Samples); unused for fc32
};

// The sample loaders (Fc32Samples / Sc16Samples) are in sample_loaders.hpp, shared with phase_offset_est.hip.
template <class L> __device__ __forceinline__ const typename L::sample_t *stream(const CovArgs &g, int k)
{
    return static_cast<const typename L::sample_t *>(g.in[k]);
}

// Multi-batch form (kernels.hpp, BatchGroup; N <= 4): snapshot g = batch * n + local reads its batch's own streams and
// writes its batch's own items.  n_out is the group's total.
struct CovGroupArgs : CovArgs {
    const void *gin[kMaxGroup][4];
    float2 *gout[kMaxGroup];
    GroupSplit split;
};

// where one snapshot's samples come from and where its item goes
template <class L, int TN> struct SnapIO {
    const typename L::sample_t *in[TN];
    size_t base;        // first sample of the window in every stream
    float2 *out;        // the item
};
template <class L, int TN> __device__ __forceinline__ SnapIO<L, TN> snap_io(const CovArgs &g, int snap)
{
    SnapIO<L, TN> io;
#pragma unroll
    for (int a = 0; a < TN; a++) io.in[a] = stream<L>(g, a);
    io.base = (size_t)snap * (size_t)g.S;
    io.out = g.out + (size_t)snap * (TN * TN);
    return io;
}
template <class L, int TN> __device__ __forceinline__ SnapIO<L, TN> snap_io(const CovGroupArgs &g, int snap)
{
    static_assert(TN <= 4, "the group table holds four streams per batch");
    unsigned batch, local;
    g.split((unsigned)__builtin_amdgcn_readfirstlane(snap), batch, local);      // wave-uniform: the table is read with scalar loads
    SnapIO<L, TN> io;
#pragma unroll
    for (int a = 0; a < TN; a++) io.in[a] = static_cast<const typename L::sample_t *>(g.gin[batch][a]);
    io.base = (size_t)local * (size_t)g.S;
    io.out = g.gout[batch] + (size_t)local * (TN * TN);
    return io;
}

template <int TN> struct TriAcc {
    float d[TN];
    float re[TN * (TN - 1) / 2 > 0 ? TN * (TN - 1) / 2 : 1];
    float im[TN * (TN - 1) / 2 > 0 ? TN * (TN - 1) / 2 : 1];
};

template <int TN> __device__ __forceinline__ void tri_accumulate(TriAcc<TN> &acc, const float2 (&x)[TN])
{
    int idx = 0;
#pragma unroll
    for (int a = 0; a < TN; a++) {
        acc.d[a] = fmaf(x[a].x, x[a].x, fmaf(x[a].y, x[a].y, acc.d[a]));
#pragma unroll
        for (int b = a + 1; b < TN; b++) {
            // x_a * conj(x_b)
            acc.re[idx] = fmaf(x[a].x, x[b].x, fmaf(x[a].y, x[b].y, acc.re[idx]));
            acc.im[idx] = fmaf(x[a].y, x[b].x, fmaf(-x[a].x, x[b].y, acc.im[idx]));
            idx++;
        }
    }
}

// One wave per snapshot, N = TN <= 8, Hermitian symmetry exploited.
// VEC2: all streams aligned to two samples at every window start (base 16-B aligned for fc32, 8-B for sc16; S even) ->
// one load per sample pair.
// A = CovArgs (one batch) or CovGroupArgs (a group of batches): only snap_io differs.
template <class L, int TN, bool VEC2, int UN, bool NT = false, class A = CovArgs>
__global__ __launch_bounds__(256) void cov_wave_kernel(A g)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave0 = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const int n_waves = gridDim.x * (blockDim.x / kWave);
    // grid-stride over snapshots: the launch may use fewer waves than snapshots so that other kernels
    // (the EVD / scan of the previous batch on another stream) find free wave slots on every CU
    for (int snap = wave0; snap < g.n_out; snap += n_waves) {
    const SnapIO<L, TN> io = snap_io<L, TN>(g, snap);
    const size_t base = io.base;

    TriAcc<TN> acc;
#pragma unroll
    for (int a = 0; a < TN; a++) acc.d[a] = 0.f;
#pragma unroll
    for (int i = 0; i < TN * (TN - 1) / 2; i++) { acc.re[i] = 0.f; acc.im[i] = 0.f; }

    if constexpr (VEC2) {
        const int npair = g.K >> 1;
        // UN wave-iterations (UN*128 samples) per trip: all UN*TN 16-byte loads are issued before the
        // first one is consumed, so each wave keeps UN*TN KiB in flight (HBM latency x bandwidth needs
        // ~50 KiB per CU; 16 waves x 16 KiB gives 5x that while staying under 96 VGPRs).
        int p = lane;
        for (; p + (UN - 1) * kWave < npair; p += UN * kWave) {
            float4 v[UN][TN];
#pragma unroll
            for (int u = 0; u < UN; u++)
#pragma unroll
                for (int a = 0; a < TN; a++)
                    v[u][a] = L::template pair<NT>(io.in[a] + base + 2 * (size_t)(p + u * kWave), g.scale);
#pragma unroll
            for (int u = 0; u < UN; u++) {
                float2 x0[TN], x1[TN];
#pragma unroll
                for (int a = 0; a < TN; a++) { x0[a] = make_float2(v[u][a].x, v[u][a].y); x1[a] = make_float2(v[u][a].z, v[u][a].w); }
                tri_accumulate<TN>(acc, x0);
                tri_accumulate<TN>(acc, x1);
            }
        }
        for (; p < npair; p += kWave) {
            float4 v[TN];
#pragma unroll
            for (int a = 0; a < TN; a++) v[a] = L::template pair<NT>(io.in[a] + base + 2 * (size_t)p, g.scale);
            float2 x0[TN], x1[TN];
#pragma unroll
            for (int a = 0; a < TN; a++) { x0[a] = make_float2(v[a].x, v[a].y); x1[a] = make_float2(v[a].z, v[a].w); }
            tri_accumulate<TN>(acc, x0);
            tri_accumulate<TN>(acc, x1);
        }
        if ((g.K & 1) && lane == 0) {
            float2 x[TN];
#pragma unroll
            for (int a = 0; a < TN; a++) x[a] = L::one(io.in[a] + (base + (size_t)(g.K - 1)), g.scale);
            tri_accumulate<TN>(acc, x);
        }
    } else {
#pragma unroll 4
        for (int t = lane; t < g.K; t += kWave) {
            float2 x[TN];
#pragma unroll
            for (int a = 0; a < TN; a++) x[a] = L::one(io.in[a] + (base + (size_t)t), g.scale);
            tri_accumulate<TN>(acc, x);
        }
    }

    // wave all-reduce of the N^2 real partial sums
#pragma unroll
    for (int a = 0; a < TN; a++) acc.d[a] = wave_allreduce_sum(acc.d[a]);
#pragma unroll
    for (int i = 0; i < TN * (TN - 1) / 2; i++) {
        acc.re[i] = wave_allreduce_sum(acc.re[i]);
        acc.im[i] = wave_allreduce_sum(acc.im[i]);
    }

    // lane e = a + b*N picks element R[a,b]
    float2 r = make_float2(0.f, 0.f);
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < TN; a++) {
            if (lane == a + a * TN) r = make_float2(acc.d[a], 0.f);
#pragma unroll
            for (int b = a + 1; b < TN; b++) {
                if (lane == a + b * TN) r = make_float2(acc.re[idx], acc.im[idx]);
                if (lane == b + a * TN) r = make_float2(acc.re[idx], -acc.im[idx]);
                idx++;
            }
        }
    }
    r.x = __fmul_rn(r.x, g.inv_k);
    r.y = __fmul_rn(r.y, g.inv_k);
    if (g.gain && lane < TN * TN) {            // fused antenna correction: R[a,b] *= g_a conj(g_b)
        const float2 w = g.gain[lane];
        r = make_float2(fmaf(w.x, r.x, -w.y * r.y), fmaf(w.x, r.y, w.y * r.x));
    }
    if (g.avg == 1) {
        // (J conj(R) J)[a,b] = conj(R[N-1-a, N-1-b])  ->  element index N^2-1-e
        const int src = (lane < TN * TN) ? (TN * TN - 1 - lane) : lane;
        const float px = __shfl(r.x, src, kWave);
        const float py = __shfl(r.y, src, kWave);
        r.x = __fadd_rn(__fmul_rn(0.5f, r.x), __fmul_rn(g.fb_hk, px));
        r.y = __fadd_rn(__fmul_rn(0.5f, r.y), __fmul_rn(g.fb_hk, -py));
    }
    if (lane < TN * TN) io.out[lane] = r;
    }  // snapshot loop
}

// ---------------------------------------------------------------------------------------------
// Overlapping windows, read-once.  With S = K - overlap and K = q S + r, cut every stream at j S and
// j S + r: step j owns piece A_j = [j S, j S + r) and piece B_j = [j S + r, (j+1) S), and
//     window i  =  sum_{j=i}^{i+q-1} (A_j + B_j)  +  A_{i+q}.
// cov_piece_kernel: one wave per step streams its S new samples ONCE (same loads, accumulators and DPP
// reduction as cov_wave_kernel) and writes the two raw N x N piece sums (2 x 8N^2 B per step);
// cov_combine_kernel adds the q+... pieces of each window and applies 1/K, the fused antenna
// correction and the forward-backward step.  HBM traffic = the new samples only (the single-kernel
// path re-fetches the overlap of almost every window: measured 253 MB against 201 MB algorithmic at
// K = 2048, overlap = 512), and the overlap's multiply-adds are not repeated either.  The price is
// one more (tiny) launch, so windows without overlap stay on cov_wave_kernel.
// ---------------------------------------------------------------------------------------------
template <class L, int TN, int UN, bool NT>
__device__ __forceinline__ void accumulate_pairs(TriAcc<TN> &acc, const CovArgs &g, size_t first, int npair, int lane)
{
    int p = lane;
    for (; p + (UN - 1) * kWave < npair; p += UN * kWave) {
        float4 v[UN][TN];
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int a = 0; a < TN; a++)
                v[u][a] = L::template pair<NT>(stream<L>(g, a) + first + 2 * (size_t)(p + u * kWave), g.scale);
#pragma unroll
        for (int u = 0; u < UN; u++) {
            float2 x0[TN], x1[TN];
#pragma unroll
            for (int a = 0; a < TN; a++) { x0[a] = make_float2(v[u][a].x, v[u][a].y); x1[a] = make_float2(v[u][a].z, v[u][a].w); }
            tri_accumulate<TN>(acc, x0);
            tri_accumulate<TN>(acc, x1);
        }
    }
    for (; p < npair; p += kWave) {
        float4 v[TN];
#pragma unroll
        for (int a = 0; a < TN; a++) v[a] = L::template pair<NT>(stream<L>(g, a) + first + 2 * (size_t)p, g.scale);
        float2 x0[TN], x1[TN];
#pragma unroll
        for (int a = 0; a < TN; a++) { x0[a] = make_float2(v[a].x, v[a].y); x1[a] = make_float2(v[a].z, v[a].w); }
        tri_accumulate<TN>(acc, x0);
        tri_accumulate<TN>(acc, x1);
    }
}

template <int TN> __device__ __forceinline__ void tri_clear(TriAcc<TN> &acc)
{
#pragma unroll
    for (int a = 0; a < TN; a++) acc.d[a] = 0.f;
#pragma unroll
    for (int i = 0; i < TN * (TN - 1) / 2; i++) { acc.re[i] = 0.f; acc.im[i] = 0.f; }
}

// wave all-reduce, then lane e = a + b*N holds the raw sum of x_a conj(x_b)
template <int TN> __device__ __forceinline__ float2 tri_reduce_to_lane(TriAcc<TN> &acc, int lane)
{
#pragma unroll
    for (int a = 0; a < TN; a++) acc.d[a] = wave_allreduce_sum(acc.d[a]);
#pragma unroll
    for (int i = 0; i < TN * (TN - 1) / 2; i++) {
        acc.re[i] = wave_allreduce_sum(acc.re[i]);
        acc.im[i] = wave_allreduce_sum(acc.im[i]);
    }
    float2 r = make_float2(0.f, 0.f);
    int idx = 0;
#pragma unroll
    for (int a = 0; a < TN; a++) {
        if (lane == a + a * TN) r = make_float2(acc.d[a], 0.f);
#pragma unroll
        for (int b = a + 1; b < TN; b++) {
            if (lane == a + b * TN) r = make_float2(acc.re[idx], acc.im[idx]);
            if (lane == b + a * TN) r = make_float2(acc.re[idx], -acc.im[idx]);
            idx++;
        }
    }
    return r;
}

// requires: S and r even, every stream base aligned to two samples (one pair load at every piece start)
template <class L, int TN, int UN, bool NT>
__global__ __launch_bounds__(256) void cov_piece_kernel(CovArgs g)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave0 = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const int n_waves = gridDim.x * (blockDim.x / kWave);
    for (int step = wave0; step < g.n_steps; step += n_waves) {
        const size_t base = (size_t)step * (size_t)g.S;
        float2 *po = g.pieces + (size_t)step * (2 * TN * TN);
        TriAcc<TN> acc;
        if (g.r > 0) {                                     // piece A_j
            tri_clear<TN>(acc);
            accumulate_pairs<L, TN, UN, NT>(acc, g, base, g.r >> 1, lane);
            const float2 v = tri_reduce_to_lane<TN>(acc, lane);
            if (lane < TN * TN) po[lane] = v;
        }
        if (step + 1 < g.n_steps) {                        // piece B_j (the last step only contributes its A)
            tri_clear<TN>(acc);
            accumulate_pairs<L, TN, UN, NT>(acc, g, base + (size_t)g.r, (g.S - g.r) >> 1, lane);
            const float2 v = tri_reduce_to_lane<TN>(acc, lane);
            if (lane < TN * TN) po[TN * TN + lane] = v;
        }
    }
}

__global__ __launch_bounds__(256) void cov_combine_kernel(CovArgs g)
{
    const int nn = g.n_ch * g.n_ch;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)g.n_out * nn) return;
    const int i = (int)(idx / nn), e = (int)(idx % nn);
    auto window_sum = [&](int el) {
        float sx = 0.f, sy = 0.f;
        for (int j = i; j < i + g.q; j++) {
            const float2 *pj = g.pieces + (size_t)j * (2 * nn);
            if (g.r > 0) { const float2 a = pj[el]; sx = __fadd_rn(sx, a.x); sy = __fadd_rn(sy, a.y); }
            const float2 b = pj[nn + el];
            sx = __fadd_rn(sx, b.x); sy = __fadd_rn(sy, b.y);
        }
        if (g.r > 0) { const float2 a = g.pieces[(size_t)(i + g.q) * (2 * nn) + el]; sx = __fadd_rn(sx, a.x); sy = __fadd_rn(sy, a.y); }
        float2 r = make_float2(__fmul_rn(sx, g.inv_k), __fmul_rn(sy, g.inv_k));
        if (g.gain) {                                      // fused antenna correction: R[a,b] *= g_a conj(g_b)
            const float2 w = g.gain[el];
            r = make_float2(fmaf(w.x, r.x, -w.y * r.y), fmaf(w.x, r.y, w.y * r.x));
        }
        return r;
    };
    float2 r = window_sum(e);
    if (g.avg == 1) {                                      // (J conj(R) J)[a,b] = conj(R[N-1-a, N-1-b]) = element N^2-1-e
        const float2 m = window_sum(nn - 1 - e);
        r.x = __fadd_rn(__fmul_rn(0.5f, r.x), __fmul_rn(g.fb_hk, m.x));
        r.y = __fadd_rn(__fmul_rn(0.5f, r.y), __fmul_rn(g.fb_hk, -m.y));
    }
    g.out[idx] = r;
}

// Wide arrays (8 < N <= 16): the per-snapshot outer-product sum is a 16 x K by K x 16 complex GEMM,
// run on the matrix cores as four real v_mfma_f32_16x16x4_f32 per 4-sample step (exact fp32, same
// rate as the vector FMA pipe but with the whole 16 x 16 accumulator held in 8 registers):
//     Re R += Xr Xr^T + Xi Xi^T,      Im R += Xi Xr^T - Xr Xi^T.
// One wave owns one snapshot.  Lane l = (channel l&15, sample group l>>4) loads 4 consecutive samples
// (two 16-byte loads; 128 B contiguous per channel per wave-iteration) and feeds the SAME register as
// the A and the B operand (A[a][k] = x_a[t_k], B[k][b] = x_b[t_k]); channels >= N contribute zeros.
// No cross-lane reduction is needed: the K dimension is summed inside the MFMA accumulators, whose
// C/D layout (row = 4*(l>>4)+reg, col = l&15) is written straight to the column-major item.
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// UN wave-iterations (16 UN samples per lane group) of loads in flight.
template <class L, bool VEC2, int UN> __global__ __launch_bounds__(256) void cov_mfma_kernel(CovArgs g)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave0 = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const int n_waves = gridDim.x * (blockDim.x / kWave);
    const int ch = lane & 15, grp = lane >> 4;
    const bool live = ch < g.n_ch;
    const typename L::sample_t *src = stream<L>(g, live ? ch : 0);
    for (int snap = wave0; snap < g.n_out; snap += n_waves) {
        // VEC2: per 16-sample block this lane takes samples {2 grp, 2 grp + 1, 8 + 2 grp, 9 + 2 grp}: each 16-byte
        // load instruction then covers 64 contiguous bytes per channel (two full 32-byte sectors) instead of four
        // half-used ones; which four samples meet in one MFMA step does not matter for the sum (sc16: two 8-byte loads)
        const typename L::sample_t *p = src + (size_t)snap * (size_t)g.S + (VEC2 ? 2 : 4) * grp;
        f32x4_t acc_re = {0.f, 0.f, 0.f, 0.f}, acc_im = {0.f, 0.f, 0.f, 0.f};
        auto step = [&](float xr, float xi) {
            acc_re = __builtin_amdgcn_mfma_f32_16x16x4f32(xr, xr, acc_re, 0, 0, 0);
            acc_im = __builtin_amdgcn_mfma_f32_16x16x4f32(xi, xr, acc_im, 0, 0, 0);
            acc_re = __builtin_amdgcn_mfma_f32_16x16x4f32(xi, xi, acc_re, 0, 0, 0);
            acc_im = __builtin_amdgcn_mfma_f32_16x16x4f32(-xr, xi, acc_im, 0, 0, 0);
        };
        int t = 0;
        for (; t + 16 * UN <= g.K; t += 16 * UN) {
            float2 x[UN][4];
#pragma unroll
            for (int u = 0; u < UN; u++) {
                if constexpr (VEC2) {
                    // default cache policy on purpose: the two loads of a block share 128-byte lines and
                    // want to meet in L1 (non-temporal: 169 vs 120 us)
                    const float4 v0 = L::template pair<false>(p + t + 16 * u, g.scale);
                    const float4 v1 = L::template pair<false>(p + t + 16 * u + 8, g.scale);
                    x[u][0] = make_float2(v0.x, v0.y); x[u][1] = make_float2(v0.z, v0.w);
                    x[u][2] = make_float2(v1.x, v1.y); x[u][3] = make_float2(v1.z, v1.w);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) x[u][j] = L::one(p + t + 16 * u + j, g.scale);
                }
            }
#pragma unroll
            for (int u = 0; u < UN; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) step(live ? x[u][j].x : 0.f, live ? x[u][j].y : 0.f);
        }
        for (; t < g.K; t += 16) {                      // remainder, sample by sample with bounds checks
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int sidx = t + 4 * grp + j;
                float2 v = make_float2(0.f, 0.f);
                if (live && sidx < g.K) v = L::one(src + ((size_t)snap * (size_t)g.S + sidx), g.scale);
                step(v.x, v.y);
            }
        }
        float2 *item = g.out + (size_t)snap * g.n_ch * g.n_ch;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int a = 4 * grp + r;
            if (a < g.n_ch && live) {
                float2 v = make_float2(__fmul_rn(acc_re[r], g.inv_k), __fmul_rn(acc_im[r], g.inv_k));
                if (g.gain) {
                    const float2 w = g.gain[a + ch * g.n_ch];
                    v = make_float2(fmaf(w.x, v.x, -w.y * v.y), fmaf(w.x, v.y, w.y * v.x));
                }
                item[a + (size_t)ch * g.n_ch] = v;
            }
        }
    }
}

// R <- 0.5 R + (0.5/K) conj(R[N-1-a, N-1-b]), pairwise in place (element e with N^2-1-e).
__global__ void cov_fb_kernel(float2 *out, int nn, long long n_items, float fb_hk)
{
    const int half = (nn + 1) / 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_items * half) return;
    const long long item = gid / half;
    const int e = (int)(gid - item * half), e2 = nn - 1 - e;
    float2 *p = out + item * nn;
    const float2 u = p[e], v = p[e2];
    float2 nu, nv;
    nu.x = __fadd_rn(__fmul_rn(0.5f, u.x), __fmul_rn(fb_hk, v.x));
    nu.y = __fadd_rn(__fmul_rn(0.5f, u.y), __fmul_rn(fb_hk, -v.y));
    nv.x = __fadd_rn(__fmul_rn(0.5f, v.x), __fmul_rn(fb_hk, u.x));
    nv.y = __fadd_rn(__fmul_rn(0.5f, v.y), __fmul_rn(fb_hk, -u.y));
    p[e] = nu;
    if (e2 != e) p[e2] = nv;
}

// The launches of a route (launch_routes.hpp: cov_route).  A = CovArgs (one batch) or CovGroupArgs (a group of batches).
// Measurements behind the route's numbers:
//  * waves per CU: at N = 4, 16 (= one wave per snapshot at the benchmark batch: 4096 snapshots on 256 CUs) measured against 8
//    with the round-1 kernels: -0.6 us on the kernel alone (23.2 vs 23.8 us) and -1.2 us per 4-stream pipeline step (25.6 vs
//    27.1); wider arrays hold 2-4x the registers per wave and measured better with 8 (N = 6: 54.4 vs 57.3 us, 4-stream step
//    56.8 vs 63.0 us);
//  * UN*TN 16-byte loads in flight per wave (UN = 1, 2, 8 measured within 3 % of UN = 4 at N = 4; N = 6: 44 us with UN = 4
//    against 55 with 2; N = 7: 68 us with 2 against 74 with 1); sc16: UN 8-byte loads, see Sc16Samples;
//  * the pair loads are a read-once stream: non-temporal loads (+19 % on MI355X against the default cache policy);
//  * a group is ONE WAVE PER SNAPSHOT, no cap: the single-batch cap (16 waves per CU, which at the benchmark batch is one wave
//    per snapshot anyway) would turn a group into 4096 waves that stay for the whole launch, and the EVD / scan workgroups of
//    the neighbouring lane would find no free wave slots until it ends; with one wave per snapshot workgroups retire all the
//    time.  (Lab builds: DOA_COV_GROUP_WAVES_PER_CU > 0 restores a cap; profiles/grouped_batches.txt.)
template <class L, int TN, class A> static void launch_cov_tn(const CovRoute &rt, const A &g, hipStream_t st)
{
    const dim3 grid(rt.main.grid), block(rt.main.block);
    constexpr int UN = cov_unroll(TN);
    if constexpr (std::is_same<A, CovArgs>::value) {
        if (rt.kernel == CovKernel::Pieces) {               // the read-once two-kernel path (see cov_piece_kernel)
            hipLaunchKernelGGL((cov_piece_kernel<L, TN, UN, true>), grid, block, 0, st, g);
            hipLaunchKernelGGL(cov_combine_kernel, dim3(rt.second.grid), dim3(rt.second.block), 0, st, g);
            return;
        }
    }
    if (!rt.vec2) hipLaunchKernelGGL((cov_wave_kernel<L, TN, false, 1, false, A>), grid, block, 0, st, g);
    else          hipLaunchKernelGGL((cov_wave_kernel<L, TN, true, UN, true, A>), grid, block, 0, st, g);
}

template <class L> static void launch_cov(const CovRoute &rt, const CovArgs &g, hipStream_t st)
{
    switch (rt.kernel == CovKernel::Mfma ? 0 : rt.TN) {
    case 1: launch_cov_tn<L, 1>(rt, g, st); break;
    case 2: launch_cov_tn<L, 2>(rt, g, st); break;
    case 3: launch_cov_tn<L, 3>(rt, g, st); break;
    case 4: launch_cov_tn<L, 4>(rt, g, st); break;
    case 5: launch_cov_tn<L, 5>(rt, g, st); break;
    case 6: launch_cov_tn<L, 6>(rt, g, st); break;
    case 7: launch_cov_tn<L, 7>(rt, g, st); break;
    case 8: launch_cov_tn<L, 8>(rt, g, st); break;
    default: {
        const dim3 grid(rt.main.grid), block(rt.main.block);
        if (rt.vec2) hipLaunchKernelGGL((cov_mfma_kernel<L, true, 4>), grid, block, 0, st, g);
        else         hipLaunchKernelGGL((cov_mfma_kernel<L, false, 4>), grid, block, 0, st, g);
        if (rt.second.grid)
            hipLaunchKernelGGL(cov_fb_kernel, dim3(rt.second.grid), dim3(rt.second.block), 0, st, g.out, g.n_ch * g.n_ch,
                               (long long)g.n_out, g.fb_hk);
    }
    }
}
template <class L> static void launch_cov(const CovRoute &rt, const CovGroupArgs &g, hipStream_t st)
{
    switch (rt.TN) {
    case 2: launch_cov_tn<L, 2>(rt, g, st); break;
    case 3: launch_cov_tn<L, 3>(rt, g, st); break;
    default: launch_cov_tn<L, 4>(rt, g, st); break;
    }
}

static CovKnobs cov_knobs()
{
    return {DOA_LAB_ENV_INT("DOA_COV_WAVES_PER_CU", -1), DOA_LAB_ENV_INT("DOA_COV_MFMA_WAVES_PER_CU", 16),
            DOA_LAB_ENV_INT("DOA_COV_GROUP_WAVES_PER_CU", 0)};
}

static void fill_cov_args(CovArgs &g, int N, int K, int S, int avg, int n_out, const void *d_gain_outer, int format, float scale)
{
    g.n_ch = N; g.K = K; g.S = S; g.n_out = n_out; g.avg = avg;
    g.inv_k = (float)(1.0 / K);
    g.fb_hk = (float)(0.5 / K);
    g.gain = static_cast<const float2 *>(d_gain_outer);
    g.scale = (format == DOA_SAMPLE_SC16) ? scale : 1.0f;
}

// Launches K1 on `st`.  d_in: N device pointers.  Returns DOA_OK / error.
// The route rule is the same in both formats: every stream aligned to one sample is required, every stream aligned to two
// samples with S even takes the pair loads (and, with overlap and a workspace, the read-once path)
int launch_autocorrelate(int N, int K, int ovl, int avg, int n_out, const void *const *d_in, void *d_out,
                         hipStream_t st, const void *d_gain_outer, void *d_workspace, int format, float scale)
{
    if (n_out <= 0) return DOA_OK;
    CovArgs g;
    memset(&g, 0, sizeof g);
    CovShape shape;
    shape.N = N; shape.K = K; shape.ovl = ovl; shape.avg = avg; shape.n_out = n_out; shape.format = format;
    shape.workspace = (d_workspace != nullptr);
    if (int rc = check_streams("autocorrelate", d_in, N, sample_bytes(format), &shape.pair_aligned); rc != DOA_OK) return rc;
    const CovRoute rt = cov_route(shape, cu_count(), cov_knobs());
    for (int k = 0; k < DOA_MAX_ANT_ELE; k++) g.in[k] = d_in[k < N ? k : 0];
    g.out = static_cast<float2 *>(d_out);
    fill_cov_args(g, N, K, K - ovl, avg, n_out, d_gain_outer, format, scale);
    if (rt.kernel == CovKernel::Pieces) {
        g.pieces = static_cast<float2 *>(d_workspace);
        g.q = rt.q; g.r = rt.r; g.n_steps = rt.n_steps;
    }
    if (format == DOA_SAMPLE_SC16) launch_cov<Sc16Samples>(rt, g, st);
    else                           launch_cov<Fc32Samples>(rt, g, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

bool autocorrelate_pair_loads(int N, int K, int ovl, const void *const *d_in, int format)
{
    bool pair_aligned = true;           // (not check_streams: this only asks, a bad stream is the launch's to refuse)
    for (int k = 0; k < N; k++) pair_aligned = pair_aligned && reinterpret_cast<uintptr_t>(d_in[k]) % (2 * sample_bytes(format)) == 0;
    return cov_pair_loads(K, ovl, pair_aligned);
}

int launch_autocorrelate_group(int N, int K, int avg, const BatchGroup &grp, hipStream_t st, const void *d_gain_outer,
                               int format, float scale)
{
    if (grp.n_batches <= 0 || grp.n <= 0) return DOA_OK;
    CovShape shape;
    shape.N = N; shape.K = K; shape.avg = avg; shape.n_out = grp.n_batches * grp.n; shape.format = format; shape.group = true;
    // (whether the route takes a group does not depend on the streams: refuse before reading them)
    if (grp.n_batches > kMaxGroup || cov_route(shape, cu_count(), cov_knobs()).status != DOA_OK) {
        set_error("autocorrelate: not a group shape (N=%d, %d batches)", N, grp.n_batches);
        return DOA_ERR_INVALID_ARG;
    }
    // a group must be uniform in the load route, because the two routes sum in different orders
    for (int b = 0; b < grp.n_batches; b++) {
        bool pair_aligned;
        if (int rc = check_streams("autocorrelate", grp.in[b], N, sample_bytes(format), &pair_aligned, b); rc != DOA_OK) return rc;
        if (b == 0) shape.pair_aligned = pair_aligned;
        else if (cov_pair_loads(K, 0, pair_aligned) != cov_pair_loads(K, 0, shape.pair_aligned)) {
            set_error("autocorrelate: a group mixes the two load routes");
            return DOA_ERR_INVALID_ARG;
        }
    }
    const CovRoute rt = cov_route(shape, cu_count(), cov_knobs());
    CovGroupArgs g;
    memset(static_cast<void *>(&g), 0, sizeof g);
    for (int b = 0; b < kMaxGroup; b++) {
        const int src = b < grp.n_batches ? b : 0;          // unused entries repeat batch 0: never a wild pointer
        for (int k = 0; k < 4; k++) g.gin[b][k] = grp.in[src][k < N ? k : 0];
        g.gout[b] = static_cast<float2 *>(grp.cov[src]);
    }
    g.split = GroupSplit::make(grp.n);
    fill_cov_args(g, N, K, K, avg, shape.n_out, d_gain_outer, format, scale);
    if (format == DOA_SAMPLE_SC16) launch_cov<Sc16Samples>(rt, g, st);
    else                           launch_cov<Fc32Samples>(rt, g, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
struct doa_autocorrelate : doa::BlockBase {
    int inputs = 0, avg = 0;
    doa::StreamWindow win;
    doa::InputFormat fmt;               // doa_autocorrelate_set_input_format
    doa::DevBuf d_in, d_out, d_gain, d_work;
    bool has_gain = false;
    // K1 for n items on `st`, with the piece-sum workspace of the read-once path (grow-only; growing frees the old buffer,
    // which waits for the device)
    int launch(int n, const void *const *d_in_ptrs, void *d_out_items, hipStream_t st)
    {
        const size_t ws = doa::cov_workspace_bytes(inputs, win.K, win.overlap, n);
        if (int rc = ws ? d_work.reserve(ws) : (int)DOA_OK; rc != DOA_OK) return rc;
        const int rc = doa::launch_autocorrelate(inputs, win.K, win.overlap, avg, n, d_in_ptrs, d_out_items, st,
                                                 has_gain ? d_gain.p : nullptr, ws ? d_work.p : nullptr, fmt.format, fmt.scale);
        return rc == DOA_OK ? n : rc;
    }
};

extern "C" {

doa_autocorrelate_t *doa_autocorrelate_create(int inputs, int snapshot_size, int overlap_size, int avg_method)
{
    doa::clear_error();
    // grc/doa_autocorrelate.xml:41-43 checks; the C++ ctor of the reference does not validate, so a
    // violating call would read/write out of bounds there — here it fails in create.
    if (inputs <= 0 || snapshot_size <= 0 || overlap_size < 0 || overlap_size >= snapshot_size) {
        doa::set_error("autocorrelate: need inputs > 0, snapshot_size > 0, 0 <= overlap_size < snapshot_size "
                       "(got %d, %d, %d)", inputs, snapshot_size, overlap_size);
        return nullptr;
    }
    if (inputs > DOA_MAX_ANT_ELE) {
        doa::set_error("autocorrelate: inputs=%d exceeds DOA_MAX_ANT_ELE=%d", inputs, DOA_MAX_ANT_ELE);
        return nullptr;
    }
    return doa::create_block<doa_autocorrelate>("autocorrelate", [&](doa_autocorrelate &h) {
        h.inputs = inputs; h.avg = avg_method; h.win.K = snapshot_size; h.win.overlap = overlap_size;
        return (int)DOA_OK;
    });
}

void doa_autocorrelate_destroy(doa_autocorrelate_t *h) { doa::destroy_block(h); }

int doa_autocorrelate_fuse_antenna_correction(doa_autocorrelate_t *h, const float *gains_re_im)
{
    doa::clear_error();
    if (!h) return DOA_ERR_INVALID_ARG;
    if (!gains_re_im) { h->has_gain = false; return DOA_OK; }
    const int N = h->inputs;
    float2 w[DOA_MAX_ANT_ELE * DOA_MAX_ANT_ELE];
    for (int b = 0; b < N; b++)
        for (int a = 0; a < N; a++) {
            const float ar = gains_re_im[2 * a], ai = gains_re_im[2 * a + 1], br = gains_re_im[2 * b], bi = gains_re_im[2 * b + 1];
            w[a + b * N] = make_float2(ar * br + ai * bi, ai * br - ar * bi);   // g_a conj(g_b)
        }
    int rc = h->d_gain.reserve(sizeof(float2) * N * N);
    if (rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(h->d_gain.p, w, sizeof(float2) * N * N, hipMemcpyHostToDevice));
    h->has_gain = true;
    return DOA_OK;
}

int doa_autocorrelate_set_input_format(doa_autocorrelate_t *h, int format, float scale)
{
    doa::clear_error();
    return doa::set_input_format("autocorrelate", h ? &h->fmt : nullptr, format, scale);
}

int doa_autocorrelate_history(const doa_autocorrelate_t *h) { return h ? h->win.history() : DOA_ERR_INVALID_ARG; }

int doa_autocorrelate_forecast(const doa_autocorrelate_t *h, int noutput_items)
{
    return h && noutput_items >= 0 ? h->win.forecast(noutput_items) : DOA_ERR_INVALID_ARG;
}

long long doa_autocorrelate_input_span(const doa_autocorrelate_t *h, int noutput_items) { return h ? h->win.input_span(noutput_items) : 0; }

int doa_autocorrelate_work_dev(doa_autocorrelate_t *h, int noutput_items, const void *const *d_input_items,
                               void *d_output_items0, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("autocorrelate_work_dev", h, noutput_items, {d_input_items, d_output_items0}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    return h->launch(noutput_items, d_input_items, d_output_items0, static_cast<hipStream_t>(hip_stream));
}

int doa_autocorrelate_work(doa_autocorrelate_t *h, int noutput_items, const void *const *input_items,
                           void *output_items0)
{
    doa::clear_error();
    if (int rc = doa::work_args("autocorrelate_work", h, noutput_items, {input_items, output_items0}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    const int N = h->inputs;
    doa::HostCall io(*h);
    const void *d_ptrs[DOA_MAX_ANT_ELE];
    // (the device copies start on their stride boundaries, 16-byte aligned, whatever the caller's alignment)
    io.in_streams("autocorrelate_work", h->d_in, input_items, N, (size_t)h->win.input_span(noutput_items) * h->fmt.sample_bytes(), d_ptrs);
    int rc = io.out(h->d_out, output_items0, (size_t)noutput_items * N * N * sizeof(float2));
    if (rc == DOA_OK) rc = h->launch(noutput_items, d_ptrs, h->d_out.p, h->stream);
    return io.finish(rc);
}

}  // extern "C"
