// capon.hip — the Capon (MVDR) spectrum of a uniform linear array on gfx950: capon_inverse_kernel (the C ABI of
// doa_capon_lin_array: spectrum_blocks.hip).  Not a block of the reference; the definition is stated once in include/doa_hip.h.
//
// For a ULA the scan kernels (music_scan_impl.hpp) never see a matrix, only its diagonal sums u_l = sum_r W[r+l, r]
// (music.hip:8-13), and they output 1/Q normalised to the row maximum.  So the Capon spectrum 1 / (a^H R^-1 a) is the MUSIC
// chain with ONE launch replaced: instead of the eigen stage, capon_inverse_kernel writes the record of
// W = (H / mu + delta I)^-1.  Scan, fused peak pick, find_local_max and spatial smoothing run unchanged.
//
// W = L^-H L^-1 with A = L L^H (Cholesky), M = L^-1 lower triangular:  W[i,j] = sum_k conj(M[k,i]) M[k,j], so
//     u_l = sum_k sum_r conj(M[k, r+l]) M[k, r]:
// row k of M contributes on its own, and W is never formed (except for the diagnostics entry).
//   N <= 4   capon_inverse_lane_kernel   one lane per item, the lower triangle in registers, everything unrolled
//   N <= 8   capon_inverse_group_kernel<8>   8 lanes per item, 8 items per wave
//   N <= 16  capon_inverse_group_kernel<16>  16 lanes per item, 4 items per wave
//            lane r owns row r of A / L and row r of M; columns travel inside the group by __shfl.  Every register array is
//            indexed by unrolled loop counters only (a lane's own diagonal entry lives in a scalar, not in its row array).
// No iteration, no atomics, no data-dependent trip count: the time of a launch depends on N and n_items alone, and an item's
// result on nothing but the item.  A failing item (status 1) computes on with whatever its arithmetic gives -- no lane leaves
// a cross-lane operation -- and its record is replaced by NaN at the end.
#include "kernels.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace doa {
namespace {

constexpr double kPivotMin = DOA_CAPON_PIVOT_MIN;

// ---- N <= 4: one lane per item ---------------------------------------------------------------------------------------------
template <int N, bool WOUT>
__global__ __launch_bounds__(64) void capon_inverse_lane_kernel(const float2 *__restrict__ R, double loading,
                                                                double *__restrict__ coef_d, double *__restrict__ cheb_d,
                                                                float2 *__restrict__ w_out, int *__restrict__ status, int n_items,
                                                                double *__restrict__ full_out)
{
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= n_items) return;
    const float2 *__restrict__ Ri = R + (size_t)item * (N * N);
    // lower triangle, A[i][j] = conj(H[j][i]) for j <= i: first A, then L in place (its diagonal as the reciprocal dinv)
    double lr[N][N], li[N][N], dinv[N];
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const float2 x = Ri[j + i * N];
            lr[i][j] = (double)x.x;
            li[i][j] = (i == j) ? 0.0 : -(double)x.y;
        }
        tr += lr[i][i];
    }
    const double mu = tr / (double)N;
    bool bad = !(mu > 0.0);
    const double rmu = 1.0 / mu;
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) { lr[i][j] *= rmu; li[i][j] *= rmu; }
        lr[i][i] += loading;
    }
    // Cholesky, column by column
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double ajj = lr[j][j];
        double s = ajj;
#pragma unroll
        for (int k = 0; k < j; k++) s -= fma(lr[j][k], lr[j][k], li[j][k] * li[j][k]);
        bad = bad || !(s > kPivotMin * ajj);
        const double rs = 1.0 / sqrt(s);
        dinv[j] = rs;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double xr = lr[i][j], xi = li[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) {           // x -= L[i][k] conj(L[j][k])
                xr -= fma(lr[i][k], lr[j][k], li[i][k] * li[j][k]);
                xi -= fma(li[i][k], lr[j][k], -(lr[i][k] * li[j][k]));
            }
            lr[i][j] = xr * rs; li[i][j] = xi * rs;
        }
    }
    // M = L^-1 (lower triangular; real diagonal)
    double mr[N][N], mi[N][N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        mr[j][j] = dinv[j]; mi[j][j] = 0.0;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double xr = 0.0, xi = 0.0;
#pragma unroll
            for (int k = j; k < i; k++) {           // x += L[i][k] M[k][j]
                xr += fma(lr[i][k], mr[k][j], -(li[i][k] * mi[k][j]));
                xi += fma(lr[i][k], mi[k][j], li[i][k] * mr[k][j]);
            }
            mr[i][j] = -xr * dinv[i]; mi[i][j] = -xi * dinv[i];
        }
    }
    // u_l = sum_r sum_{k >= r+l} conj(M[k][r+l]) M[k][r]
    double ux[4] = {0, 0, 0, 0}, uy[4] = {0, 0, 0, 0};
    double fin = 0.0;
#pragma unroll
    for (int l = 0; l < N; l++) {
        double tr_ = 0.0, ti_ = 0.0;
#pragma unroll
        for (int r = 0; r + l < N; r++) {
#pragma unroll
            for (int k = r + l; k < N; k++) {
                tr_ = fma(mr[k][r + l], mr[k][r], fma(mi[k][r + l], mi[k][r], tr_));
                ti_ = fma(mr[k][r + l], mi[k][r], fma(-mi[k][r + l], mr[k][r], ti_));
            }
        }
        ux[l] = tr_; uy[l] = (l == 0) ? 0.0 : ti_;
        fin = fma(tr_, 0.0, fma(ti_, 0.0, fin));
    }
    bad = bad || !(fin == 0.0);
    if (bad) {
#pragma unroll
        for (int l = 0; l < 4; l++) { ux[l] = (l < N) ? (double)NAN : 0.0; uy[l] = (l < N && l > 0) ? (double)NAN : 0.0; }
    }
    if (status) status[item] = bad ? 1 : 0;
    if (coef_d) {                                        // (NULL on a steering-table handle: its scan reads the full record)
        double *cd = coef_d + (size_t)item * (2 * N);
        cd[0] = ux[0];
#pragma unroll
        for (int l = 1; l < N; l++) { cd[2 * l - 1] = ux[l]; cd[2 * l] = uy[l]; }
        cd[2 * N - 1] = 0.0;
    }
    if (cheb_d) write_cheb_record(cheb_d + (size_t)item * kChebRecord, ux, uy);
    if constexpr (WOUT) {
        const size_t off = (size_t)item * (N * N);
#pragma unroll
        for (int i = 0; i < N; i++) {
#pragma unroll
            for (int j = i; j < N; j++) {
                double wr = 0.0, wi = 0.0;             // W[i][j] = sum_{k >= j} conj(M[k][i]) M[k][j]
#pragma unroll
                for (int k = j; k < N; k++) {
                    wr = fma(mr[k][i], mr[k][j], fma(mi[k][i], mi[k][j], wr));
                    wi = fma(mr[k][i], mi[k][j], fma(-mi[k][i], mr[k][j], wi));
                }
                if (bad) { wr = (double)NAN; wi = (double)NAN; }
                if (w_out) {
                    float2 *wo = w_out + off;
                    wo[i + j * N] = make_float2((float)wr, (float)((i == j) ? 0.0 : wi));
                    if (i != j) wo[j + i * N] = make_float2((float)wr, (float)-wi);
                }
                if (full_out) {                        // the full record (kernels.hpp), before any rounding
                    double *fo = full_out + off;
                    fo[i + j * N] = wr;
                    if (i != j) fo[j + i * N] = wi;
                }
            }
        }
    }
}

// ---- 4 < N <= 16: G lanes per item, lane r owns row r ---------------------------------------------------------------------
// A lane keeps the strict lower part of its row in ar / ai (entries c < r) and its diagonal entry apart in dg, so that no
// array is indexed by the lane number.  Rows and columns N .. G-1 are padding: their lanes hold zeros and contribute
// nothing, and the elimination steps beyond N are skipped (N is wave-uniform).  Entries c > r of a lane's arrays are
// updated by the unrolled code like the others; they are masked to zero when their column's step comes, before anything
// reads them.
template <int G, bool WOUT>
__global__ __launch_bounds__(64) void capon_inverse_group_kernel(const float2 *__restrict__ R, double loading,
                                                                 double *__restrict__ coef_d, float2 *__restrict__ w_out,
                                                                 int *__restrict__ status, int n_items, int N,
                                                                 double *__restrict__ full_out)
{
    constexpr int IPW = kWave / G;                       // items per wave
    const int lane = threadIdx.x & (kWave - 1);
    const int r = lane % G, base = lane - r;
    int item = blockIdx.x * IPW + lane / G;
    const bool real_item = item < n_items;
    if (!real_item) item = n_items - 1;                  // idle groups shadow the last item (no stores)
    const float2 *__restrict__ Ri = R + (size_t)item * (N * N);
    const bool row = r < N;

    // row r of the lower triangle: A[r][c] = conj(H[c][r]) = conj(Ri[c + r N]), c <= r (one contiguous run of column r).
    // Every load is issued (indices clamped into the item) and masked afterwards: no load waits behind a branch.
    const int rr = row ? r : N - 1;
    double ar[G], ai[G];
    double dg = 0.0;
#pragma unroll
    for (int c = 0; c < G; c++) {
        const float2 x = Ri[(c < rr ? c : rr) + rr * N];
        const bool low = row && c < r;
        ar[c] = low ? (double)x.x : 0.0;
        ai[c] = low ? -(double)x.y : 0.0;
        if (c == r) dg = (double)x.x;
    }
    const double mu = group_sum<G, double>(row ? dg : 0.0, lane) / (double)N;
    bool bad = !(mu > 0.0);
    const double rmu = 1.0 / mu;
#pragma unroll
    for (int c = 0; c < G; c++) { ar[c] *= rmu; ai[c] *= rmu; }
    dg = row ? dg * rmu + loading : 1.0;
    const double diag = dg;                              // A[r][r], for the pivot test

    // Cholesky, right-looking: step j scales column j and takes its outer product off the columns behind it; dg ends as
    // the lane's own pivot s_r
#pragma unroll
    for (int j = 0; j < G; j++) {
        if (j < N) {
            const double rs = 1.0 / sqrt(lane_fetch<double>(dg, base + j));        // 1 / L[j][j]
            const bool below = r > j;
            const double lr = below ? ar[j] * rs : 0.0, li = below ? ai[j] * rs : 0.0;      // L[r][j]
            ar[j] = lr; ai[j] = li;
            dg -= fma(lr, lr, li * li);
#pragma unroll
            for (int c = j + 1; c < G; c++) {
                const double cr = lane_fetch<double>(lr, base + c), ci = lane_fetch<double>(li, base + c);      // L[c][j]
                ar[c] -= fma(lr, cr, li * ci);                       // A[r][c] -= L[r][j] conj(L[c][j]), r > c
                ai[c] -= fma(li, cr, -(lr * ci));
            }
        }
    }
    bad = bad || !(dg > kPivotMin * diag);
    const double rd = row ? 1.0 / sqrt(dg) : 0.0;        // M[r][r] = 1 / L[r][r]; 0 on padding lanes

    // M = L^-1 by rows: row r = (e_r - sum_{k<r} L[r][k] row k) / L[r][r]; row k is complete at step k and travels then.
    // mr / mi hold the sum (entries c < r); L[r][k] is zero on the lanes r <= k, which therefore stay as they are.
    double mr[G], mi[G];
#pragma unroll
    for (int c = 0; c < G; c++) { mr[c] = 0.0; mi[c] = 0.0; }
#pragma unroll
    for (int k = 0; k < G - 1; k++) {
        if (k < N - 1) {
            const double lkr = ar[k], lki = ai[k];
#pragma unroll
            for (int c = 0; c < k; c++) {
                const double vr = lane_fetch<double>(mr[c] * rd, base + k), vi = lane_fetch<double>(mi[c] * rd, base + k);   // M[k][c]
                mr[c] -= fma(lkr, vr, -(lki * vi));
                mi[c] -= fma(lkr, vi, lki * vr);
            }
            const double vd = lane_fetch<double>(rd, base + k);                                                         // M[k][k]
            mr[k] -= lkr * vd;
            mi[k] -= lki * vd;
        }
    }
#pragma unroll
    for (int c = 0; c < G; c++) {                        // the row itself, diagonal included (padding lanes: all zero)
        mr[c] = (c == r) ? rd : mr[c] * rd;
        mi[c] = (c == r) ? 0.0 : mi[c] * rd;
    }

    // u_l: this lane's part is sum_c conj(M[r][c+l]) M[r][c]; one group reduction per l; lane l keeps u_l
    double ur = 0.0, ui = 0.0, fin = 0.0;
#pragma unroll
    for (int l = 0; l < G; l++) {
        if (l < N) {
            double tr = 0.0, ti = 0.0;
#pragma unroll
            for (int c = 0; c + l < G; c++) {
                tr = fma(mr[c + l], mr[c], fma(mi[c + l], mi[c], tr));
                ti = fma(mr[c + l], mi[c], fma(-mi[c + l], mr[c], ti));
            }
            tr = group_sum<G, double>(tr, lane);
            ti = (l == 0) ? 0.0 : group_sum<G, double>(ti, lane);
            fin = fma(tr, 0.0, fma(ti, 0.0, fin));
            if (r == l) { ur = tr; ui = ti; }
        }
    }
    bad = bad || !(fin == 0.0);
    bad = group_or<G>(bad ? 1 : 0, lane) != 0;
    if (bad) { ur = (double)NAN; ui = (double)NAN; }
    if (real_item && r == 0 && status) status[item] = bad ? 1 : 0;
    if (real_item && row && coef_d) {                    // (NULL on a steering-table handle: its scan reads the full record)
        double *cd = coef_d + (size_t)item * (2 * N);
        if (r == 0) {
            cd[0] = ur; cd[2 * N - 1] = 0.0;
        } else {
            cd[2 * r - 1] = ur; cd[2 * r] = ui;
        }
    }
    if constexpr (WOUT) {
        const size_t off = (size_t)item * (N * N);
#pragma unroll
        for (int i = 0; i < G; i++) {
#pragma unroll
            for (int j = i; j < G; j++) {
                if (j < N) {
                    double wr = fma(mr[i], mr[j], mi[i] * mi[j]);                  // conj(M[r][i]) M[r][j]
                    double wi = fma(mr[i], mi[j], -(mi[i] * mr[j]));
                    wr = group_sum<G, double>(wr, lane);
                    wi = group_sum<G, double>(wi, lane);
                    if (bad) { wr = (double)NAN; wi = (double)NAN; }
                    if (real_item && r == 0 && w_out) {
                        float2 *wo = w_out + off;
                        wo[i + j * N] = make_float2((float)wr, (float)((i == j) ? 0.0 : wi));
                        if (i != j) wo[j + i * N] = make_float2((float)wr, (float)-wi);
                    }
                    // the full record (kernels.hpp), before any rounding: every lane holds the sums, lane j stores column j
                    if (real_item && r == j && full_out) {
                        double *fo = full_out + off;
                        fo[i + j * N] = wr;
                        if (i != j) fo[j + i * N] = wi;
                    }
                }
            }
        }
    }
}

// One wave per item; a wave with status 0 returns after one load.
__global__ __launch_bounds__(256) void capon_invalid_rows_kernel(const int *__restrict__ status, float *__restrict__ spec, int P,
                                                                 float *__restrict__ mx, float *__restrict__ am, int M, int n_items)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int item = wave_index();
    if (item >= n_items) return;
    if (status[item] == 0) return;
    if (spec) {
        float *row = spec + (size_t)item * P;
        for (int p = lane; p < P; p += kWave) row[p] = NAN;
    }
    if (mx && lane < M) mx[(size_t)item * M + lane] = NAN;
    if (am && lane < M) am[(size_t)item * M + lane] = NAN;
}

template <int N> void launch_capon_lane(int n_items, const void *d_R, double loading, const CaponOut &out, hipStream_t st)
{
    const dim3 grid((n_items + 63) / 64), block(64);
    if (out.w_out || out.full)
        hipLaunchKernelGGL((capon_inverse_lane_kernel<N, true>), grid, block, 0, st, (const float2 *)d_R, loading, out.coef_d, out.cheb_d,
                           out.w_out, out.status, n_items, out.full);
    else
        hipLaunchKernelGGL((capon_inverse_lane_kernel<N, false>), grid, block, 0, st, (const float2 *)d_R, loading, out.coef_d, out.cheb_d,
                           (float2 *)nullptr, out.status, n_items, (double *)nullptr);
}

template <int G> void launch_capon_group(int N, int n_items, const void *d_R, double loading, const CaponOut &out, hipStream_t st)
{
    constexpr int IPW = kWave / G;
    const dim3 grid((n_items + IPW - 1) / IPW), block(64);
    if (out.w_out || out.full)
        hipLaunchKernelGGL((capon_inverse_group_kernel<G, true>), grid, block, 0, st, (const float2 *)d_R, loading, out.coef_d, out.w_out,
                           out.status, n_items, N, out.full);
    else
        hipLaunchKernelGGL((capon_inverse_group_kernel<G, false>), grid, block, 0, st, (const float2 *)d_R, loading, out.coef_d,
                           (float2 *)nullptr, out.status, n_items, N, (double *)nullptr);
}

}  // namespace

int launch_capon_inverse(int N, int n_items, const void *d_R, double loading, const CaponOut &out, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    if (N < 2 || N > DOA_MAX_ANT_ELE) {
        set_error("Capon: num_ant_ele=%d outside the built range 2..%d", N, DOA_MAX_ANT_ELE);
        return DOA_ERR_UNSUPPORTED;
    }
    // the diagonal-sum records are what the ULA scans read; a caller that asks for full records may leave them out
    const bool need_records = !out.full;
    if (!d_R || (need_records && (!out.coef_d || (scan_reads_cheb(N, 64) && !out.cheb_d))) || !(loading >= 0.0) || !std::isfinite(loading)) {
        set_error("Capon: bad arguments of the inverse launch (N=%d, loading=%g)", N, loading);
        return DOA_ERR_INVALID_ARG;
    }
    if (N > 8) launch_capon_group<16>(N, n_items, d_R, loading, out, st);
    else if (N > 4) launch_capon_group<8>(N, n_items, d_R, loading, out, st);
    else if (N == 4) launch_capon_lane<4>(n_items, d_R, loading, out, st);
    else if (N == 3) launch_capon_lane<3>(n_items, d_R, loading, out, st);
    else launch_capon_lane<2>(n_items, d_R, loading, out, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

int launch_capon_invalid_rows(int P, int M, int n_items, const void *d_status, void *d_spec, void *d_max, void *d_argmax, hipStream_t st)
{
    if (n_items <= 0 || (!d_spec && !d_max && !d_argmax)) return DOA_OK;
    hipLaunchKernelGGL(capon_invalid_rows_kernel, dim3((n_items + 3) / 4), dim3(256), 0, st, (const int *)d_status, (float *)d_spec, P,
                       (float *)d_max, (float *)d_argmax, M, n_items);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa
