// focus_covariance.hip — coherent wideband focusing on gfx950 (the coherent signal-subspace method: Wang and Kaveh 1985): one
// focused covariance item per snapshot, R_i = sum_j w_ij T_j H(R_ij) T_j^H / sum_j w_ij over the used bins.  The kernel and its
// launcher, the host routine that builds rotational-signal-subspace focusing matrices (Hung and Kaveh 1988), and the C ABI of
// doa_focus_covariance.  Not a block of the reference; the definition is stated once in include/doa_hip.h.
//
// Structure: one wave per snapshot, nothing crosses snapshots.  The 64 lanes are G row lanes x B = 64 / G bin slots
// (lane = r B + b; G = 4 / 8 / 16 for N <= 4 / 8 / 16), and the wave takes its snapshot's bins B at a time, bin slot b the bins
// b, b + B, b + 2 B, .. in this order:
//   stage   the B items of the round are one contiguous range: coalesced 16-byte loads (8-byte ones where the range does not
//           start on 16 bytes, the same bits either way) into registers one round ahead, then into LDS
//   step 1  lane (r, b) holds row r of T_j in registers (the table is row-major: a coalesced read from L2) and forms row r of
//           Y = T_j H(R): every upper-triangle element of the item is read from LDS once (a broadcast among the row lanes) and
//           serves both y[c] += T[r][k] h and y[k] += T[r][c] conj(h).  w Y's row goes to LDS.
//   step 2  Z = T_j H T_j^H = T_j Y^H, because H is Hermitian: Z[r][c] = sum_k T[r][k] conj(Y[c][k]) needs the lane's own row of
//           T again and row c of Y from LDS.  Lane r accumulates the columns c = r, r + 1, .., r + N/2 (mod N) only: every
//           pair {r, c} once (for even N the distance N/2 twice; the lanes r < N/2 write it), half the arithmetic of full rows
//           and the same for every lane.  Rows of Y are N + 1 apart in LDS so that the lanes' different rows fall in different banks.
// After the last round the bin slots' partial sums are added by wave_ops.hpp's group_sum over the B slots (a fixed tree), divided
// by the weight sum and rounded once; lane (r, 0) stores Z[r][c] and its conjugate mirror, so the item is exactly Hermitian.
// A used item that is not finite makes every row of Y, and so every diagonal sum, not finite: status 3 is read off the sums.
// No atomics; the order of additions depends on nb alone.
#include "kernels.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

namespace doa {
namespace {

template <int N> struct FocusShape {
    static constexpr int G = N <= 4 ? 4 : N <= 8 ? 8 : 16;      // row lanes
    static constexpr int B = kWave / G;                         // bin slots = items per round
    static constexpr int NN = N * N;
    static constexpr int HS = NN + 1;                           // float2 between the round's items in LDS
    static constexpr int YR = N + 1;                            // double2 between the rows of a slot's Y
    static constexpr int YS = N * YR;                           // double2 between the slots' Y
    static constexpr int M = N / 2 + 1;                         // columns per lane in step 2
    static constexpr int Q = ((B * NN + 1) / 2 + kWave - 1) / kWave;    // pairs of float2 per lane and round
};

// A round's items on their way from global memory to LDS: cnt float2 from src, pair p = lane + 64 q per register.
template <int N> struct FocusStage {
    using S = FocusShape<N>;
    doa_f32x4 v[S::Q];
    __device__ __forceinline__ void load(const float2 *src, int cnt, int lane)
    {
        const bool v16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0;          // wave-uniform
#pragma unroll
        for (int q = 0; q < S::Q; q++) {
            const int e = 2 * (lane + kWave * q);
            if (e + 1 < cnt) {
                if (v16) {
                    v[q] = *reinterpret_cast<const doa_f32x4 *>(src + e);
                } else {
                    const float2 lo = src[e], hi = src[e + 1];
                    v[q] = doa_f32x4{lo.x, lo.y, hi.x, hi.y};
                }
            } else if (e < cnt) {
                const float2 lo = src[e];
                v[q] = doa_f32x4{lo.x, lo.y, 0.0f, 0.0f};
            }
        }
    }
    __device__ __forceinline__ void put(float2 *sH, int cnt, int lane) const
    {
#pragma unroll
        for (int q = 0; q < S::Q; q++) {
            const int e = 2 * (lane + kWave * q);
            if (e < cnt) sH[(e / S::NN) * S::HS + e % S::NN] = make_float2(v[q].x, v[q].y);
            if (e + 1 < cnt) sH[((e + 1) / S::NN) * S::HS + (e + 1) % S::NN] = make_float2(v[q].z, v[q].w);
        }
    }
};

template <int N>
__global__ __launch_bounds__(kWave) void focus_covariance_kernel(const float2 *__restrict__ items, const double2 *__restrict__ tab,
                                                                 const float *__restrict__ weights, float2 *__restrict__ out,
                                                                 int *__restrict__ status, int nb)
{
    using S = FocusShape<N>;
    __shared__ float2 sH[S::B * S::HS];
    __shared__ double2 sY[S::B * S::YS];
    const int lane = threadIdx.x;
    const int b = lane % S::B, r = lane / S::B;
    const int snap = blockIdx.x;
    const size_t item0 = (size_t)snap * nb;
    const float2 *src = items + item0 * S::NN;

    double acc_re[S::M], acc_im[S::M];
#pragma unroll
    for (int m = 0; m < S::M; m++) acc_re[m] = acc_im[m] = 0.0;
    double wsum = 0.0;

    FocusStage<N> stage;
    stage.load(src, min(S::B, nb) * S::NN, lane);
    for (int k0 = 0; k0 < nb; k0 += S::B) {
        stage.put(sH, min(S::B, nb - k0) * S::NN, lane);
        __syncthreads();                                        // the round's items are in LDS; step 2 of the last round is over
        if (k0 + S::B < nb) stage.load(src + (size_t)(k0 + S::B) * S::NN, min(S::B, nb - k0 - S::B) * S::NN, lane);
        const int j = k0 + b;
        const float wf = (r < N && j < nb) ? (weights ? weights[item0 + j] : 1.0f) : 0.0f;
        const bool used = bin_weight_used(wf);
        const double w = (double)wf;
        double tr[N], ti[N];
        if (used) {
            const double2 *trow = tab + ((size_t)j * N + r) * N;
#pragma unroll
            for (int k = 0; k < N; k++) { const double2 t = trow[k]; tr[k] = t.x; ti[k] = t.y; }
            // ---- step 1: row r of Y = T H(R) ----
            const float2 *H = sH + b * S::HS;
            double yr[N], yi[N];
#pragma unroll
            for (int c = 0; c < N; c++) yr[c] = yi[c] = 0.0;
#pragma unroll
            for (int c = 0; c < N; c++) {
#pragma unroll
                for (int k = 0; k <= c; k++) {
                    const float2 f = H[k + c * N];
                    const double hr = (double)f.x;
                    if (k == c) {
                        yr[c] = fma(tr[c], hr, yr[c]);
                        yi[c] = fma(ti[c], hr, yi[c]);
                    } else {
                        const double hi = (double)f.y;
                        yr[c] = fma(tr[k], hr, yr[c]); yr[c] = fma(-ti[k], hi, yr[c]);      // y[c] += T[r][k] h
                        yi[c] = fma(tr[k], hi, yi[c]); yi[c] = fma(ti[k], hr, yi[c]);
                        yr[k] = fma(tr[c], hr, yr[k]); yr[k] = fma(ti[c], hi, yr[k]);       // y[k] += T[r][c] conj(h)
                        yi[k] = fma(-tr[c], hi, yi[k]); yi[k] = fma(ti[c], hr, yi[k]);
                    }
                }
            }
            double2 *yrow = sY + b * S::YS + r * S::YR;
#pragma unroll
            for (int c = 0; c < N; c++) yrow[c] = make_double2(w * yr[c], w * yi[c]);
        }
        __syncthreads();                                        // the slots' w Y are in LDS
        if (used) {
            // ---- step 2: acc[m] += sum_k T[r][k] conj(w Y[c][k]), c = r + m (mod N) ----
#pragma unroll
            for (int m = 0; m < S::M; m++) {
                int c = r + m;
                if (c >= N) c -= N;
                const double2 *yc = sY + b * S::YS + c * S::YR;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double2 y = yc[k];
                    acc_re[m] = fma(tr[k], y.x, acc_re[m]); acc_re[m] = fma(ti[k], y.y, acc_re[m]);
                    acc_im[m] = fma(ti[k], y.x, acc_im[m]); acc_im[m] = fma(-tr[k], y.y, acc_im[m]);
                }
            }
            wsum += w;
        }
    }

    // ---- the bin slots' sums, the status, the item ----
#pragma unroll
    for (int m = 0; m < S::M; m++) {
        acc_re[m] = group_sum<S::B>(acc_re[m], lane);
        acc_im[m] = group_sum<S::B>(acc_im[m], lane);
    }
    const double ws = lane_fetch<double>(group_sum<S::B>(wsum, lane), 0);
    int bad = 0;
    if (r < N) {
#pragma unroll
        for (int m = 0; m < S::M; m++) bad |= (__builtin_isfinite(acc_re[m]) && __builtin_isfinite(acc_im[m])) ? 0 : 1;
    }
    bad = group_or<kWave>(bad, lane);
    const int st = !(ws > 0.0) ? 1 : bad ? 3 : 0;               // wave-uniform
    if (lane == 0 && status) status[snap] = st;
    float2 *o = out + (size_t)snap * S::NN;
    if (st != 0) {
        for (int e = lane; e < S::NN; e += kWave) o[e] = make_float2(NAN, NAN);
        return;
    }
    if (b == 0 && r < N) {
        o[r + r * N] = make_float2((float)(acc_re[0] / ws), 0.0f);
#pragma unroll
        for (int m = 1; m < S::M; m++) {
            if (N % 2 == 0 && m == N / 2 && r >= N / 2) continue;       // the pair {r, r + N/2} belongs to the lower lane
            int c = r + m;
            if (c >= N) c -= N;
            const float x = (float)(acc_re[m] / ws), y = (float)(acc_im[m] / ws);
            o[r + c * N] = make_float2(x, y);
            o[c + r * N] = make_float2(x, -y);
        }
    }
}

}  // namespace

int FocusTables::build(int num_ant_ele, int num_bins_, const double *matrices)
{
    N = num_ant_ele; num_bins = num_bins_;
    const size_t bytes = (size_t)num_bins * N * N * sizeof(double2);
    if (int rc = d_t.reserve(bytes); rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_t.p, matrices, bytes, hipMemcpyHostToDevice));
    return DOA_OK;
}

int launch_focus_covariance(const FocusTables &t, int n, const void *d_items, const void *d_weights, void *d_out, void *d_status,
                            hipStream_t st)
{
    if (n <= 0) return DOA_OK;
    if (t.N < 2 || t.N > DOA_MAX_ANT_ELE || t.num_bins < 1 || !t.d_t.p || !d_items || !d_out ||
        (reinterpret_cast<uintptr_t>(d_items) | reinterpret_cast<uintptr_t>(d_out)) % sizeof(float2)) {
        set_error("focus_covariance: bad arguments (N=%d, %d bins, or items not 8-byte aligned)", t.N, t.num_bins);
        return DOA_ERR_INVALID_ARG;
    }
    switch (t.N) {
#define DOA_FOCUS_CASE(N_)                                                                                                      \
    case N_:                                                                                                                    \
        hipLaunchKernelGGL(focus_covariance_kernel<N_>, dim3(n), dim3(kWave), 0, st, (const float2 *)d_items,                    \
                           t.d_t.as<double2>(), (const float *)d_weights, (float2 *)d_out, (int *)d_status, t.num_bins);         \
        break;
    DOA_FOCUS_CASE(2) DOA_FOCUS_CASE(3) DOA_FOCUS_CASE(4) DOA_FOCUS_CASE(5) DOA_FOCUS_CASE(6) DOA_FOCUS_CASE(7) DOA_FOCUS_CASE(8)
    DOA_FOCUS_CASE(9) DOA_FOCUS_CASE(10) DOA_FOCUS_CASE(11) DOA_FOCUS_CASE(12) DOA_FOCUS_CASE(13) DOA_FOCUS_CASE(14)
    DOA_FOCUS_CASE(15) DOA_FOCUS_CASE(16)
#undef DOA_FOCUS_CASE
    }
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

// ---- rotational-signal-subspace focusing matrices (host) --------------------------------------------------------------------
namespace {

using cplx = std::complex<double>;

// inv = A^-1 by Gauss-Jordan elimination with partial pivoting (row-major N x N); false for a singular or non-finite matrix
bool invert_matrix(int N, const cplx *A, cplx *inv)
{
    std::vector<cplx> a(A, A + N * N);
    for (int i = 0; i < N; i++)
        for (int k = 0; k < N; k++) inv[i * N + k] = i == k ? 1.0 : 0.0;
    for (int col = 0; col < N; col++) {
        int piv = col;
        for (int i = col + 1; i < N; i++)
            if (std::abs(a[i * N + col]) > std::abs(a[piv * N + col])) piv = i;
        const double mag = std::abs(a[piv * N + col]);
        if (!(mag > 0.0) || !std::isfinite(mag)) return false;
        if (piv != col)
            for (int k = 0; k < N; k++) { std::swap(a[piv * N + k], a[col * N + k]); std::swap(inv[piv * N + k], inv[col * N + k]); }
        const cplx s = 1.0 / a[col * N + col];
        for (int k = 0; k < N; k++) { a[col * N + k] *= s; inv[col * N + k] *= s; }
        for (int i = 0; i < N; i++) {
            if (i == col) continue;
            const cplx f = a[i * N + col];
            if (f == 0.0) continue;
            for (int k = 0; k < N; k++) { a[i * N + k] -= f * a[col * N + k]; inv[i * N + k] -= f * inv[col * N + k]; }
        }
    }
    return true;
}

double norm_one(int N, const cplx *A, bool by_rows)
{
    double best = 0.0;
    for (int i = 0; i < N; i++) {
        double s = 0.0;
        for (int k = 0; k < N; k++) s += std::abs(by_rows ? A[i * N + k] : A[k * N + i]);
        best = std::max(best, s);
    }
    return best;
}

// X <- its unitary polar factor, by the Newton iteration X <- (g X + (g X)^-H) / 2 with Higham's scaling
// g = (|X^-1|_1 |X^-1|_inf / (|X|_1 |X|_inf))^(1/4) until the steps are small, unscaled (quadratic convergence) from there.
bool polar_factor(int N, cplx *X)
{
    std::vector<cplx> Y(N * N), Xn(N * N);
    bool scale = true;
    for (int it = 0; it < 100; it++) {
        if (!invert_matrix(N, X, Y.data())) return false;
        double g = 1.0;
        if (scale) g = std::pow(norm_one(N, Y.data(), false) * norm_one(N, Y.data(), true) / (norm_one(N, X, false) * norm_one(N, X, true)), 0.25);
        double diff = 0.0, size = 0.0;
        for (int a = 0; a < N; a++)
            for (int b = 0; b < N; b++) {
                Xn[a * N + b] = 0.5 * (g * X[a * N + b] + std::conj(Y[b * N + a]) / g);
                diff += std::norm(Xn[a * N + b] - X[a * N + b]);
                size += std::norm(Xn[a * N + b]);
            }
        for (int i = 0; i < N * N; i++) X[i] = Xn[i];
        if (!std::isfinite(diff)) return false;
        if (diff <= 1e-4 * size) scale = false;                 // |step| <= 1e-2 |X|
        if (diff <= 1e-20 * size) return true;                  // |step| <= 1e-10 |X|: the next step is below rounding
    }
    return false;
}

}  // namespace
}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"

struct doa_focus_covariance : doa::BlockBase {
    doa::FocusTables tab;
    doa::DevBuf d_in, d_w, d_out, d_status;
};

namespace {

int focus_args(const char *who, const doa_focus_covariance *h, int n, const void *items, const void *out)
{
    if (int rc = doa::work_args(who, h, n, {items, out}); rc != DOA_OK) return rc;
    if (int rc = doa::snapshot_items(who, n, h->tab.num_bins); rc != DOA_OK) return rc;
    return doa::need_bits64(who, h->bits, "focusing");
}

}  // namespace

extern "C" {

int doa_rss_focusing_matrices(float norm_spacing, int num_ant_ele, int fft_len, int first_bin, int num_bins, double rate_over_carrier,
                              int n_focus, const double *focus_angles_deg, double regularization, double *matrices_out)
{
    constexpr const char *who = "rss_focusing_matrices";
    doa::clear_error();
    const int N = num_ant_ele, J = n_focus;
    if (N < 2 || N > DOA_MAX_ANT_ELE) {
        doa::set_error("%s: need 2 <= num_ant_ele <= %d (got %d)", who, DOA_MAX_ANT_ELE, N);
        return DOA_ERR_INVALID_ARG;
    }
    if (int rc = doa::check_norm_spacing(who, norm_spacing); rc != DOA_OK) return rc;
    if (doa::fft_len_log2(fft_len) < 0) {
        doa::set_error("%s: fft_len must be 16, 32, 64, 128 or 256 (got %d)", who, fft_len);
        return DOA_ERR_INVALID_ARG;
    }
    if (int rc = doa::check_bin_selection(who, fft_len, first_bin, num_bins); rc != DOA_OK) return rc;
    if (int rc = doa::check_rate_over_carrier(who, rate_over_carrier); rc != DOA_OK) return rc;
    if (J < 1) {
        doa::set_error("%s: need n_focus >= 1 focus angles (got %d)", who, J);
        return DOA_ERR_INVALID_ARG;
    }
    if (!focus_angles_deg || !matrices_out) {
        doa::set_error("%s: focus_angles_deg and matrices_out must not be NULL", who);
        return DOA_ERR_INVALID_ARG;
    }
    for (int k = 0; k < J; k++)
        if (!std::isfinite(focus_angles_deg[k])) {
            doa::set_error("%s: focus angle %d is not finite", who, k);
            return DOA_ERR_INVALID_ARG;
        }
    if (!(regularization > 0.0) || !std::isfinite(regularization)) {
        doa::set_error("%s: regularization must be positive and finite (got %g)", who, regularization);
        return DOA_ERR_INVALID_ARG;
    }
    const doa::BinSelection sel{fft_len, first_bin, num_bins};
    if (int rc = doa::check_bin_spacings(who, norm_spacing, rate_over_carrier, sel); rc != DOA_OK) return rc;
    // A_d[n][k] = exp(i psi_k (N - 1 - 2n) / 2), psi_k = -2 pi cos(theta_k) d
    std::vector<double> kk(J);
    for (int k = 0; k < J; k++) kk[k] = -1.0 * 2 * M_PI * std::cos(focus_angles_deg[k] * (M_PI / 180.0));
    auto steering = [&](double d, std::vector<doa::cplx> &A) {
        for (int n = 0; n < N; n++)
            for (int k = 0; k < J; k++) A[n * J + k] = std::polar(1.0, kk[k] * d * ((N - 1 - 2 * n) / 2.0));
    };
    std::vector<doa::cplx> A0(N * J), Aj(N * J), X(N * N);
    steering((double)norm_spacing, A0);
    for (int j = 0; j < num_bins; j++) {
        const int f = sel.bin(j);
        steering(doa::wideband_bin_spacing(norm_spacing, rate_over_carrier, fft_len, f), Aj);
        for (int a = 0; a < N; a++)
            for (int b = 0; b < N; b++) {
                doa::cplx s = a == b ? regularization * J : 0.0;
                for (int k = 0; k < J; k++) s += A0[a * J + k] * std::conj(Aj[b * J + k]);
                X[a * N + b] = s;
            }
        if (!doa::polar_factor(N, X.data())) {
            doa::set_error("%s: the polar iteration did not converge at bin %d", who, f);
            return DOA_ERR_INVALID_ARG;
        }
        for (int i = 0; i < N * N; i++) {
            matrices_out[2 * ((size_t)j * N * N + i)] = X[i].real();
            matrices_out[2 * ((size_t)j * N * N + i) + 1] = X[i].imag();
        }
    }
    return DOA_OK;
}

doa_focus_covariance_t *doa_focus_covariance_create(int num_ant_ele, int num_bins, const double *matrices)
{
    constexpr const char *who = "focus_covariance";
    doa::clear_error();
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("%s: need 2 <= num_ant_ele <= %d (got %d)", who, DOA_MAX_ANT_ELE, num_ant_ele);
        return nullptr;
    }
    if (num_bins < 1 || num_bins > 256) {
        doa::set_error("%s: need 1 <= num_bins <= 256 (got %d)", who, num_bins);
        return nullptr;
    }
    if (!matrices) {
        doa::set_error("%s: the table of focusing matrices is NULL", who);
        return nullptr;
    }
    const size_t len = (size_t)2 * num_bins * num_ant_ele * num_ant_ele;
    for (size_t i = 0; i < len; i++)
        if (!std::isfinite(matrices[i])) {
            doa::set_error("%s: the focusing matrix of bin slot %d has an entry that is not finite", who,
                           (int)(i / ((size_t)2 * num_ant_ele * num_ant_ele)));
            return nullptr;
        }
    return doa::create_block<doa_focus_covariance>(who, [&](doa_focus_covariance &h) { return h.tab.build(num_ant_ele, num_bins, matrices); });
}
void doa_focus_covariance_destroy(doa_focus_covariance_t *h) { doa::destroy_block(h); }
long long doa_focus_covariance_items_total(const doa_focus_covariance_t *h) { return h ? h->items_total : 0; }

int doa_focus_covariance_work_dev(doa_focus_covariance_t *h, int noutput_items, const void *d_cov_items, const void *d_weights,
                                  void *d_focused_items, void *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = focus_args("focus_covariance_work_dev", h, noutput_items, d_cov_items, d_focused_items); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int rc = doa::launch_focus_covariance(h->tab, noutput_items, d_cov_items, d_weights, d_focused_items, d_status_out,
                                                static_cast<hipStream_t>(hip_stream));
    if (rc != DOA_OK) return rc;
    h->items_total += noutput_items;
    return noutput_items;
}

int doa_focus_covariance_work(doa_focus_covariance_t *h, int noutput_items, const void *cov_items, const float *weights,
                              void *focused_items, void *status_out)
{
    doa::clear_error();
    if (int rc = focus_args("focus_covariance_work", h, noutput_items, cov_items, focused_items); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    const int N = h->tab.N;
    const size_t items = (size_t)noutput_items * h->tab.num_bins;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, items * N * N * sizeof(float2));
    if (weights) io.in(h->d_w, weights, items * sizeof(float));
    io.out(h->d_out, focused_items, (size_t)noutput_items * N * N * sizeof(float2));
    if (status_out) io.out(h->d_status, status_out, (size_t)noutput_items * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = doa_focus_covariance_work_dev(h, noutput_items, h->d_in.p, weights ? h->d_w.p : nullptr, h->d_out.p,
                                           status_out ? h->d_status.p : nullptr, h->stream);
    return io.finish(rc);
}

}  // extern "C"
