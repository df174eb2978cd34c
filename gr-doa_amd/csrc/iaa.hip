// iaa.hip — the iterative adaptive (IAA) power spectrum of a uniform linear array on gfx950: iaa_wave_kernel, its launcher
// and the C ABI of doa_iaa_lin_array.  Not a block of the reference; the definition is stated once in include/doa_hip.h.
//
// With w_k = conj(z_k), z_k = exp(j psi_k) the phase table of MUSIC_lin_array (music.hip), a steering vector is a common
// phase times (1, w_k, w_k^2, ...), and the common phase drops out of everything below.  Two facts keep the kernel small:
//   * R = sum_k p_k a_k a_k^H + delta I is Hermitian Toeplitz, fixed by the N lags r_l = sum_k p_k w_k^l (R[i][j] = r_{i-j}, i >= j);
//   * a^H X a = u_0 + 2 Re sum_l u_l z^l with the diagonal sums u_l = sum_r X[r+l][r] (music.hip:8-13) for X = H / mu, W and B.
// p_k itself is never stored between iterations: the sweep that accumulates the lags of iteration t+1 evaluates p_k from the
// two coefficient records iteration t left in LDS.  One iteration of one item is therefore
//   one sweep over the grid (two Horner chains of degree N-1 and N lag accumulators per direction; z_k is read from the
//   handle's table, which every item shares and the caches hold), a butterfly reduction of the 2 N lag sums, and the small dense
//   step in LDS: Cholesky of R (left-looking, lane i = row i), M = L^-1 (lane j = column j), W = M^H M, T = W (H / mu),
//   B = T W (one entry per lane and pass), the two records of diagonal sums.
// Shape: ONE WAVE PER ITEM, one wave per workgroup, at every N and P of the built range.  A workgroup's barriers are then
// free and nothing crosses a wave.  While one item is in its dense step, a chain of LDS round trips on a few lanes, its
// SIMD has only the other waves resident on it to run: 3 to 6 by the report below, and at 4096 items each of the 1024 SIMDs
// gets 4 waves in all, so that step is hidden in part only.  Three instantiations of the launcher; what separates them is
// the compile-time bound NT of the unrolled loops of the sweep (steps from N on are skipped by a wave-uniform test):
//   iaa_wave_kernel<4>  N = 2..4     iaa_wave_kernel<8>  N = 5..8     iaa_wave_kernel<16>  N = 9..16
// All arithmetic is in double.  No atomics, no scratch, no data-dependent trip count, no early exit: the time of a launch
// depends on N, P, the iteration count and n_items alone, and an item's result on nothing but the item.  A failing item
// (status 1) computes on with whatever its arithmetic gives and its rows are replaced by NaN at the end.
// Resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no AGPRs, scratch 0 in all three,
// and the build fails on a non-zero scratch size):
//   iaa_wave_kernel<4>    78 VGPRs,  1184 B LDS, occupancy 6 waves per SIMD
//   iaa_wave_kernel<8>    95 VGPRs,  3904 B LDS, occupancy 5
//   iaa_wave_kernel<16>  163 VGPRs, 13952 B LDS, occupancy 3
// (profiles/iaa.txt has the times: 4.4 to 5.1 times those of the sweeps' flops at the FP64 peak.  Seen in the assembly, not
// measured apart: the per-step tests on N put a scalar branch around every unrolled step and make the 2 N butterflies of the
// reduction wait one after another, and the dense step is a chain of LDS round trips.  DESIGN.md section 8: what is left.)
#include "block_host.hpp"
#include "kernels.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace doa {
namespace {

constexpr double kPivotMin = DOA_CAPON_PIVOT_MIN;
constexpr float kIaaDbPerUnit = 4.3429448190325183f;    // 10 / ln(10)

// Everything one item keeps in LDS.  Rows are LD = NT + 1 entries apart, so that lanes reading down a column hit distinct banks.
template <int NT> struct IaaLds {
    static constexpr int LD = NT + 1;
    double2 a[NT * LD];     // L (strict lower part), then W
    double2 m[NT * LD];     // M = L^-1 (lower), then T = W (H / mu), then B = T W
    double2 h[NT * LD];     // H / mu
    double2 u[2][NT];       // the coefficient records: [0] of W (before the first iteration: of H / mu), [1] of B
    double2 lag[NT];        // r_l
    double dinv[NT];        // 1 / L[j][j]
};

// p_k from the records.  START: the Bartlett spectrum Re(a^H (H / mu) a) / N^2; otherwise n / g^2, g = Re(a^H W a),
// n = max(Re(a^H B a), 0) (a NaN stays a NaN).  Horner from the highest lag down; N is wave-uniform.
template <int NT, bool START>
__device__ __forceinline__ double iaa_power(const double2 *uw, const double2 *ub, int N, double zr, double zi, double inv_n2)
{
    double gr = 0.0, gi = 0.0, br = 0.0, bi = 0.0;
#pragma unroll
    for (int l = NT - 1; l >= 1; l--) {
        if (l < N) {
            const double2 cw = uw[l];
            const double t = fma(gr, zr, fma(-gi, zi, cw.x));
            gi = fma(gr, zi, fma(gi, zr, cw.y));
            gr = t;
            if constexpr (!START) {
                const double2 cb = ub[l];
                const double tb = fma(br, zr, fma(-bi, zi, cb.x));
                bi = fma(br, zi, fma(bi, zr, cb.y));
                br = tb;
            }
        }
    }
    const double g = fma(2.0, fma(gr, zr, -(gi * zi)), uw[0].x);
    if constexpr (START) return g * inv_n2;
    const double b = fma(2.0, fma(br, zr, -(bi * zi)), ub[0].x);
    const double nn = (b < 0.0) ? 0.0 : b;
    return nn / (g * g);
}

// r_l += p w^l, w = conj(z), l = 0 .. N-1
template <int NT> __device__ __forceinline__ void iaa_accumulate(double (&lr)[NT], double (&li)[NT], int N, double p, double zr, double zi)
{
    double xr = p, xi = 0.0;
#pragma unroll
    for (int l = 0; l < NT; l++) {
        if (l < N) {
            lr[l] += xr; li[l] += xi;
            const double t = fma(xr, zr, xi * zi);
            xi = fma(xi, zr, -(xr * zi));
            xr = t;
        }
    }
}

// One sweep: the lags of the next R from the records in LDS, reduced over the wave (the balanced tree of
// wave_butterfly_sum_xor: the same bits in every lane) and left in s.lag.  Lane `lane` takes the directions lane + 64 c in
// ascending order; the directions past P of the last chunk add zeros.  The phases of the next chunk are fetched before the
// arithmetic of the current one.
template <int NT, bool START>
__device__ __forceinline__ void iaa_sweep(IaaLds<NT> &s, const double2 *__restrict__ zd, int N, int P, int lane, double inv_n2)
{
    double lr[NT], li[NT];
#pragma unroll
    for (int l = 0; l < NT; l++) { lr[l] = 0.0; li[l] = 0.0; }
    double2 z = zd[lane < P ? lane : P - 1];
    for (int k0 = 0; k0 < P; k0 += kWave) {
        const int k = k0 + lane, kn = k + kWave;
        const double2 zn = zd[kn < P ? kn : P - 1];
        // the records are re-read from LDS in every chunk (a broadcast read per Horner step) instead of being held in up to
        // 128 registers next to the 64 of the accumulators, which would leave one wave per SIMD at NT = 16
        asm volatile("" ::: "memory");
        double p = iaa_power<NT, START>(s.u[0], s.u[1], N, z.x, z.y, inv_n2);
        if (k >= P) p = 0.0;
        iaa_accumulate<NT>(lr, li, N, p, z.x, z.y);
        z = zn;
    }
#pragma unroll
    for (int l = 0; l < NT; l++) {
        if (l < N) {
            const double r = wave_butterfly_sum_xor<double>(lr[l]);
            const double i = wave_butterfly_sum_xor<double>(li[l]);
            if (lane == l) s.lag[l] = make_double2(r, (l == 0) ? 0.0 : i);
        }
    }
    __syncthreads();
}

// The dense step: from s.lag the records of W = R^-1 and B = W (H / mu) W in s.u.  `bad` collects a failed pivot (the same in
// every lane) and non-finite records (per lane; the caller ORs over the wave at the end).  The matrices are in LDS, so the
// loops over the array size run to N itself (wave-uniform), not to the compile-time bound.
template <int NT> __device__ __forceinline__ void iaa_factor(IaaLds<NT> &s, int N, double loading, int lane, bool &bad)
{
    constexpr int LD = IaaLds<NT>::LD;
    constexpr int CE = (NT * NT + kWave - 1) / kWave;    // entries of an NT x NT matrix per lane
    const double a00 = s.lag[0].x + loading;             // every diagonal entry of R
    // The Cholesky and the inverse below issue every LDS read unconditionally and mask afterwards.  So they also read cells
    // that hold no entry of L or M: s.a[i][k] for k >= i and s.m above the diagonal, which were never written or still hold
    // the last iteration's W and B (NaN included).  Those values only reach results that the i > j and k >= jc guards drop:
    // they are selected away, never multiplied into something that is kept.
    {   // Cholesky R = L L^H, left-looking: at step j lane i >= j finishes L[i][j]; lanes i < j compute and drop a value
        const int i = lane;
        const bool row = i < N;
        const int ic = row ? i : 0;
        for (int j = 0; j < N; j++) {
            double2 x = s.lag[(row && i >= j) ? i - j : 0];
            if (i == j) x.x += loading;
            for (int k = 0; k < j; k++) {                // x -= L[i][k] conj(L[j][k])
                const double2 lik = s.a[ic * LD + k], ljk = s.a[j * LD + k];
                x.x -= fma(lik.x, ljk.x, lik.y * ljk.y);
                x.y -= fma(lik.y, ljk.x, -(lik.x * ljk.y));
            }
            const double sj = lane_fetch<double>(x.x, j);                    // the pivot s_j
            bad = bad || !(sj > kPivotMin * a00);
            const double rs = 1.0 / sqrt(sj);
            if (row && i > j) s.a[i * LD + j] = make_double2(x.x * rs, x.y * rs);
            if (i == j) s.dinv[j] = rs;
            __syncthreads();
        }
    }
    {   // M = L^-1, lane j = column j: M[i][j] = -(sum_{k=j}^{i-1} L[i][k] M[k][j]) / L[i][i], rows in ascending order
        const bool col = lane < N;
        const int jc = col ? lane : 0;
        if (col) s.m[jc * LD + jc] = make_double2(s.dinv[jc], 0.0);
        for (int i = 1; i < N; i++) {
            double xr = 0.0, xi = 0.0;
            for (int k = 0; k < i; k++) {
                const double2 l = s.a[i * LD + k], mm = s.m[k * LD + jc];
                if (col && k >= jc) {
                    xr += fma(l.x, mm.x, -(l.y * mm.y));
                    xi += fma(l.x, mm.y, l.y * mm.x);
                }
            }
            const double di = s.dinv[i];
            if (col && i > jc) s.m[i * LD + jc] = make_double2(-xr * di, -xi * di);
        }
        __syncthreads();
    }
    // the dense products: entry e = lane + 64 c is (row e / NT, column e % NT)
    int ei[CE], ej[CE];
    bool ok[CE];
#pragma unroll
    for (int c = 0; c < CE; c++) {
        const int e = lane + kWave * c;
        ok[c] = e < NT * NT && e / NT < N && e % NT < N;
        ei[c] = ok[c] ? e / NT : 0;
        ej[c] = ok[c] ? e % NT : 0;
    }
#pragma unroll
    for (int c = 0; c < CE; c++) {                       // W[i][j] = sum_{k >= max(i,j)} conj(M[k][i]) M[k][j]  -> s.a (L is done with)
        const int i = ei[c], j = ej[c], top = i > j ? i : j;
        double wr = 0.0, wi = 0.0;
        for (int k = 0; k < N; k++) {
            const double2 x = s.m[k * LD + i], y = s.m[k * LD + j];
            if (k >= top) {
                wr = fma(x.x, y.x, fma(x.y, y.y, wr));
                wi = fma(x.x, y.y, fma(-x.y, y.x, wi));
            }
        }
        if (ok[c]) s.a[i * LD + j] = make_double2(wr, wi);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CE; c++) {                       // T = W (H / mu)  -> s.m (M is done with)
        const int i = ei[c], j = ej[c];
        double tr = 0.0, ti = 0.0;
        for (int k = 0; k < N; k++) {
            const double2 x = s.a[i * LD + k], y = s.h[k * LD + j];
            tr = fma(x.x, y.x, fma(-x.y, y.y, tr));
            ti = fma(x.x, y.y, fma(x.y, y.x, ti));
        }
        if (ok[c]) s.m[i * LD + j] = make_double2(tr, ti);
    }
    __syncthreads();
    double pr[CE], pi[CE];
#pragma unroll
    for (int c = 0; c < CE; c++) {                       // B = T W, kept in registers until every lane has read T
        const int i = ei[c], j = ej[c];
        double tr = 0.0, ti = 0.0;
        for (int k = 0; k < N; k++) {
            const double2 x = s.m[i * LD + k], y = s.a[k * LD + j];
            tr = fma(x.x, y.x, fma(-x.y, y.y, tr));
            ti = fma(x.x, y.y, fma(x.y, y.x, ti));
        }
        pr[c] = tr; pi[c] = ti;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CE; c++)
        if (ok[c]) s.m[ei[c] * LD + ej[c]] = make_double2(pr[c], pi[c]);
    __syncthreads();
    {   // the records: lanes 0..15 sum the diagonals of W (s.a), lanes 16..31 those of B (s.m); lane l takes u_l = sum_r X[r+l][r]
        const int l = lane & 15, which = (lane >> 4) & 1;
        const bool on = lane < 32 && l < N;
        const double2 *X = which ? s.m : s.a;
        double ur = 0.0, ui = 0.0;
        for (int r = 0; r < N; r++) {
            const bool in = on && r + l < N;
            const double2 x = X[in ? (r + l) * LD + r : 0];
            if (in) { ur += x.x; ui += x.y; }
        }
        if (on) {
            s.u[which][l] = make_double2(ur, (l == 0) ? 0.0 : ui);
            bad = bad || !(fma(ur, 0.0, ui * 0.0) == 0.0);
        }
    }
    __syncthreads();
}

struct IaaArgs {
    const float2 *R;
    const double2 *zd;
    float *spec, *power;
    int *status;
    double *p_dbg, *lag_dbg;
    double loading;
    int N, P, iterations;
};

template <int NT> __global__ __launch_bounds__(64) void iaa_wave_kernel(const IaaArgs g)
{
    constexpr int LD = IaaLds<NT>::LD;
    constexpr int CE = (NT * NT + kWave - 1) / kWave;
    __shared__ IaaLds<NT> s;
    const int lane = threadIdx.x, item = blockIdx.x;
    const int N = g.N, P = g.P;
    const float2 *__restrict__ Ri = g.R + (size_t)item * (N * N);

    double tr = 0.0;
    for (int i = 0; i < N; i++) tr += (double)Ri[i + i * N].x;
    const double mu = tr / (double)N;
    bool bad = !(mu > 0.0);
    const double rmu = 1.0 / mu;
    // H / mu from the upper triangle (row i, column j at [i + j N], i <= j) and the real part of the diagonal
#pragma unroll
    for (int c = 0; c < CE; c++) {
        const int e = lane + kWave * c;
        const int i = e / NT, j = e % NT;
        if (e < NT * NT && i < N && j < N) {
            const float2 x = (i <= j) ? Ri[i + j * N] : Ri[j + i * N];
            const double im = (i == j) ? 0.0 : (i < j) ? (double)x.y : -(double)x.y;
            s.h[i * LD + j] = make_double2((double)x.x * rmu, im * rmu);
        }
    }
    __syncthreads();
    if (lane < N) {                                      // the record of H / mu: u_l = sum_r (H / mu)[r+l][r]
        double ur = 0.0, ui = 0.0;
        for (int r = 0; r + lane < N; r++) {
            const double2 x = s.h[(r + lane) * LD + r];
            ur += x.x; ui += x.y;
        }
        s.u[0][lane] = make_double2(ur, (lane == 0) ? 0.0 : ui);
    }
    __syncthreads();

    const double inv_n2 = 1.0 / ((double)N * (double)N);
    iaa_sweep<NT, true>(s, g.zd, N, P, lane, inv_n2);
    for (int it = 1; it < g.iterations; it++) {
        iaa_factor<NT>(s, N, g.loading, lane, bad);
        iaa_sweep<NT, false>(s, g.zd, N, P, lane, inv_n2);
    }
    iaa_factor<NT>(s, N, g.loading, lane, bad);

    // the last records give the rows.  Pass 1 stores out = (float) p in the spectrum row and takes its maximum; pass 2, behind
    // the workgroup barrier that makes the stores visible, turns the row into dB against the maximum as the scan kernels do:
    // 0 dB exactly where out equals the maximum, an IEEE quotient everywhere else.
    float *__restrict__ srow = g.spec + (size_t)item * P;
    float *__restrict__ prow = g.power ? g.power + (size_t)item * P : nullptr;
    double *__restrict__ drow = g.p_dbg ? g.p_dbg + (size_t)item * P : nullptr;
    float mx = 0.0f;
    double fin = 0.0;
    for (int k0 = 0; k0 < P; k0 += kWave) {
        const int k = k0 + lane;
        const double2 z = g.zd[k < P ? k : P - 1];
        const double p = iaa_power<NT, false>(s.u[0], s.u[1], N, z.x, z.y, inv_n2);
        if (k < P) {
            const float out = (float)p;
            fin = fma(p, 0.0, fin);
            srow[k] = out;
            if (prow) prow[k] = (float)(mu * p);
            if (drow) drow[k] = p;
            mx = fmaxf(mx, out);
        }
    }
    bad = bad || !(fin == 0.0);
    bad = group_or<kWave>(bad ? 1 : 0, lane) != 0;
    mx = group_max<kWave, float>(mx, lane);
    __syncthreads();
    for (int k0 = 0; k0 < P; k0 += kWave) {
        const int k = k0 + lane;
        if (k < P) {
            const float out = srow[k];
            const float q = out / mx;
            float db = (out == mx) ? 0.0f : (q > 0.99999f) ? kIaaDbPerUnit * (q - 1.0f) : 10.0f * log10f(q);
            if (bad) db = NAN;
            srow[k] = db;
            if (bad && prow) prow[k] = NAN;
            if (bad && drow) drow[k] = (double)NAN;
        }
    }
    if (lane == 0 && g.status) g.status[item] = bad ? 1 : 0;
    if (g.lag_dbg && lane < N) {
        double *o = g.lag_dbg + (size_t)item * (2 * N) + 2 * lane;
        o[0] = bad ? (double)NAN : s.lag[lane].x;
        o[1] = bad ? (double)NAN : s.lag[lane].y;
    }
}

}  // namespace

int launch_iaa(int N, int P, int iterations, double loading, int n_items, const void *d_R, const void *d_zd, const IaaOut &out,
               hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    if (N < 2 || N > DOA_MAX_ANT_ELE || P < 1 || P > DOA_IAA_MAX_PSPECTRUM_LEN) {
        set_error("IAA: num_ant_ele=%d, pspectrum_len=%d outside the built range 2..%d, 1..%d", N, P, DOA_MAX_ANT_ELE,
                  DOA_IAA_MAX_PSPECTRUM_LEN);
        return DOA_ERR_UNSUPPORTED;
    }
    if (!d_R || !d_zd || !out.spec || iterations < 1 || iterations > DOA_IAA_MAX_ITERATIONS || !(loading >= 0.0) || !std::isfinite(loading)) {
        set_error("IAA: bad arguments of the launch (N=%d, iterations=%d, loading=%g)", N, iterations, loading);
        return DOA_ERR_INVALID_ARG;
    }
    IaaArgs g;
    g.R = (const float2 *)d_R; g.zd = (const double2 *)d_zd;
    g.spec = out.spec; g.power = out.power; g.status = out.status; g.p_dbg = out.p_dbg; g.lag_dbg = out.lag_dbg;
    g.loading = loading; g.N = N; g.P = P; g.iterations = iterations;
    const dim3 grid(n_items), block(kWave);
    if (N > 8) hipLaunchKernelGGL(iaa_wave_kernel<16>, grid, block, 0, st, g);
    else if (N > 4) hipLaunchKernelGGL(iaa_wave_kernel<8>, grid, block, 0, st, g);
    else hipLaunchKernelGGL(iaa_wave_kernel<4>, grid, block, 0, st, g);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

// ---- the C ABI of doa_iaa_lin_array (include/doa_hip.h) on the scaffold of block_host.hpp -----------------------------------
struct doa_iaa_lin_array : doa::BlockBase {
    int N = 0, P = 0, iterations = 0;
    double loading = 0.0;
    doa::MusicTables ula;             // its double phase table is the grid
    doa::DevBuf d_in, d_spec, d_power, d_status, d_p, d_lag;
};

namespace {

int iaa_args(const char *who, const doa_iaa_lin_array *h, int n, std::initializer_list<const void *> required, int min_n = 0)
{
    if (int rc = doa::work_args(who, h, n, required, min_n); rc != DOA_OK) return rc;
    return doa::need_bits64(who, h->bits, "the IAA kernel");
}

int iaa_launch(doa_iaa_lin_array *h, int n, const void *d_cov, const doa::IaaOut &out, hipStream_t st)
{
    return doa::launch_iaa(h->N, h->P, h->iterations, h->loading, n, d_cov, h->ula.d_zd.p, out, st);
}

}  // namespace

extern "C" {

doa_iaa_lin_array_t *doa_iaa_lin_array_create(float norm_spacing, int num_ant_ele, int pspectrum_len, float diagonal_loading,
                                              int iterations)
{
    doa::clear_error();
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("iaa_lin_array: need 2 <= num_ant_ele <= %d (got %d)", DOA_MAX_ANT_ELE, num_ant_ele);
        return nullptr;
    }
    if (!(norm_spacing > 0.0f) || norm_spacing > 0.5f) {
        doa::set_error("iaa_lin_array: need 0 < norm_spacing <= 0.5 (got %g)", (double)norm_spacing);
        return nullptr;
    }
    if (pspectrum_len < 1 || pspectrum_len > DOA_IAA_MAX_PSPECTRUM_LEN) {
        doa::set_error("iaa_lin_array: need 1 <= pspectrum_len <= %d (got %d)", DOA_IAA_MAX_PSPECTRUM_LEN, pspectrum_len);
        return nullptr;
    }
    if (!std::isfinite(diagonal_loading) || !(diagonal_loading >= 0.0f)) {
        doa::set_error("iaa_lin_array: diagonal_loading must be finite and >= 0 (got %g)", (double)diagonal_loading);
        return nullptr;
    }
    if (iterations < 1 || iterations > DOA_IAA_MAX_ITERATIONS) {
        doa::set_error("iaa_lin_array: need 1 <= iterations <= %d (got %d)", DOA_IAA_MAX_ITERATIONS, iterations);
        return nullptr;
    }
    return doa::create_block<doa_iaa_lin_array>("iaa_lin_array", [&](doa_iaa_lin_array &h) {
        h.N = num_ant_ele; h.P = pspectrum_len; h.iterations = iterations; h.loading = (double)diagonal_loading;
        return h.ula.build(norm_spacing, 1, num_ant_ele, pspectrum_len);
    });
}

void doa_iaa_lin_array_destroy(doa_iaa_lin_array_t *h) { doa::destroy_block(h); }
long long doa_iaa_lin_array_items_total(const doa_iaa_lin_array_t *h) { return h ? h->items_total : 0; }

int doa_iaa_lin_array_work_dev(doa_iaa_lin_array_t *h, int noutput_items, const void *d_cov_items, void *d_spectrum_out,
                               void *d_power_out, void *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = iaa_args("iaa_lin_array_work_dev", h, noutput_items, {d_cov_items, d_spectrum_out}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int rc = doa::bind_device(h->device); rc != DOA_OK) return rc;
    doa::IaaOut out;
    out.spec = (float *)d_spectrum_out; out.power = (float *)d_power_out; out.status = (int *)d_status_out;
    if (int rc = iaa_launch(h, noutput_items, d_cov_items, out, static_cast<hipStream_t>(hip_stream)); rc != DOA_OK) return rc;
    h->items_total += noutput_items;
    return noutput_items;
}

int doa_iaa_lin_array_work(doa_iaa_lin_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out, void *power_out,
                           void *status_out)
{
    doa::clear_error();
    if (int rc = iaa_args("iaa_lin_array_work", h, noutput_items, {cov_items, spectrum_out}); rc != DOA_OK) return rc;
    const int n = noutput_items;
    if (n == 0) return 0;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, (size_t)n * h->N * h->N * sizeof(float2));
    io.out(h->d_spec, spectrum_out, (size_t)n * h->P * sizeof(float));
    if (power_out) io.out(h->d_power, power_out, (size_t)n * h->P * sizeof(float));
    if (status_out) io.out(h->d_status, status_out, (size_t)n * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = doa_iaa_lin_array_work_dev(h, n, h->d_in.p, h->d_spec.p, power_out ? h->d_power.p : nullptr,
                                        status_out ? h->d_status.p : nullptr, h->stream);
    return io.finish(rc);
}

int doa_iaa_lin_array_debug(doa_iaa_lin_array_t *h, int noutput_items, const void *cov_items, void *power_out, void *lags_out)
{
    doa::clear_error();
    if (int rc = iaa_args("iaa_lin_array_debug", h, noutput_items, {cov_items}, 1); rc != DOA_OK) return rc;
    const int n = noutput_items;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, (size_t)n * h->N * h->N * sizeof(float2));
    io.out(h->d_spec, nullptr, (size_t)n * h->P * sizeof(float));
    io.out(h->d_p, power_out, (size_t)n * h->P * sizeof(double));
    io.out(h->d_lag, lags_out, (size_t)n * 2 * h->N * sizeof(double));
    int rc = io.status();
    if (rc == DOA_OK) {
        doa::IaaOut out;
        out.spec = h->d_spec.as<float>(); out.p_dbg = h->d_p.as<double>(); out.lag_dbg = h->d_lag.as<double>();
        rc = iaa_launch(h, n, h->d_in.p, out, h->stream);
    }
    return io.finish(rc == DOA_OK ? n : rc);
}

}  // extern "C"
