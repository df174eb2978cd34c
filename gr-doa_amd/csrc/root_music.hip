// root_music.hip — K6: Root-MUSIC for a uniform linear array on gfx950.
//
// Replaces gr::doa::rootMUSIC_linear_array (reference lib/rootMUSIC_linear_array_impl.cc:46-152):
//   EVD + noise projector as MUSIC (:108-116; here K2+K3 of music.hip), then
//   u[k], k = 0..2N-2: sums of the diagonals of P_N (:68-79), roots of sum_k u[k] z^k — the
//   reference gets them as eigenvalues of the Frobenius companion matrix through LAPACK cgeev
//   (:80-86) — keep the roots strictly inside the unit circle (:122-127), take the num_targets
//   closest to it (:131-141), angle = acos(arg(z) / (2 pi d)) in degrees, sorted ascending (:144).
//
// Here the roots come from a batched Aberth-Ehrlich iteration in double, one root per lane (the
// polynomial has degree 2N-2 <= 30; root_music_group_kernel).  Root-MUSIC's root pairs
// (z, 1/conj(z)) sit within ~1e-4 of each other at the unit circle, which is why a float solver
// (the reference's cgeev) is itself only ~0.01 degree accurate; see DESIGN.md "parity".
// Edge cases follow the reference: with fewer than num_targets interior roots the missing slots
// come out as 90 degrees (arg(inf+0i) = 0, :135-141); with none, the reference raises inside
// Armadillo (index_min on an empty vector) — here the item's status word is set and its angles
// are NaN, and the host entry point returns DOA_ERR_NUMERIC.
#include "kernels.hpp"

#include <cstdlib>

namespace doa {

// |p(z)| <= kResidualFloor * (degree+1) * sum |c_m||z|^m counts as "zero to working precision" (16 eps)
constexpr double kResidualFloor = 16.0 * 2.220446049250313e-16;

// ---------------------------------------------------------------------------------------------
// Group-parallel Aberth-Ehrlich: GR lanes (the power of two >= 2N-2) share one item, one root per
// lane.  Every lane evaluates p and p' at its own root by Horner (the 2N-1 coefficients are held
// redundantly in registers, padded with zeros up to GR so the loop bounds are compile-time), reads
// the other roots with cross-lane fetches for the Aberth correction, and all roots move
// simultaneously.  The dependent chain per item is ~1/(2N-2) of the one-lane-per-item kernel's.
// ---------------------------------------------------------------------------------------------
// 1/x for a finite positive double well inside the exponent range: hardware seed + two Newton steps
// (what the compiler's IEEE division expands to, minus its scaling / fix-up instructions: ~6 instead
// of ~18 instructions, and one reciprocal serves both parts of a complex quotient)
__device__ __forceinline__ double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}

// How many angles an item wants (the pattern of find_local_max.hip's PeakFixedM / PeakCounts).  RootFixedM: the handle's
// num_targets for every item -- no code added, the kernels are the ones they were.  RootCounts: a count m_i per item read from
// an int32 array; items stay W = num_targets floats wide:
//   1 <= m_i <= min(W, N-1)  the first m_i slots as the fixed kernel writes them for M = m_i, slots m_i.. NaN, status 0 / 1
//   m_i == 0                 W NaN, status 0 -- decided from the count: the record of such an item (u_0 = N, u_l = 0: one root
//                            of multiplicity 2N-2 at 0) is never read and the iteration never runs on it
//   anything else            W NaN, status 2 ("no usable count"; the estimator's -1 among them)
// The count is range-checked where it is loaded (item_count); nothing but the checked value leaves that function, so no
// address and no loop bound is ever formed from a raw count.
struct RootFixedM {
    static constexpr bool kCounted = false;
    int M;
    __device__ __forceinline__ int width() const { return M; }
};
struct RootCounts {
    static constexpr bool kCounted = true;
    const int *counts;
    int W;
    __device__ __forceinline__ int width() const { return W; }
    // `item` is already clamped to 0..n_items-1.  Returns m_i (0 when there is nothing to find); code: the status of such an item
    __device__ __forceinline__ int item_count(int item, int N, int &code) const
    {
        const int c = counts[item];
        const int top = (W < N - 1) ? W : N - 1;
        const bool usable = (c >= 0) && (c <= top);
        code = usable ? 0 : 2;
        return usable ? c : 0;
    }
};

// Selection stage (reference lib/rootMUSIC_linear_array_impl.cc:122-145) on the GR lanes of one group, lane k holding
// root k (is_root: k < 2N-2): dist = 1 - |z| (:122), keep dist > 0 -- strictly inside (:125-127) --, num_targets times the
// interior root closest to the circle (index_min: ties -> the first, i.e. the lowest root index), angle =
// 180 acos(arg z / (2 pi d)) / pi (:135), a used root becomes inf + 0i with dist inf (:138-139) -- so once the interior
// roots are exhausted index_min lands on an inf entry, arg(inf + 0i) = 0 and the slot reads 90 degrees --, ascending
// sort (:144; NaN last).  No interior root at all: the reference raises inside arma::index_min; here NaN angles and
// status 1.  Shared by the solver kernel and by root_select_kernel (the selection on caller-supplied roots).
// Counted (Cnt = RootCounts): n_want = m, the group's checked count; code = its status when m == 0.  The groups of one wave then want
// different numbers of picks, and both loops below shuffle: they run to the WAVE-UNIFORM bound W with the effects of the
// steps j >= m predicated off (dist keeps its value, the rank ignores slot j), so every lane of the wave executes every
// shuffle -- no lane is ever read while it is switched off -- and every source lane (lane ^ m with m < GR, base + bk with
// bk < GR, base + j with j < W <= N-1 < GR) lies in the reading lane's own group.  Steps j < m see exactly the state the
// fixed kernel's steps see for M = m.
template <int GR, class Cnt>
__device__ __forceinline__ void root_select(double zr, double zi, bool is_root, int k, int base, int lane, int item,
                                            bool real_item, const Cnt cnt, int n_want, int code, double two_pi_d,
                                            float *__restrict__ out, int *__restrict__ status)
{
    const int M = cnt.width();
    // dist = 1 - |z|; keep dist > 0; the M smallest, one at a time (:122-141)
    double dist = is_root ? 1.0 - sqrt(zr * zr + zi * zi) : -1.0;
    if (!(dist > 0.0)) dist = -1.0;
    const unsigned long long inside_mask = __ballot(dist > 0.0);
    const int n_inside = __popcll((inside_mask >> base) & ((GR == 64) ? ~0ull : ((1ull << GR) - 1ull)));
    float my_aoa = 0.f;
    for (int j = 0; j < M; j++) {
        // group arg-min of dist over the remaining interior roots (ties -> lowest lane)
        double bd = (dist > 0.0) ? dist : 1e300;
        int bk = (dist > 0.0) ? k : GR;
#pragma unroll
        for (int m = 1; m < GR; m <<= 1) {
            const double od = __shfl(bd, lane ^ m, kWave);
            const int ok = __shfl(bk, lane ^ m, kWave);
            if (od < bd || (od == bd && ok < bk)) { bd = od; bk = ok; }
        }
        double ang = 0.0;                                   // exhausted: arg(inf + 0i) = 0 -> 90 degrees
        if (bk < GR) {
            const double br = __shfl(zr, base + bk, kWave), bi = __shfl(zi, base + bk, kWave);
            ang = atan2(bi, br);
            if constexpr (Cnt::kCounted) { if (k == bk && j < n_want) dist = -1.0; }
            else { if (k == bk) dist = -1.0; }
        }
        const float a = (float)(180.0 * acos(ang / two_pi_d) / M_PI);
        if (k == j) my_aoa = a;
    }
    // ascending sort of the M picks held by lanes 0..M-1 (NaN sorts last)
    const float key = (my_aoa != my_aoa) ? INFINITY : my_aoa;
    int rank = 0;
    for (int j = 0; j < M; j++) {
        const float kj = __shfl(key, base + j, kWave);
        if constexpr (Cnt::kCounted) rank += (j < n_want && (kj < key || (kj == key && j < k))) ? 1 : 0;
        else rank += (kj < key || (kj == key && j < k)) ? 1 : 0;
    }
    if constexpr (Cnt::kCounted) {
        if (real_item) {
            float *o = out + (size_t)item * M;
            const bool found = (n_want > 0) && (n_inside != 0);
            // lanes n_want..W-1 (all W of them when nothing was found): NaN; lanes 0..n_want-1: their pick at its rank < n_want
            if (k < M && (k >= n_want || !found)) o[k] = __builtin_nanf("");
            if (k < n_want && found) o[rank] = my_aoa;
            if (k == 0 && status) status[item] = (n_want > 0) ? (found ? 0 : 1) : code;
        }
    } else if (real_item) {
        float *o = out + (size_t)item * M;
        if (n_inside == 0) {
            if (k < M) o[k] = __builtin_nanf("");
            if (k == 0 && status) status[item] = 1;
        } else {
            if (k < M) o[rank] = my_aoa;
            if (k == 0 && status) status[item] = 0;
        }
    }
}

// DEG = compile-time polynomial degree when it is known to be below GR (N = 4: degree 6 on 8 lanes),
// so that neither the Horner recurrence nor the root-pair loop spends steps on padding.
// Counted (Cnt = RootCounts): a group whose checked count is 0 (a zero count, or no usable one) has is_root = false in all its
// lanes and all-zero coefficients -- its record is not read --, so its p, p' and steps are finite, its rel is 0 in the float
// and in the double phase, and the wave leaves the loops as soon as the groups that do have roots to find are done; no
// cross-lane fetch leaves a group, so nothing of one group reaches another.
template <int GR, int DEG = GR, bool FLOAT_PHASE = true, class Cnt = RootFixedM>
__global__ __launch_bounds__(64) void root_music_group_kernel(const double *__restrict__ coef, float *__restrict__ out,
                                                              int *__restrict__ status, int n_items, int N, const Cnt cnt,
                                                              double two_pi_d, double2 *__restrict__ roots_out,
                                                              int float_iters, float float_tol2)
{
    constexpr int IPW = kWave / GR;
    const int lane = threadIdx.x & (kWave - 1);
    const int k = lane % GR, base = lane - k;
    int item = blockIdx.x * IPW + lane / GR;
    const bool real_item = item < n_items;
    if (!real_item) item = n_items - 1;
    const int D = 2 * N - 2;
    int n_want = 0, code = 0;                             // (counted form only)
    bool is_root = k < D;
    if constexpr (Cnt::kCounted) {
        n_want = cnt.item_count(item, N, code);
        is_root = is_root && (n_want > 0);
    }
    const double *co = coef + (size_t)item * (2 * N);
    // polynomial c[m], m = 0..D: c[N-1-l] = u_l, c[N-1+l] = conj(u_l); zero above D
    double cr[GR + 1], ci[GR + 1], ca[GR + 1];
#pragma unroll
    for (int m = 0; m <= GR; m++) {
        double vr = 0.0, vi = 0.0;
        bool have = (m <= D);
        if constexpr (Cnt::kCounted) have = have && (n_want > 0);
        if (have) {
            const int l = (m <= N - 1) ? (N - 1 - m) : (m - (N - 1));
            if (l == 0) vr = co[0];
            else { vr = co[2 * l - 1]; vi = (m < N - 1) ? co[2 * l] : -co[2 * l]; }
        }
        cr[m] = vr; ci[m] = vi; ca[m] = fabs(vr) + fabs(vi);
    }
    double zr, zi;
    {
        const double ang = 2.0 * M_PI * (k + 0.37) / D;
        const double rad = 0.75 + 0.5 * ((k * 0.6180339887498949) - floor(k * 0.6180339887498949));
        double sn, cs;
        sincos(ang, &sn, &cs);
        zr = is_root ? rad * cs : 1e6 * (k + 1);          // idle lanes park far away and never move
        zi = is_root ? rad * sn : 0.0;
    }
    if constexpr (FLOAT_PHASE) {
        // Round 4: the first iterations in FLOAT.  This kernel is one dependent chain per wave (512 waves on 1024 SIMDs), so
        // what an iteration costs is the latency of its instructions, and most of the 10-13 iterations only carry the roots from
        // the generic starting points into their basins: the same Aberth step on float copies of the coefficients (one
        // v_rcp_f32 per quotient instead of a seed and two Newton steps in double) until the steps are at float's own floor --
        // relative 1e-5, or 12 iterations --, then the double iteration below with its residual-based stopping test, unchanged,
        // which needs two or three more steps from there (cubic convergence).  What comes out has passed exactly the test it
        // passed before; the roots of a pair z, 1/conj(z), 1e-3..1e-5 apart, are told apart by float well enough to start from.
        float fzr = (float)zr, fzi = (float)zi;
        float fcr[DEG + 1], fci[DEG + 1];
        {
            // scale by the largest coefficient: float has the range, this keeps p and p' O(1)
            double mx = 0.0;
#pragma unroll
            for (int m = 0; m <= DEG; m++) mx = fmax(mx, ca[m]);
            const double inv = (mx > 0.0 && mx < 1e300) ? 1.0 / mx : 1.0;
#pragma unroll
            for (int m = 0; m <= DEG; m++) { fcr[m] = (float)(cr[m] * inv); fci[m] = (float)(ci[m] * inv); }
        }
        for (int it = 0; it < float_iters; it++) {
            float pr = 0.f, pi = 0.f, dr = 0.f, di = 0.f;
#pragma unroll
            for (int m = DEG; m >= 0; m--) {
                const float ndr = fmaf(dr, fzr, fmaf(-di, fzi, pr));
                const float ndi = fmaf(dr, fzi, fmaf(di, fzr, pi));
                dr = ndr; di = ndi;
                const float npr = fmaf(pr, fzr, fmaf(-pi, fzi, fcr[m]));
                const float npi = fmaf(pr, fzi, fmaf(pi, fzr, fci[m]));
                pr = npr; pi = npi;
            }
            const float dn = fmaf(dr, dr, di * di);
            float wr = 1e-3f, wi = 1e-3f;
            if (dn > 0.f) { const float inv = __builtin_amdgcn_rcpf(dn); wr = (pr * dr + pi * di) * inv; wi = (pi * dr - pr * di) * inv; }
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int j = 0; j < DEG; j++) {
                const float ojr = __shfl(fzr, base + j, kWave), oji = __shfl(fzi, base + j, kWave);
                const float er = fzr - ojr, ei = fzi - oji;
                const float en = fmaf(er, er, ei * ei);
                if (j != k && j < D && en > 0.f) { const float inv = __builtin_amdgcn_rcpf(en); sr = fmaf(er, inv, sr); si = fmaf(-ei, inv, si); }
            }
            const float qr = 1.f - (wr * sr - wi * si), qi = -(wr * si + wi * sr);
            const float qn = fmaf(qr, qr, qi * qi);
            float er = wr, ei = wi;
            if (qn > 0.f) { const float inv = __builtin_amdgcn_rcpf(qn); er = (wr * qr + wi * qi) * inv; ei = (wi * qr - wr * qi) * inv; }
            float rel = 0.f;
            const bool finite_step = (er == er) && (ei == ei) && (fabsf(er) < 1e30f) && (fabsf(ei) < 1e30f);
            if (is_root && finite_step) {
                fzr -= er; fzi -= ei;
                rel = (er * er + ei * ei) / (1.f + fzr * fzr + fzi * fzi);
            }
            if (__ballot(rel >= float_tol2) == 0ull) break;  // (squared relative step)
        }
        // a float phase that went astray (overflow, NaN) hands back the generic starting point
        const bool sane = (fzr == fzr) && (fzi == fzi) && (fabsf(fzr) < 1e6f) && (fabsf(fzi) < 1e6f);
        if (is_root && sane) { zr = (double)fzr; zi = (double)fzi; }
        // two lanes on the SAME float (the two roots of a pair, unresolved): the repulsion term between them would be
        // skipped (distance 0) and they would travel together for good; the later one steps aside by 1e-4
        bool twin = false;
#pragma unroll
        for (int j = 0; j < DEG; j++) {
            const double ojr = __shfl(zr, base + j, kWave), oji = __shfl(zi, base + j, kWave);
            twin = twin || (j < k && j < D && ojr == zr && oji == zi);
        }
        if (is_root && twin) { zr += 1e-4 * (k + 1); zi -= 0.7e-4 * (k + 1); }
    }
    for (int it = 0; it < 80; it++) {
        double pr = 0.0, pi = 0.0, dr = 0.0, di = 0.0, eb = 0.0;
        const double rk = (double)sqrtf((float)(zr * zr + zi * zi));
#pragma unroll
        for (int m = DEG; m >= 0; m--) {
            const double ndr = dr * zr - di * zi + pr;
            const double ndi = dr * zi + di * zr + pi;
            dr = ndr; di = ndi;
            const double npr = pr * zr - pi * zi + cr[m];
            const double npi = pr * zi + pi * zr + ci[m];
            pr = npr; pi = npi;
            eb = fma(eb, rk, ca[m]);             // rounding-error bound of p(z): sum |c_m| |z|^m
        }
        const double floor_k = kResidualFloor * (D + 1) * eb;
        const bool at_floor = (pr * pr + pi * pi <= floor_k * floor_k);
        // (coefficients above degree D are zero, so starting the recurrence at DEG >= D changes nothing)
        const double dn = dr * dr + di * di;
        double wr = 1e-3, wi = 1e-3;
        if (dn > 0.0) { const double inv = fast_rcp(dn); wr = (pr * dr + pi * di) * inv; wi = (pi * dr - pr * di) * inv; }
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int j = 0; j < DEG; j++) {
            const double ojr = __shfl(zr, base + j, kWave), oji = __shfl(zi, base + j, kWave);
            const double er = zr - ojr, ei = zi - oji;
            const double en = er * er + ei * ei;
            if (j != k && j < D && en > 0.0) { const double inv = fast_rcp(en); sr = fma(er, inv, sr); si = fma(-ei, inv, si); }
        }
        const double qr = 1.0 - (wr * sr - wi * si), qi = -(wr * si + wi * sr);
        const double qn = qr * qr + qi * qi;
        double er = wr, ei = wi;
        if (qn > 0.0) { const double inv = fast_rcp(qn); er = (wr * qr + wi * qi) * inv; ei = (wi * qr - wr * qi) * inv; }
        double rel = 0.0;
        if (is_root && !at_floor) {
            zr -= er; zi -= ei;
            rel = (er * er + ei * ei) / (1.0 + zr * zr + zi * zi);
        }
        if (__ballot(rel >= 1e-29) == 0ull) break;   // every root of every group of the wave has converged
    }
    {
        // a non-finite polynomial (non-finite covariance item) has no roots: without this the iteration above stops at
        // once -- every comparison with NaN is false -- and the starting points would pass for roots
        double csum = 0.0;
#pragma unroll
        for (int m = 0; m <= GR; m++) csum += ca[m];
        if (!(csum < INFINITY)) { zr = __builtin_nan(""); zi = __builtin_nan(""); }
    }
    if constexpr (Cnt::kCounted) {                        // diagnostics; an item without roots to find: NaN
        if (roots_out && real_item && k < D)
            roots_out[(size_t)item * D + k] = is_root ? make_double2(zr, zi) : make_double2(__builtin_nan(""), __builtin_nan(""));
    } else {
    if (roots_out && real_item && is_root) roots_out[(size_t)item * D + k] = make_double2(zr, zi);    // diagnostics
    }
    root_select<GR, Cnt>(zr, zi, is_root, k, base, lane, item, real_item, cnt, n_want, code, two_pi_d, out, status);
}

template <int GR, int DEG = GR>
static void launch_root_group(int N, int M, int n_items, const void *d_coef, void *d_out, void *d_status, double two_pi_d,
                              hipStream_t st, void *d_roots, const void *d_counts = nullptr)
{
    constexpr int IPW = kWave / GR;
    dim3 block(64), grid((n_items + IPW - 1) / IPW);
    // float phase: at most kFloatIters iterations, left as soon as every root of the wave moves by less than 1e-3 relative
    // (profiles/r04_lab_root_float_phase.txt has the sweep behind the two numbers)
    const int float_iters = DOA_LAB_ENV_INT("DOA_ROOT_FLOAT_ITERS", 12);
    const float float_tol2 = exp2f(-(float)DOA_LAB_ENV_INT("DOA_ROOT_FLOAT_TOL_LOG2", 33));      // 2^-33 = (1.1e-5)^2
    if (d_counts) {                                       // a count per item, items M floats wide (always the float phase)
        hipLaunchKernelGGL((root_music_group_kernel<GR, DEG, true, RootCounts>), grid, block, 0, st, (const double *)d_coef,
                           (float *)d_out, (int *)d_status, n_items, N, RootCounts{(const int *)d_counts, M}, two_pi_d,
                           (double2 *)d_roots, float_iters, float_tol2);
        return;
    }
    if (DOA_LAB_ENV_INT("DOA_ROOT_FLOAT_PHASE", 1))
        hipLaunchKernelGGL((root_music_group_kernel<GR, DEG, true>), grid, block, 0, st, (const double *)d_coef, (float *)d_out,
                           (int *)d_status, n_items, N, RootFixedM{M}, two_pi_d, (double2 *)d_roots, float_iters, float_tol2);
#ifdef DOA_LAB
    else
        hipLaunchKernelGGL((root_music_group_kernel<GR, DEG, false>), grid, block, 0, st, (const double *)d_coef, (float *)d_out,
                           (int *)d_status, n_items, N, RootFixedM{M}, two_pi_d, (double2 *)d_roots, 0, 0.f);
#endif
}

static int launch_root_any(int N, int M, float norm_spacing, int n_items, const void *d_coef, const void *d_counts, void *d_out,
                           void *d_status, hipStream_t st, void *d_roots)
{
    if (n_items <= 0) return DOA_OK;
    const double two_pi_d = 2 * M_PI * (double)norm_spacing;   // 2*datum::pi*d_norm_spacing, float promoted (:135)
    if (N < 2 || N > DOA_MAX_ANT_ELE) {
        set_error("rootMUSIC: num_ant_ele=%d outside the built range 2..%d", N, DOA_MAX_ANT_ELE);
        return DOA_ERR_UNSUPPORTED;
    }
    const int D = 2 * N - 2;
    if (D <= 2) launch_root_group<2>(N, M, n_items, d_coef, d_out, d_status, two_pi_d, st, d_roots, d_counts);
    else if (D <= 4) launch_root_group<4>(N, M, n_items, d_coef, d_out, d_status, two_pi_d, st, d_roots, d_counts);
    else if (D == 6) launch_root_group<8, 6>(N, M, n_items, d_coef, d_out, d_status, two_pi_d, st, d_roots, d_counts);
    else if (D <= 8) launch_root_group<8>(N, M, n_items, d_coef, d_out, d_status, two_pi_d, st, d_roots, d_counts);
    else if (D <= 16) launch_root_group<16>(N, M, n_items, d_coef, d_out, d_status, two_pi_d, st, d_roots, d_counts);
    else launch_root_group<32>(N, M, n_items, d_coef, d_out, d_status, two_pi_d, st, d_roots, d_counts);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

int launch_root_music(int N, int M, float norm_spacing, int n_items, const void *d_coef, void *d_out, void *d_status,
                      hipStream_t st, void *d_roots)
{
    return launch_root_any(N, M, norm_spacing, n_items, d_coef, nullptr, d_out, d_status, st, d_roots);
}

int launch_root_music_counts(int N, int W, float norm_spacing, int n_items, const void *d_coef, const void *d_counts, void *d_out,
                             void *d_status, hipStream_t st, void *d_roots)
{
    if (n_items > 0 && (!d_counts || W < 1 || W > N - 1)) {
        set_error("rootMUSIC: per-item counts need the count array and 1 <= num_targets <= num_ant_ele - 1 (got %d, %d)", W, N);
        return DOA_ERR_INVALID_ARG;
    }
    return launch_root_any(N, W, norm_spacing, n_items, d_coef, d_counts, d_out, d_status, st, d_roots);
}

// The selection stage alone, on caller-supplied roots (diagnostics: doa_rootMUSIC_linear_array_select_debug): the same
// root_select<GR> instantiation the solver kernel of this array size ends in, fed from memory instead of from the
// Aberth iteration, so every branch of the rule can be driven with hand-made root lists.
template <int GR, class Cnt = RootFixedM>
__global__ __launch_bounds__(64) void root_select_kernel(const double2 *__restrict__ roots, float *__restrict__ out,
                                                         int *__restrict__ status, int n_items, int N, const Cnt cnt,
                                                         double two_pi_d)
{
    constexpr int IPW = kWave / GR;
    const int lane = threadIdx.x & (kWave - 1);
    const int k = lane % GR, base = lane - k;
    int item = blockIdx.x * IPW + lane / GR;
    const bool real_item = item < n_items;
    if (!real_item) item = n_items - 1;
    const int D = 2 * N - 2;
    int n_want = 0, code = 0;                             // (counted form only)
    bool is_root = k < D;
    if constexpr (Cnt::kCounted) {
        n_want = cnt.item_count(item, N, code);
        is_root = is_root && (n_want > 0);                // an item without roots to find: its roots are not read
    }
    double zr = 0.0, zi = 0.0;
    if (is_root) { const double2 z = roots[(size_t)item * D + k]; zr = z.x; zi = z.y; }
    root_select<GR, Cnt>(zr, zi, is_root, k, base, lane, item, real_item, cnt, n_want, code, two_pi_d, out, status);
}

// d_counts == NULL: num_targets = M for every item; else a count per item, items M floats wide
static int launch_root_select_any(int N, int M, float norm_spacing, int n_items, const void *d_roots, const void *d_counts,
                                  void *d_out, void *d_status, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    const double two_pi_d = 2 * M_PI * (double)norm_spacing;
    const int D = 2 * N - 2;
#define DOA_SELECT(GR_)                                                                                                       \
    do {                                                                                                                      \
        const dim3 grid_((n_items + kWave / GR_ - 1) / (kWave / GR_));                                                        \
        if (d_counts)                                                                                                         \
            hipLaunchKernelGGL((root_select_kernel<GR_, RootCounts>), grid_, dim3(64), 0, st, (const double2 *)d_roots,       \
                               (float *)d_out, (int *)d_status, n_items, N, RootCounts{(const int *)d_counts, M}, two_pi_d);  \
        else                                                                                                                  \
            hipLaunchKernelGGL((root_select_kernel<GR_>), grid_, dim3(64), 0, st, (const double2 *)d_roots, (float *)d_out,   \
                               (int *)d_status, n_items, N, RootFixedM{M}, two_pi_d);                                         \
    } while (0)
    if (D <= 2) DOA_SELECT(2);
    else if (D <= 4) DOA_SELECT(4);
    else if (D <= 8) DOA_SELECT(8);
    else if (D <= 16) DOA_SELECT(16);
    else DOA_SELECT(32);
#undef DOA_SELECT
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

int launch_root_select(int N, int M, float norm_spacing, int n_items, const void *d_roots, void *d_out, void *d_status,
                       hipStream_t st)
{
    return launch_root_select_any(N, M, norm_spacing, n_items, d_roots, nullptr, d_out, d_status, st);
}

int launch_root_select_counts(int N, int W, float norm_spacing, int n_items, const void *d_roots, const void *d_counts,
                              void *d_out, void *d_status, hipStream_t st)
{
    if (n_items > 0 && (!d_counts || W < 1 || W > N - 1)) {
        set_error("rootMUSIC: per-item counts need the count array and 1 <= num_targets <= num_ant_ele - 1 (got %d, %d)", W, N);
        return DOA_ERR_INVALID_ARG;
    }
    return launch_root_select_any(N, W, norm_spacing, n_items, d_roots, d_counts, d_out, d_status, st);
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"
#include "gridfree_chain.hpp"

struct doa_rootMUSIC_linear_array : doa::BlockBase {
    float norm_spacing = 0.f;
    int M = 0, N = 0;
    doa::DevBuf d_in, d_out, d_roots, d_counts;
    doa::GridfreeBufs rec;              // coefficient records and status words
    doa::PinnedBuf h_status;
    doa::GridfreeDesc desc() const { return {DOA_GRIDFREE_ROOT_MUSIC, N, M, norm_spacing, bits}; }
};

// the host entries' status scan after the synchronise (counted: gridfree_first_error)
static int root_status_scan(const doa_rootMUSIC_linear_array *h, int n, bool counted)
{
    const int bad = doa::gridfree_first_error(h->h_status.as<int>(), n, counted);
    if (bad < 0) return n;
    doa::set_error("rootMUSIC_linear_array: item %d has no root strictly inside the unit circle "
                   "(the reference raises in arma::index_min here)", bad);
    return DOA_ERR_NUMERIC;
}

// records for n items, then the chain on `st`; d_status: the caller's status words, or NULL for the handle's
static int root_run_dev(doa_rootMUSIC_linear_array_t *h, int n, const void *d_cov, const doa::EvdCounts *counts, void *d_angles,
                        void *d_status, hipStream_t st, void *d_roots = nullptr)
{
    const doa::GridfreeDesc d = h->desc();
    const doa::GridfreePlan plan = doa::gridfree_plan(d, counts != nullptr);
    if (int rc = h->rec.reserve(plan, (size_t)n, !d_status); rc != DOA_OK) return rc;
    const int rc = doa::gridfree_run(d, n, d_cov, counts, h->rec.view(plan), d_angles, d_status, st, d_roots);
    return rc == DOA_OK ? n : rc;
}

static int root_counts_args(const char *who, doa_rootMUSIC_linear_array_t *h, int n, const void *cov, const void *counts, const void *out)
{
    if (int rc = doa::work_args(who, h, n, {cov, counts, out}); rc != DOA_OK) return rc;
    return doa::need_bits64(who, h->bits, "per-item counts");
}

extern "C" {

doa_rootMUSIC_linear_array_t *doa_rootMUSIC_linear_array_create(float norm_spacing, int num_targets, int num_ant_ele)
{
    doa::clear_error();
    // grc/doa_rootMUSIC_linear_array.xml:28-30
    if (num_ant_ele <= 0 || num_targets <= 0 || num_targets >= num_ant_ele) {
        doa::set_error("rootMUSIC_linear_array: need 0 < num_targets < num_ant_ele (got %d, %d)", num_targets, num_ant_ele);
        return nullptr;
    }
    if (!(norm_spacing > 0.0f) || norm_spacing > 0.5f) {
        doa::set_error("rootMUSIC_linear_array: need 0 < norm_spacing <= 0.5 (got %g)", (double)norm_spacing);
        return nullptr;
    }
    if (num_ant_ele > DOA_MAX_ANT_ELE || num_targets > DOA_MAX_PEAKS) {
        doa::set_error("rootMUSIC_linear_array: num_ant_ele=%d / num_targets=%d exceed the built caps (%d / %d)",
                       num_ant_ele, num_targets, DOA_MAX_ANT_ELE, DOA_MAX_PEAKS);
        return nullptr;
    }
    return doa::create_block<doa_rootMUSIC_linear_array>("rootMUSIC_linear_array", [&](doa_rootMUSIC_linear_array &h) {
        h.norm_spacing = norm_spacing; h.M = num_targets; h.N = num_ant_ele;
        return DOA_OK;
    });
}

void doa_rootMUSIC_linear_array_destroy(doa_rootMUSIC_linear_array_t *h) { doa::destroy_block(h); }

int doa_rootMUSIC_linear_array_work_dev(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *d_input_items0,
                                        void *d_output_items0, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("rootMUSIC_linear_array_work_dev", h, noutput_items, {d_input_items0, d_output_items0}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    return root_run_dev(h, noutput_items, d_input_items0, nullptr, d_output_items0, nullptr, static_cast<hipStream_t>(hip_stream));
}

int doa_rootMUSIC_linear_array_work(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *input_items0,
                                    void *output_items0)
{
    doa::clear_error();
    if (int rc = doa::work_args("rootMUSIC_linear_array_work", h, noutput_items, {input_items0, output_items0}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    const size_t st_bytes = (size_t)noutput_items * sizeof(int);
    doa::HostCall io(*h);
    int rc = io.status();
    if (rc == DOA_OK) rc = h->h_status.reserve(st_bytes);
    if (rc != DOA_OK) return rc;                         // nothing is queued yet
    io.in(h->d_in, input_items0, (size_t)noutput_items * h->N * h->N * sizeof(float2));
    io.out(h->d_out, output_items0, (size_t)noutput_items * h->M * sizeof(float));
    io.out(h->rec.status, h->h_status.p, st_bytes);
    rc = io.status();
    if (rc == DOA_OK) rc = doa_rootMUSIC_linear_array_work_dev(h, noutput_items, h->d_in.p, h->d_out.p, h->stream);
    rc = io.finish(rc);
    return rc < 0 ? rc : root_status_scan(h, noutput_items, false);
}

int doa_rootMUSIC_linear_array_work_dev_counts(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *d_cov_items,
                                               const void *d_counts, void *d_angles_out, int *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = root_counts_args("rootMUSIC_linear_array_work_dev_counts", h, noutput_items, d_cov_items, d_counts, d_angles_out); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    // forced-count mode
    const doa::EvdCounts counts = doa::evd_counts_forced((const int *)d_counts);
    return root_run_dev(h, noutput_items, d_cov_items, &counts, d_angles_out, d_status_out, static_cast<hipStream_t>(hip_stream));
}

int doa_rootMUSIC_linear_array_work_counts(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *cov_items,
                                           const void *counts, void *angles_out)
{
    doa::clear_error();
    if (int rc = root_counts_args("rootMUSIC_linear_array_work_counts", h, noutput_items, cov_items, counts, angles_out); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    const size_t cnt_bytes = (size_t)noutput_items * sizeof(int);
    doa::HostCall io(*h);
    int rc = io.status();
    if (rc == DOA_OK) rc = h->h_status.reserve(cnt_bytes);
    if (rc != DOA_OK) return rc;                         // nothing is queued yet
    io.in(h->d_in, cov_items, (size_t)noutput_items * h->N * h->N * sizeof(float2));
    io.in(h->d_counts, counts, cnt_bytes);
    io.out(h->d_out, angles_out, (size_t)noutput_items * h->M * sizeof(float));
    io.out(h->rec.status, h->h_status.p, cnt_bytes);
    rc = io.status();
    if (rc == DOA_OK)
        rc = doa_rootMUSIC_linear_array_work_dev_counts(h, noutput_items, h->d_in.p, h->d_counts.p, h->d_out.p, nullptr, h->stream);
    rc = io.finish(rc);
    return rc < 0 ? rc : root_status_scan(h, noutput_items, true);
}

int doa_rootMUSIC_linear_array_debug(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *input_items0,
                                     void *output_items0, void *roots_out, int *status_out)
{
    doa::clear_error();
    if (int rc = doa::work_args("rootMUSIC_linear_array_debug", h, noutput_items, {input_items0, output_items0}, 1); rc != DOA_OK) return rc;
    doa::HostCall io(*h);
    io.in(h->d_in, input_items0, (size_t)noutput_items * h->N * h->N * sizeof(float2));
    io.out(h->d_out, output_items0, (size_t)noutput_items * h->M * sizeof(float));
    io.out(h->d_roots, roots_out, (size_t)noutput_items * (2 * h->N - 2) * sizeof(double2));
    io.out(h->rec.status, status_out, (size_t)noutput_items * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK) rc = root_run_dev(h, noutput_items, h->d_in.p, nullptr, h->d_out.p, nullptr, h->stream, h->d_roots.p);
    return io.finish(rc);
}

// the two select entries: roots (and counts, or NULL) up, the selection kernel alone, angles and status down
static int root_select_debug(doa_rootMUSIC_linear_array_t *h, int n, const void *roots_in, const void *counts,
                             void *output_items0, int *status_out)
{
    doa::HostCall io(*h);
    io.in(h->d_roots, roots_in, (size_t)n * (2 * h->N - 2) * sizeof(double2));
    if (counts) io.in(h->d_counts, counts, (size_t)n * sizeof(int));
    io.out(h->d_out, output_items0, (size_t)n * h->M * sizeof(float));
    io.out(h->rec.status, status_out, (size_t)n * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = counts ? doa::launch_root_select_counts(h->N, h->M, h->norm_spacing, n, h->d_roots.p, h->d_counts.p, h->d_out.p,
                                                     h->rec.status.p, h->stream)
                    : doa::launch_root_select(h->N, h->M, h->norm_spacing, n, h->d_roots.p, h->d_out.p, h->rec.status.p, h->stream);
    return io.finish(rc == DOA_OK ? n : rc);
}

int doa_rootMUSIC_linear_array_select_debug(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *roots_in,
                                            void *output_items0, int *status_out)
{
    doa::clear_error();
    const char *who = "rootMUSIC_linear_array_select_debug";
    if (int rc = doa::work_args(who, h, noutput_items, {roots_in, output_items0}, 1); rc != DOA_OK) return rc;
    return root_select_debug(h, noutput_items, roots_in, nullptr, output_items0, status_out);
}

int doa_rootMUSIC_linear_array_select_counts_debug(doa_rootMUSIC_linear_array_t *h, int noutput_items, const void *roots_in,
                                                   const void *counts, void *output_items0, int *status_out)
{
    doa::clear_error();
    const char *who = "rootMUSIC_linear_array_select_counts_debug";
    if (int rc = doa::work_args(who, h, noutput_items, {roots_in, counts, output_items0}, 1); rc != DOA_OK) return rc;
    return root_select_debug(h, noutput_items, roots_in, counts, output_items0, status_out);
}

int doa_rootMUSIC_linear_array_set_internal_precision(doa_rootMUSIC_linear_array_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("rootMUSIC_linear_array_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
