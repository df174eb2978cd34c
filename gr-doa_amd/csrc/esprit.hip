// esprit.hip — least-squares ESPRIT for a uniform linear array on gfx950: esprit_kernel and the C ABI of
// doa_esprit_linear_array.  Not a block of the reference; the definition is stated once in include/doa_hip.h.
//
// The eigen stage (music_evd.hip: launch_music_evd_record / launch_music_evd_counts) leaves the SIGNAL-SUBSPACE RECORD of
// every item (kernels.hpp): its eigenvectors as columns by descending eigenvalue.  esprit_kernel takes the first m columns
// Es (N x m) and computes, per item, in double:
//     gamma = 1 - sum_k |Es[N-1][k]|^2,   F = Es1^H Es2,   Psi = F + e (e^H F) / gamma,   e = Es[N-1, :]^H
// (Sherman-Morrison on Es1^H Es1 = I - e e^H: no factorisation), the eigenvalues of Psi, the angles, sorted.
//   G lanes per item (4 for N <= 4, 8 for N <= 8, 16 for N <= 16), 64 / G items per wave, one wave per block.
//   Es and Psi live in LDS (a 15 x 15 complex double matrix does not fit one lane's registers, and its rows and columns are
//   addressed by run-time indices); lane j of a group owns COLUMN j of Psi in the steps that combine rows (forming F and
//   Psi, reflections and rotations from the left) and ROW j in the steps that combine columns (from the right), so every
//   step is lane-local between two barriers and there is no cross-lane reduction whose order could depend on the neighbours.
//   m = 1: lambda = Psi.  m = 2: the quadratic, the larger root first and the other from the determinant.
//   m >= 3: Householder reduction to Hessenberg form, then explicit Wilkinson-shifted QR steps (Givens) on the active
//   window with deflation, at most 30 m steps per item (status 3).
// Every loop that holds a barrier is wave-uniform (bounds from the launch's W, the per-item work under predicates); no lane
// returns before the end.  An item's result depends on nothing but the item and its count.
#include "kernels.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace doa {
namespace {

constexpr double kGammaMin = DOA_ESPRIT_GAMMA_MIN;
constexpr double kQrEps = 2.220446049250313e-16;      // 2^-52: a sub-diagonal entry below eps (|h_kk| + |h_k-1,k-1|) is zero

struct Cplx { double re, im; };
__device__ __forceinline__ Cplx cmul(Cplx a, Cplx b) { return {fma(a.re, b.re, -(a.im * b.im)), fma(a.re, b.im, a.im * b.re)}; }
__device__ __forceinline__ Cplx cmulc(Cplx a, Cplx b) { return {fma(a.re, b.re, a.im * b.im), fma(a.im, b.re, -(a.re * b.im))}; }   // a conj(b)
__device__ __forceinline__ double cabs1(Cplx a) { return fabs(a.re) + fabs(a.im); }
__device__ __forceinline__ Cplx cdiv(Cplx a, Cplx b)
{
    const double n = fma(b.re, b.re, b.im * b.im);
    const Cplx t = cmulc(a, b);
    return {t.re / n, t.im / n};
}
__device__ __forceinline__ Cplx csqrt_d(Cplx z)
{
    if (z.re == 0.0 && z.im == 0.0) return {0.0, 0.0};
    const double m = sqrt(fma(z.re, z.re, z.im * z.im));
    if (z.re >= 0.0) {
        const double t = sqrt(0.5 * (m + z.re));
        return {t, z.im / (2.0 * t)};
    }
    const double t = sqrt(0.5 * (m - z.re));
    return {fabs(z.im) / (2.0 * t), copysign(t, z.im)};
}
// the two eigenvalues of [[a, b], [c, d]]: h = (a - d) / 2, disc = sqrt(h^2 + b c); the root of larger modulus as the sum
// without cancellation, the other one from the determinant
__device__ __forceinline__ void eig2(Cplx a, Cplx b, Cplx c, Cplx d, Cplx &l1, Cplx &l2)
{
    const Cplx h = {0.5 * (a.re - d.re), 0.5 * (a.im - d.im)};
    const Cplx bc = cmul(b, c);
    const Cplx hh = cmul(h, h);
    Cplx disc = csqrt_d({hh.re + bc.re, hh.im + bc.im});
    const Cplx mean = {0.5 * (a.re + d.re), 0.5 * (a.im + d.im)};
    if (fma(mean.re, disc.re, mean.im * disc.im) < 0.0) { disc.re = -disc.re; disc.im = -disc.im; }
    l1 = {mean.re + disc.re, mean.im + disc.im};
    const Cplx ad = cmul(a, d);
    const Cplx det = {ad.re - bc.re, ad.im - bc.im};
    if (l1.re == 0.0 && l1.im == 0.0) l2 = {0.0, 0.0};
    else l2 = cdiv(det, l1);
}

template <int G>
__global__ __launch_bounds__(64) void esprit_kernel(const float2 *__restrict__ R, const double *__restrict__ rec,
                                                    const int *__restrict__ counts, float *__restrict__ out,
                                                    int *__restrict__ status, int n_items, int N, int W, double inv_two_pi_d)
{
    constexpr int IPW = kWave / G;                       // items per wave
    constexpr int MM = G - 1;                            // the largest m, and the leading dimension of Psi
    __shared__ double sEr[IPW][MM][G], sEi[IPW][MM][G];  // Es[row][k] at [k][row]
    __shared__ double sHr[IPW][MM * MM], sHi[IPW][MM * MM];      // Psi, then its Hessenberg / triangular form: [i * MM + j]
    __shared__ double sRot[IPW][MM][4];                  // the Givens rotations of one QR step: c.re, c.im, s.re, s.im
    __shared__ double sVr[IPW][MM], sVi[IPW][MM];        // the Householder vector of one reduction step
    const int lane = threadIdx.x & (kWave - 1);
    const int r = lane % G, base = lane - r, g = lane / G;
    int item = blockIdx.x * IPW + g;
    const bool real_item = item < n_items;
    if (!real_item) item = n_items - 1;                  // idle groups shadow the last item (no stores)

    // this item's count
    int m = W, st = 0;
    if (counts) {
        m = counts[item];
        const int top = (W < N - 1) ? W : N - 1;
        if (m < 0 || m > top) { st = 2; m = 0; }
    }
    double *hr = sHr[g], *hi = sHi[g];

    // the first m columns of the record; trace and finiteness of the item itself (upper triangle, real diagonal)
    {
        const double *rc = rec + (size_t)item * subspace_record_len(N);
#pragma unroll
        for (int k = 0; k < MM; k++)
            if (k < m && r < N) {
                const double2 x = *reinterpret_cast<const double2 *>(rc + 2 * ((size_t)k * N + r));
                sEr[g][k][r] = x.x; sEi[g][k][r] = x.y;
            }
    }
    double tr = 0.0, poison = 0.0;
    if (r < N && m > 0) {
        const float2 *Ri = R + (size_t)item * (N * N);
        for (int c = r; c < N; c++) {
            const float2 x = Ri[r + c * N];
            poison = fma((double)x.x, 0.0, poison);
            if (c != r) poison = fma((double)x.y, 0.0, poison);
            else tr = (double)x.x;
        }
    }
    tr = group_sum<G, double>(tr, lane);
    poison = group_sum<G, double>(poison, lane);
    __syncthreads();

    // gamma, F = Es1^H Es2 and Psi: lane j owns column j
    double s_last = 0.0;
    for (int k = 0; k < m; k++) s_last = fma(sEr[g][k][N - 1], sEr[g][k][N - 1], fma(sEi[g][k][N - 1], sEi[g][k][N - 1], s_last));
    const double gamma = 1.0 - s_last;
    if (m > 0 && (!(tr > 0.0) || !(poison == 0.0) || !(gamma > kGammaMin))) st = 1;
    const bool solve = (st == 0) && (m > 0);
    if (solve && r < m) {
        const int j = r;
        Cplx gj = {0.0, 0.0};
        for (int i = 0; i < m; i++) {
            Cplx f = {0.0, 0.0};
            for (int row = 0; row + 1 < N; row++) {      // conj(Es[row][i]) Es[row + 1][j]
                const double ar = sEr[g][i][row], ai = sEi[g][i][row], br = sEr[g][j][row + 1], bi = sEi[g][j][row + 1];
                f.re = fma(ar, br, fma(ai, bi, f.re));
                f.im = fma(ar, bi, fma(-ai, br, f.im));
            }
            hr[i * MM + j] = f.re; hi[i * MM + j] = f.im;
            const Cplx t = cmul({sEr[g][i][N - 1], sEi[g][i][N - 1]}, f);       // (e^H F)_j += Es[N-1][i] F[i][j]
            gj.re += t.re; gj.im += t.im;
        }
        gj.re /= gamma; gj.im /= gamma;
        for (int i = 0; i < m; i++) {                    // Psi[i][j] = F[i][j] + conj(Es[N-1][i]) (e^H F)_j / gamma
            const Cplx t = cmulc(gj, {sEr[g][i][N - 1], sEi[g][i][N - 1]});
            hr[i * MM + j] += t.re; hi[i * MM + j] += t.im;
        }
    }
    __syncthreads();

    // ---- m >= 3: Hessenberg form, then shifted QR --------------------------------------------------------------------------
    const bool iterate = solve && m >= 3;
    for (int c = 0; c + 2 < W; c++) {                    // Householder step c: zero Psi[c+2 .., c]
        const bool on = iterate && (c + 2 < m);
        {
            double tail2 = 0.0;
            for (int t = c + 2; t < m; t++)
                if (on) tail2 = fma(hr[t * MM + c], hr[t * MM + c], fma(hi[t * MM + c], hi[t * MM + c], tail2));
            const bool reflect = on && (tail2 > 0.0);
            Cplx v = {0.0, 0.0};
            if (reflect && r > c && r < m) {
                const Cplx x0 = {hr[(c + 1) * MM + c], hi[(c + 1) * MM + c]};
                const double a0 = sqrt(fma(x0.re, x0.re, x0.im * x0.im));
                const double xn = sqrt(fma(a0, a0, tail2));
                const double inv = 1.0 / sqrt(fma(a0 + xn, a0 + xn, tail2));
                if (r == c + 1) {                        // v_0 = x_0 + phase(x_0) ||x||
                    const double f = (a0 > 0.0) ? (a0 + xn) / a0 : 0.0;
                    v = (a0 > 0.0) ? Cplx{x0.re * f, x0.im * f} : Cplx{xn, 0.0};
                } else {
                    v = {hr[r * MM + c], hi[r * MM + c]};
                }
                v.re *= inv; v.im *= inv;
            }
            if (r < MM) { sVr[g][r] = v.re; sVi[g][r] = v.im; }
        }
        __syncthreads();
        if (on && r < m) {                               // from the left, column r: x -= 2 v (v^H x)
            Cplx w = {0.0, 0.0};
            for (int t = c + 1; t < m; t++) {
                const Cplx p = cmulc({hr[t * MM + r], hi[t * MM + r]}, {sVr[g][t], sVi[g][t]});
                w.re += p.re; w.im += p.im;
            }
            w.re *= 2.0; w.im *= 2.0;
            for (int t = c + 1; t < m; t++) {
                const Cplx p = cmul({sVr[g][t], sVi[g][t]}, w);
                hr[t * MM + r] -= p.re; hi[t * MM + r] -= p.im;
            }
        }
        __syncthreads();
        if (on && r < m) {                               // from the right, row r: y -= 2 (y v) v^H
            Cplx w = {0.0, 0.0};
            for (int t = c + 1; t < m; t++) {
                const Cplx p = cmul({hr[r * MM + t], hi[r * MM + t]}, {sVr[g][t], sVi[g][t]});
                w.re += p.re; w.im += p.im;
            }
            w.re *= 2.0; w.im *= 2.0;
            for (int t = c + 1; t < m; t++) {
                const Cplx p = cmulc(w, {sVr[g][t], sVi[g][t]});
                hr[r * MM + t] -= p.re; hi[r * MM + t] -= p.im;
            }
        }
        __syncthreads();
    }

    bool act = iterate;
    int top = m - 1;                                     // the active window ends here; rows above `top` are done
    int steps = 0, since = 0;
    while (__any(act)) {
        // deflation: the window's start `lo`, scanning up from `top`
        int lo = 0;
        if (act) {
            for (int k = top; k >= 1; k--) {
                const double sub = fabs(hr[k * MM + k - 1]) + fabs(hi[k * MM + k - 1]);
                const double dd = fabs(hr[k * MM + k]) + fabs(hi[k * MM + k]) + fabs(hr[(k - 1) * MM + k - 1]) + fabs(hi[(k - 1) * MM + k - 1]);
                if (sub <= kQrEps * dd) { lo = k; break; }
            }
            if (lo == top) {                             // Psi[top][top] is an eigenvalue
                top--; since = 0;
                if (top <= 0) act = false;
            }
        }
        const bool step = act && lo < top;
        Cplx mu = {0.0, 0.0};
        if (step) {
            const Cplx a = {hr[(top - 1) * MM + top - 1], hi[(top - 1) * MM + top - 1]}, b = {hr[(top - 1) * MM + top], hi[(top - 1) * MM + top]};
            const Cplx cc = {hr[top * MM + top - 1], hi[top * MM + top - 1]}, d = {hr[top * MM + top], hi[top * MM + top]};
            if (since == 10 || since == 20) {            // exceptional shift
                mu = {d.re + 0.75 * cabs1(cc), d.im};
            } else {                                     // Wilkinson: the eigenvalue of the trailing 2 x 2 block closer to d
                Cplx l1, l2;
                eig2(a, b, cc, d, l1, l2);
                const double d1 = cabs1({l1.re - d.re, l1.im - d.im}), d2 = cabs1({l2.re - d.re, l2.im - d.im});
                mu = (d1 <= d2) ? l1 : l2;
            }
        }
        __syncthreads();                                 // every lane has read the trailing block before its diagonal is shifted
        if (step && r >= lo && r <= top) { hr[r * MM + r] -= mu.re; hi[r * MM + r] -= mu.im; }       // own column
        // Q^H (Psi - mu I) = R: rotation k zeroes [k+1][k]; lane j applies it to column j
        for (int k = 0; k + 1 < W; k++) {
            const bool rot = step && k >= lo && k < top;
            if (rot && r == k) {
                const Cplx a = {hr[k * MM + k], hi[k * MM + k]}, b = {hr[(k + 1) * MM + k], hi[(k + 1) * MM + k]};
                const double nrm = sqrt(fma(a.re, a.re, fma(a.im, a.im, fma(b.re, b.re, b.im * b.im))));
                Cplx cs = {1.0, 0.0}, sn = {0.0, 0.0};
                if (nrm > 0.0) { cs = {a.re / nrm, a.im / nrm}; sn = {b.re / nrm, b.im / nrm}; }
                sRot[g][k][0] = cs.re; sRot[g][k][1] = cs.im; sRot[g][k][2] = sn.re; sRot[g][k][3] = sn.im;
                if (nrm > 0.0) { hr[k * MM + k] = nrm; hi[k * MM + k] = 0.0; }
                hr[(k + 1) * MM + k] = 0.0; hi[(k + 1) * MM + k] = 0.0;
            }
            __syncthreads();
            if (rot && r > k && r <= top) {              // rows (k, k+1) <- (conj(c) x + conj(s) y, -s x + c y)
                const Cplx cs = {sRot[g][k][0], sRot[g][k][1]}, sn = {sRot[g][k][2], sRot[g][k][3]};
                const Cplx x = {hr[k * MM + r], hi[k * MM + r]}, y = {hr[(k + 1) * MM + r], hi[(k + 1) * MM + r]};
                const Cplx p1 = cmulc(x, cs), p2 = cmulc(y, sn), p3 = cmul(sn, x), p4 = cmul(cs, y);
                hr[k * MM + r] = p1.re + p2.re; hi[k * MM + r] = p1.im + p2.im;
                hr[(k + 1) * MM + r] = p4.re - p3.re; hi[(k + 1) * MM + r] = p4.im - p3.im;
            }
        }
        __syncthreads();
        // R Q + mu I: lane i takes row i through the rotations that touch it (k >= i - 1)
        if (step && r >= lo && r <= top) {
            for (int k = (r - 1 > lo) ? r - 1 : lo; k < top; k++) {      // columns (k, k+1) <- (c x + s y, -conj(s) x + conj(c) y)
                const Cplx cs = {sRot[g][k][0], sRot[g][k][1]}, sn = {sRot[g][k][2], sRot[g][k][3]};
                const Cplx x = {hr[r * MM + k], hi[r * MM + k]}, y = {hr[r * MM + k + 1], hi[r * MM + k + 1]};
                const Cplx p1 = cmul(cs, x), p2 = cmul(sn, y), p3 = cmulc(x, sn), p4 = cmulc(y, cs);
                hr[r * MM + k] = p1.re + p2.re; hi[r * MM + k] = p1.im + p2.im;
                hr[r * MM + k + 1] = p4.re - p3.re; hi[r * MM + k + 1] = p4.im - p3.im;
            }
            hr[r * MM + r] += mu.re; hi[r * MM + r] += mu.im;
        }
        __syncthreads();
        if (step) {
            steps++; since++;
            if (steps >= 30 * m) { st = 3; act = false; }
        }
    }

    // ---- eigenvalue of lane r -> angle ---------------------------------------------------------------------------------------
    Cplx lam = {0.0, 0.0};
    if (st == 0 && m > 0) {
        if (m == 2) {
            Cplx l1, l2;
            eig2({hr[0], hi[0]}, {hr[1], hi[1]}, {hr[MM], hi[MM]}, {hr[MM + 1], hi[MM + 1]}, l1, l2);
            lam = (r == 0) ? l1 : l2;
        } else if (r < m) {
            lam = {hr[r * MM + r], hi[r * MM + r]};
        }
    }
    float ang = NAN;
    if (st == 0 && r < m) {
        const double cth = atan2(lam.im, lam.re) * inv_two_pi_d;
        ang = (fabs(cth) > 1.0) ? NAN : (float)(57.295779513082320877 * acos(cth));
    }
    const int filled = (st == 0) ? m : 0;
    // ascending, NaN last, equal keys in lane order
    int rank = 0;
#pragma unroll
    for (int j = 0; j < MM; j++) {
        const float aj = __shfl(ang, base + j, kWave);
        const bool nj = aj != aj, nr = ang != ang;
        const bool before = (!nj && (nr || aj < ang)) || (((nj && nr) || aj == ang) && j < r);
        rank += (j < filled && before) ? 1 : 0;
    }
    if (real_item) {
        float *o = out + (size_t)item * W;
        if (r < filled) o[rank] = ang;
        else if (r < W) o[r] = NAN;
        if (r == 0 && status) status[item] = st;
    }
}

template <int G>
void launch_esprit_g(int N, int W, double inv_two_pi_d, int n_items, const void *d_R, const void *d_rec, const void *d_counts,
                     void *d_out, void *d_status, hipStream_t st)
{
    constexpr int IPW = kWave / G;
    hipLaunchKernelGGL((esprit_kernel<G>), dim3((n_items + IPW - 1) / IPW), dim3(64), 0, st, (const float2 *)d_R, (const double *)d_rec,
                       (const int *)d_counts, (float *)d_out, (int *)d_status, n_items, N, W, inv_two_pi_d);
}

}  // namespace

int launch_esprit(int N, int W, float norm_spacing, int n_items, const void *d_R, const void *d_rec, const void *d_counts,
                  void *d_out, void *d_status, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    if (N < 2 || N > DOA_MAX_ANT_ELE) {
        set_error("ESPRIT: num_ant_ele=%d outside the built range 2..%d", N, DOA_MAX_ANT_ELE);
        return DOA_ERR_UNSUPPORTED;
    }
    if (!d_R || !d_rec || !d_out || W < 1 || W >= N || !(norm_spacing > 0.0f)) {
        set_error("ESPRIT: bad arguments of the launch (N=%d, num_targets=%d, norm_spacing=%g)", N, W, (double)norm_spacing);
        return DOA_ERR_INVALID_ARG;
    }
    const double inv_two_pi_d = 1.0 / (2.0 * 3.14159265358979323846 * (double)norm_spacing);
    if (N > 8) launch_esprit_g<16>(N, W, inv_two_pi_d, n_items, d_R, d_rec, d_counts, d_out, d_status, st);
    else if (N > 4) launch_esprit_g<8>(N, W, inv_two_pi_d, n_items, d_R, d_rec, d_counts, d_out, d_status, st);
    else launch_esprit_g<4>(N, W, inv_two_pi_d, n_items, d_R, d_rec, d_counts, d_out, d_status, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"
#include "gridfree_chain.hpp"

struct doa_esprit_linear_array : doa::BlockBase {      // bits: the work entries need 64
    float norm_spacing = 0.f;
    int M = 0, N = 0;
    doa::DevBuf d_in, d_out, d_status, d_counts;
    doa::GridfreeBufs rec;              // signal-subspace records (no status words of its own: a caller without a buffer gets none)
    doa::GridfreeDesc desc() const { return {DOA_GRIDFREE_ESPRIT, N, M, norm_spacing, bits}; }
};

static int esprit_work_args(const char *who, doa_esprit_linear_array_t *h, int n, const void *in, const void *out, bool counted,
                            const void *counts)
{
    if (int rc = doa::work_args(who, h, n, {in, out, counted ? counts : in}); rc != DOA_OK) return rc;
    return doa::need_bits64(who, h->bits, "ESPRIT");
}

// records for n items, then the chain on `st` (d_counts, optional: a count per item from the caller)
static int esprit_run_dev(doa_esprit_linear_array_t *h, int n, const void *d_cov, const void *d_counts, void *d_angles, void *d_status,
                          hipStream_t st)
{
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const doa::GridfreeDesc d = h->desc();
    const doa::EvdCounts counts = doa::evd_counts_forced((const int *)d_counts);
    const doa::GridfreePlan plan = doa::gridfree_plan(d, d_counts != nullptr);
    if (int rc = h->rec.reserve(plan, (size_t)n, false); rc != DOA_OK) return rc;
    const int rc = doa::gridfree_run(d, n, d_cov, d_counts ? &counts : nullptr, h->rec.view(plan), d_angles, d_status, st);
    return rc == DOA_OK ? n : rc;
}

static int esprit_run_host(doa_esprit_linear_array_t *h, int n, const void *cov, const void *counts, void *angles, void *status)
{
    doa::HostCall io(*h);
    io.in(h->d_in, cov, (size_t)n * h->N * h->N * sizeof(float2));
    if (counts) io.in(h->d_counts, counts, (size_t)n * sizeof(int));
    io.out(h->d_out, angles, (size_t)n * h->M * sizeof(float));
    io.out(h->d_status, status, (size_t)n * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK) rc = esprit_run_dev(h, n, h->d_in.p, counts ? h->d_counts.p : nullptr, h->d_out.p, h->d_status.p, h->stream);
    return io.finish(rc);
}

// the record entry: items, records (and counts, or NULL) up, esprit_kernel alone, angles and status down
static int esprit_record_debug(doa_esprit_linear_array_t *h, int n, const void *cov, const void *records, const void *counts,
                               void *angles, int *status)
{
    doa::HostCall io(*h);
    io.in(h->d_in, cov, (size_t)n * h->N * h->N * sizeof(float2));
    io.in(h->rec.rec, records, (size_t)n * doa::subspace_record_len(h->N) * sizeof(double));
    if (counts) io.in(h->d_counts, counts, (size_t)n * sizeof(int));
    io.out(h->d_out, angles, (size_t)n * h->M * sizeof(float));
    io.out(h->d_status, status, (size_t)n * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = doa::launch_esprit(h->N, h->M, h->norm_spacing, n, h->d_in.p, h->rec.rec.p, counts ? h->d_counts.p : nullptr, h->d_out.p,
                                h->d_status.p, h->stream);
    return io.finish(rc == DOA_OK ? n : rc);
}

extern "C" {

doa_esprit_linear_array_t *doa_esprit_linear_array_create(float norm_spacing, int num_targets, int num_ant_ele)
{
    doa::clear_error();
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("esprit_linear_array: need 2 <= num_ant_ele <= %d (got %d)", DOA_MAX_ANT_ELE, num_ant_ele);
        return nullptr;
    }
    if (num_targets < 1 || num_targets >= num_ant_ele) {
        doa::set_error("esprit_linear_array: need 1 <= num_targets < num_ant_ele (got %d, %d)", num_targets, num_ant_ele);
        return nullptr;
    }
    if (!(norm_spacing > 0.0f) || norm_spacing > 0.5f) {
        doa::set_error("esprit_linear_array: need 0 < norm_spacing <= 0.5 (got %g)", (double)norm_spacing);
        return nullptr;
    }
    return doa::create_block<doa_esprit_linear_array>("esprit_linear_array", [&](doa_esprit_linear_array &h) {
        h.norm_spacing = norm_spacing; h.M = num_targets; h.N = num_ant_ele;
        return DOA_OK;
    });
}

void doa_esprit_linear_array_destroy(doa_esprit_linear_array_t *h) { doa::destroy_block(h); }

int doa_esprit_linear_array_work_dev(doa_esprit_linear_array_t *h, int noutput_items, const void *d_cov_items, void *d_angles_out,
                                     void *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = esprit_work_args("esprit_linear_array_work_dev", h, noutput_items, d_cov_items, d_angles_out, false, nullptr); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    return esprit_run_dev(h, noutput_items, d_cov_items, nullptr, d_angles_out, d_status_out, static_cast<hipStream_t>(hip_stream));
}

int doa_esprit_linear_array_work_dev_counts(doa_esprit_linear_array_t *h, int noutput_items, const void *d_cov_items,
                                            const void *d_counts, void *d_angles_out, void *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = esprit_work_args("esprit_linear_array_work_dev_counts", h, noutput_items, d_cov_items, d_angles_out, true, d_counts);
        rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    return esprit_run_dev(h, noutput_items, d_cov_items, d_counts, d_angles_out, d_status_out, static_cast<hipStream_t>(hip_stream));
}

int doa_esprit_linear_array_work(doa_esprit_linear_array_t *h, int noutput_items, const void *cov_items, void *angles_out,
                                 void *status_out)
{
    doa::clear_error();
    if (int rc = esprit_work_args("esprit_linear_array_work", h, noutput_items, cov_items, angles_out, false, nullptr); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    return esprit_run_host(h, noutput_items, cov_items, nullptr, angles_out, status_out);
}

int doa_esprit_linear_array_work_counts(doa_esprit_linear_array_t *h, int noutput_items, const void *cov_items, const void *counts,
                                        void *angles_out, void *status_out)
{
    doa::clear_error();
    if (int rc = esprit_work_args("esprit_linear_array_work_counts", h, noutput_items, cov_items, angles_out, true, counts); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    return esprit_run_host(h, noutput_items, cov_items, counts, angles_out, status_out);
}

int doa_esprit_linear_array_record_debug(doa_esprit_linear_array_t *h, int noutput_items, const void *cov_items, const void *records,
                                         const void *counts, void *angles_out, int *status_out)
{
    doa::clear_error();
    const char *who = "esprit_linear_array_record_debug";
    if (int rc = doa::work_args(who, h, noutput_items, {cov_items, records, angles_out}, 1); rc != DOA_OK) return rc;
    if (int rc = doa::need_bits64(who, h->bits, "ESPRIT"); rc != DOA_OK) return rc;
    return esprit_record_debug(h, noutput_items, cov_items, records, counts, angles_out, status_out);
}

}  // extern "C"
