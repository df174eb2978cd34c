// music.hip — MUSIC_lin_array on gfx950: host-side constructor tables and the K4 dispatch (the C ABI: spectrum_blocks.hip).
//
// Replaces gr::doa::MUSIC_lin_array (reference lib/MUSIC_lin_array_impl.cc):
//   ctor  :47-87,98-104  element positions, float-accumulated theta grid, steering vectors
//   work  :121-144       eig_sym (LAPACK cheevd 'V','U', ascending) -> U_N = first N-M vectors
//                        -> P_N = U_N U_N^H -> out[i] = 1/Re(a_i^H P_N a_i) -> 10 log10(out/max)
//
// Where the pieces live:
//   * K2+K3 (EVD, noise projector, diagonal sums u_l = sum_r P_N[r+l, r]): music_evd.hip, jacobi.hpp.
//   * K4 (scan): for a ULA a_i^H P_N a_i is Hermitian-Toeplitz in the element index,
//         Q(psi_i) = u_0 + 2 Re sum_{l=1}^{N-1} u_l z_i^l,   z_i = exp(j psi_i), psi_i = k_i d,
//     so each angle costs N-1 complex Horner steps instead of N^2+N complex MACs (HBM-bound: 8N B in,
//     4P B out per item).  Kernels in music_scan_impl.hpp, one translation unit per polynomial size.
#include "kernels.hpp"
#include "music_scan.hpp"
#include "peak_device.hpp"

#include <cmath>
#include <vector>

namespace doa {

// ---------------------------------------------------------------------------------------------
// host-side tables (constructor work of the reference block)
// ---------------------------------------------------------------------------------------------
void ula_theta_grid(int P, float *theta)
{
    // theta grid: float accumulator, sum formed in double (lib/MUSIC_lin_array_impl.cc:64-72)
    theta[0] = 0.0f;
    float theta_prev = 0.0f;
    for (int ii = 1; ii < P; ii++) {
        float th = (float)(theta_prev + 180.0 / P);
        theta_prev = th;
        theta[ii] = (float)(M_PI * th / 180.0);
    }
}

void ula_phase_row(const float *theta, int P, double d, double2 *zd, float2 *z)
{
    // amv (:98-104): a_i[n] = exp(j * (-2 pi cos(theta_i)) * loc_n), loc_n = d*0.5*(N-1-2n) (:57-61), so
    // the phase step between neighbouring elements is psi_i = -2 pi cos(theta_i) * d.  Evaluated in
    // double from the float theta grid; the reference's float roundings of the scalar, of loc_n and of
    // each phase (~2e-7 rad) are not replayed (they are part of its own fp32 error budget).
    for (int ii = 0; ii < P; ii++) {
        const double psi = -1.0 * 2 * M_PI * std::cos((double)theta[ii]) * d;
        if (z) z[ii] = make_float2((float)std::cos(psi), (float)std::sin(psi));
        if (zd) zd[ii] = make_double2(std::cos(psi), std::sin(psi));
    }
}

int MusicTables::build(float norm_spacing_, int num_targets, int num_ant_ele, int pspectrum_len)
{
    N = num_ant_ele; M = num_targets; P = pspectrum_len; norm_spacing = norm_spacing_;
    std::vector<float> theta(P);
    ula_theta_grid(P, theta.data());
    std::vector<float2> z(P);
    std::vector<double2> zd(P);
    ula_phase_row(theta.data(), P, (double)norm_spacing, zd.data(), z.data());
    int rc = d_z.reserve(sizeof(float2) * (size_t)P);
    if (rc == DOA_OK) rc = d_zd.reserve(sizeof(double2) * (size_t)P);
    if (rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_z.p, z.data(), sizeof(float2) * (size_t)P, hipMemcpyHostToDevice));
    DOA_HIP_TRY(hipMemcpy(d_zd.p, zd.data(), sizeof(double2) * (size_t)P, hipMemcpyHostToDevice));
    return DOA_OK;
}

// ---------------------------------------------------------------------------------------------
// K4: spectrum scan — kernels in music_scan_impl.hpp, one translation unit per polynomial size
// ---------------------------------------------------------------------------------------------
DOA_SCAN_SIZES(DOA_SCAN_EXTERN)
DOA_SCAN_GROUP_EXTERN(2) DOA_SCAN_GROUP_EXTERN(3) DOA_SCAN_GROUP_EXTERN(4)

static ScanKnobs scan_knobs()
{
    return {DOA_LAB_ENV_INT("DOA_SCAN_WPB", kRouteWavesPerBlock), DOA_LAB_ENV_INT("DOA_SCAN_LEAN_WAVES_PER_CU", 0),
            DOA_LAB_ENV_INT("DOA_SCAN_NOTRIM", 0), DOA_LAB_ENV_INT("DOA_SCAN_WAVES_PER_CU", 8)};
}

int launch_music_scan(const MusicTables &t, int bits, int n_items, const void *d_coef, void *d_spec, void *d_q,
                      hipStream_t st, const PeakTables *peaks, void *d_max, void *d_argmax, bool *peaks_done,
                      bool store_spectrum, const void *d_cheb)
{
    if (peaks_done) *peaks_done = false;
    if (n_items <= 0) return DOA_OK;
    ScanPeakArgs pk;
    pk.cheb = (bits == 64) ? d_cheb : nullptr;
    if (peaks && d_max && d_argmax && peaks->L == t.P) {
        pk.xaxis = peaks->d_x.as<float>(); pk.val = (float *)d_max; pk.loc = (float *)d_argmax; pk.M = peaks->M;
        pk.store = store_spectrum;
    }
    ScanShape s;
    s.n_ant = t.N; s.bits = bits == 32 ? 32 : 64; s.P = t.P; s.n_items = n_items;
    s.spec_aligned = reinterpret_cast<uintptr_t>(d_spec) % 16 == 0; s.q = (d_q != nullptr);
    s.pick = (pk.val != nullptr); s.M = pk.M; s.store = pk.store; s.cheb = (pk.cheb != nullptr);
    const ScanRoute rt = scan_route(s, cu_count(), scan_knobs());
    if (rt.status != DOA_OK) { set_error("%s", rt.why); return rt.status; }
    switch (rt.N) {
#define DOA_SCAN_CASE(n) case n: launch_scan_n<n>(rt, t, bits, n_items, d_coef, d_spec, d_q, pk, st); break;
    DOA_SCAN_SIZES(DOA_SCAN_CASE)
#undef DOA_SCAN_CASE
    }
    if (peaks_done) *peaks_done = rt.picked;
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

int launch_music_scan_group(const MusicTables &t, const PeakTables &peaks, const BatchGroup &grp, const void *d_cheb,
                            bool store_spectrum, hipStream_t st)
{
    if (grp.n_batches <= 0 || grp.n <= 0) return DOA_OK;
    bool ok = peaks.L == t.P && grp.n_batches <= kMaxGroup;
    ScanShape s;
    s.n_ant = t.N; s.P = t.P; s.n_items = grp.n_batches * grp.n; s.M = peaks.M; s.store = store_spectrum;
    s.cheb = (d_cheb != nullptr); s.group = true; s.spec_aligned = true;
    for (int b = 0; b < grp.n_batches && ok; b++) {
        ok = grp.spec[b] && grp.mx[b] && grp.am[b];
        if (reinterpret_cast<uintptr_t>(grp.spec[b]) % 16) s.spec_aligned = false;
    }
    const ScanRoute rt = scan_route(s, cu_count(), scan_knobs());
    if (!ok || rt.status != DOA_OK) {
        set_error("MUSIC: not a group the lean scan kernel takes (N=%d, P=%d, %d batches)", t.N, t.P, grp.n_batches);
        return DOA_ERR_INVALID_ARG;
    }
    ScanPeakArgs pk;
    pk.cheb = d_cheb; pk.xaxis = peaks.d_x.as<float>(); pk.M = peaks.M; pk.store = store_spectrum;
    if (rt.N == 2) launch_scan_group_n<2>(rt, t, grp, pk, st);
    else if (rt.N == 3) launch_scan_group_n<3>(rt, t, grp, pk, st);
    else launch_scan_group_n<4>(rt, t, grp, pk, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

// Per-item counts: the scan kernels write 0.0 dB everywhere for an all-NaN null spectrum (their maximum search drops NaNs),
// so the rows of items whose count is outside 0..N-1 -- a NaN coefficient record -- are set to NaN here.  One wave per item; a
// wave with a valid count returns after one load.
__global__ __launch_bounds__(256) void music_invalid_rows_kernel(const int *__restrict__ counts, int N, float *__restrict__ spec,
                                                                 int P, int n_items)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int item = wave_index();
    if (item >= n_items) return;
    const int m = counts[item];
    if (m >= 0 && m < N) return;
    float *row = spec + (size_t)item * P;
    for (int p = lane; p < P; p += kWave) row[p] = NAN;
}

int launch_music_invalid_rows(int N, int P, int n_items, const void *d_counts, void *d_spec, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    hipLaunchKernelGGL(music_invalid_rows_kernel, dim3((n_items + 3) / 4), dim3(256), 0, st, (const int *)d_counts, N,
                       (float *)d_spec, P, n_items);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa
