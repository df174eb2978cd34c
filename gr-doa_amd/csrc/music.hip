// music.hip — MUSIC_lin_array on gfx950: host-side constructor tables, the K4 dispatch and the C ABI.
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

#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace doa {

// ---------------------------------------------------------------------------------------------
// host-side tables (constructor work of the reference block)
// ---------------------------------------------------------------------------------------------
int MusicTables::build(float norm_spacing_, int num_targets, int num_ant_ele, int pspectrum_len)
{
    N = num_ant_ele; M = num_targets; P = pspectrum_len; norm_spacing = norm_spacing_;
    // theta grid: float accumulator, sum formed in double (lib/MUSIC_lin_array_impl.cc:64-72)
    std::vector<float> theta(P);
    theta[0] = 0.0f;
    float theta_prev = 0.0f;
    for (int ii = 1; ii < P; ii++) {
        float th = (float)(theta_prev + 180.0 / P);
        theta_prev = th;
        theta[ii] = (float)(M_PI * th / 180.0);
    }
    // amv (:98-104): a_i[n] = exp(j * (-2 pi cos(theta_i)) * loc_n), loc_n = d*0.5*(N-1-2n) (:57-61), so
    // the phase step between neighbouring elements is psi_i = -2 pi cos(theta_i) * d.  Evaluated in
    // double from the float theta grid; the reference's float roundings of the scalar, of loc_n and of
    // each phase (~2e-7 rad) are not replayed (they are part of its own fp32 error budget).
    std::vector<float2> z(P);
    std::vector<double2> zd(P);
    const double d = (double)norm_spacing;
    for (int ii = 0; ii < P; ii++) {
        const double psi = -1.0 * 2 * M_PI * std::cos((double)theta[ii]) * d;
        z[ii] = make_float2((float)std::cos(psi), (float)std::sin(psi));
        zd[ii] = make_double2(std::cos(psi), std::sin(psi));
    }
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
    bool done = false;
    // compiled polynomial sizes: 2, 3, 4, 6, 8, 12, 16 (an array of n elements uses the next size up
    // with zero high-order coefficients)
    const int n = t.N;
    if (n < 2 || n > DOA_MAX_ANT_ELE) {
        set_error("MUSIC: num_ant_ele=%d outside the built range 2..%d", n, DOA_MAX_ANT_ELE);
        return DOA_ERR_UNSUPPORTED;
    }
    if (n == 2) done = launch_scan_n<2>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    else if (n == 3) done = launch_scan_n<3>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    else if (n == 4) done = launch_scan_n<4>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    else if (n <= 6) done = launch_scan_n<6>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    else if (n <= 8) done = launch_scan_n<8>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    else if (n <= 12) done = launch_scan_n<12>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    else done = launch_scan_n<16>(t, bits, n_items, d_coef, d_spec, d_q, pk, st);
    if (peaks_done) *peaks_done = done;
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

int launch_music_scan_group(const MusicTables &t, const PeakTables &peaks, const BatchGroup &grp, const void *d_cheb,
                            bool store_spectrum, hipStream_t st)
{
    if (grp.n_batches <= 0 || grp.n <= 0) return DOA_OK;
    bool ok = music_group_shape_ok(t.N, peaks.M, t.P, 64) && peaks.L == t.P && d_cheb && grp.n_batches <= kMaxGroup;
    for (int b = 0; b < grp.n_batches && ok; b++)
        ok = grp.spec[b] && reinterpret_cast<uintptr_t>(grp.spec[b]) % 16 == 0 && grp.mx[b] && grp.am[b];
    if (!ok) { set_error("MUSIC: not a group the lean scan kernel takes (N=%d, P=%d, %d batches)", t.N, t.P, grp.n_batches); return DOA_ERR_INVALID_ARG; }
    ScanPeakArgs pk;
    pk.cheb = d_cheb; pk.xaxis = peaks.d_x.as<float>(); pk.M = peaks.M; pk.store = store_spectrum;
    if (t.N == 2) launch_scan_group_n<2>(t, grp, pk, st);
    else if (t.N == 3) launch_scan_group_n<3>(t, grp, pk, st);
    else launch_scan_group_n<4>(t, grp, pk, st);
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
    const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave));
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

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"

struct doa_MUSIC_lin_array : doa::BlockBase {
    doa::MusicTables tab;
    doa::DevBuf d_in, d_out, d_coef, d_pn, d_q, d_cheb, d_counts;
};

static int music_validate(const char *who, float norm_spacing, int num_targets, int num_ant_ele)
{
    // grc/doa_MUSIC_lin_array.xml:33-35 (inputs > 0, inputs > num_targets, norm_spacing <= 0.5); the
    // reference ctor does not validate (num_targets >= N would index cols(0,-1)), so create fails here.
    if (num_ant_ele <= 0 || num_targets <= 0 || num_targets >= num_ant_ele) {
        doa::set_error("%s: need 0 < num_targets < num_ant_ele (got %d, %d)", who, num_targets, num_ant_ele);
        return DOA_ERR_INVALID_ARG;
    }
    if (!(norm_spacing > 0.0f) || norm_spacing > 0.5f) {
        doa::set_error("%s: need 0 < norm_spacing <= 0.5 (got %g)", who, (double)norm_spacing);
        return DOA_ERR_INVALID_ARG;
    }
    if (num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("%s: num_ant_ele=%d exceeds DOA_MAX_ANT_ELE=%d", who, num_ant_ele, DOA_MAX_ANT_ELE);
        return DOA_ERR_UNSUPPORTED;
    }
    return DOA_OK;
}

// checks of the per-item-count entries
static int music_counts_args(const char *who, doa_MUSIC_lin_array_t *h, int n, const void *cov, const void *counts, const void *out)
{
    if (int rc = doa::work_args(who, h, n, {cov, counts, out}); rc != DOA_OK) return rc;
    return doa::need_bits64(who, h->bits, "per-item counts");
}

extern "C" {

doa_MUSIC_lin_array_t *doa_MUSIC_lin_array_create(float norm_spacing, int num_targets, int num_ant_ele,
                                                  int pspectrum_len)
{
    doa::clear_error();
    if (music_validate("MUSIC_lin_array", norm_spacing, num_targets, num_ant_ele) != DOA_OK) return nullptr;
    if (pspectrum_len <= 0) {
        doa::set_error("MUSIC_lin_array: pspectrum_len must be > 0 (got %d)", pspectrum_len);
        return nullptr;
    }
    return doa::create_block<doa_MUSIC_lin_array>("MUSIC_lin_array", [&](doa_MUSIC_lin_array &h) {
        return h.tab.build(norm_spacing, num_targets, num_ant_ele, pspectrum_len);
    });
}

void doa_MUSIC_lin_array_destroy(doa_MUSIC_lin_array_t *h) { doa::destroy_block(h); }

long long doa_MUSIC_lin_array_items_total(const doa_MUSIC_lin_array_t *h) { return h ? h->items_total : 0; }

int doa_MUSIC_lin_array_work_dev(doa_MUSIC_lin_array_t *h, int noutput_items, const void *d_input_items0,
                                 void *d_output_items0, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("MUSIC_lin_array_work_dev", h, noutput_items, {d_input_items0, d_output_items0}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int N = h->tab.N;
    int rc = h->d_coef.reserve((size_t)noutput_items * doa::coef_stride(N) * sizeof(double));
    const bool cheb = doa::music_uses_cheb(N, h->bits);
    if (rc == DOA_OK && cheb) rc = h->d_cheb.reserve((size_t)noutput_items * doa::kChebRecord * sizeof(double));
    if (rc != DOA_OK) return rc;
    doa::EvdOut out;
    if (h->bits == 64) out.coef_d = h->d_coef.as<double>();
    else out.coef = h->d_coef.as<float>();
    if (cheb) out.cheb_d = h->d_cheb.as<double>();
    rc = doa::launch_music_evd(N, h->tab.M, noutput_items, d_input_items0, out, h->bits, st);
    if (rc != DOA_OK) return rc;
    rc = doa::launch_music_scan(h->tab, h->bits, noutput_items, h->d_coef.p, d_output_items0, nullptr, st, nullptr, nullptr, nullptr,
                                nullptr, true, cheb ? h->d_cheb.p : nullptr);
    if (rc != DOA_OK) return rc;
    h->items_total += noutput_items;
    return noutput_items;
}

int doa_MUSIC_lin_array_work(doa_MUSIC_lin_array_t *h, int noutput_items, const void *input_items0,
                             void *output_items0)
{
    doa::clear_error();
    if (int rc = doa::work_args("MUSIC_lin_array_work", h, noutput_items, {input_items0, output_items0}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    doa::HostCall io(*h);
    io.in(h->d_in, input_items0, (size_t)noutput_items * h->tab.N * h->tab.N * sizeof(float2));
    io.out(h->d_out, output_items0, (size_t)noutput_items * h->tab.P * sizeof(float));
    int rc = io.status();
    if (rc == DOA_OK) rc = doa_MUSIC_lin_array_work_dev(h, noutput_items, h->d_in.p, h->d_out.p, h->stream);
    return io.finish(rc);
}

int doa_MUSIC_lin_array_work_dev_counts(doa_MUSIC_lin_array_t *h, int noutput_items, const void *d_cov_items,
                                        const void *d_counts, void *d_spectrum_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = music_counts_args("MUSIC_lin_array_work_dev_counts", h, noutput_items, d_cov_items, d_counts, d_spectrum_out); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int N = h->tab.N;
    int rc = h->d_coef.reserve((size_t)noutput_items * doa::coef_stride(N) * sizeof(double));
    const bool cheb = doa::music_uses_cheb(N, 64);
    if (rc == DOA_OK && cheb) rc = h->d_cheb.reserve((size_t)noutput_items * doa::kChebRecord * sizeof(double));
    if (rc != DOA_OK) return rc;
    doa::EvdOut out;
    out.coef_d = h->d_coef.as<double>();
    if (cheb) out.cheb_d = h->d_cheb.as<double>();
    rc = doa::launch_music_evd_counts(N, noutput_items, d_cov_items, doa::evd_counts_forced((const int *)d_counts), out, st);
    if (rc != DOA_OK) return rc;
    rc = doa::launch_music_scan(h->tab, 64, noutput_items, h->d_coef.p, d_spectrum_out, nullptr, st, nullptr, nullptr, nullptr,
                                nullptr, true, cheb ? h->d_cheb.p : nullptr);
    if (rc == DOA_OK) rc = doa::launch_music_invalid_rows(N, h->tab.P, noutput_items, d_counts, d_spectrum_out, st);
    if (rc != DOA_OK) return rc;
    h->items_total += noutput_items;
    return noutput_items;
}

int doa_MUSIC_lin_array_work_counts(doa_MUSIC_lin_array_t *h, int noutput_items, const void *cov_items, const void *counts,
                                    void *spectrum_out)
{
    doa::clear_error();
    if (int rc = music_counts_args("MUSIC_lin_array_work_counts", h, noutput_items, cov_items, counts, spectrum_out); rc != DOA_OK)
        return rc;
    if (noutput_items == 0) return 0;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, (size_t)noutput_items * h->tab.N * h->tab.N * sizeof(float2));
    io.in(h->d_counts, counts, (size_t)noutput_items * sizeof(int));
    io.out(h->d_out, spectrum_out, (size_t)noutput_items * h->tab.P * sizeof(float));
    int rc = io.status();
    if (rc == DOA_OK) rc = doa_MUSIC_lin_array_work_dev_counts(h, noutput_items, h->d_in.p, h->d_counts.p, h->d_out.p, h->stream);
    return io.finish(rc);
}

int doa_MUSIC_lin_array_debug(doa_MUSIC_lin_array_t *h, int noutput_items, const void *input_items0,
                              void *projector_out, void *null_spectrum_out)
{
    doa::clear_error();
    if (int rc = doa::work_args("MUSIC_lin_array_debug", h, noutput_items, {input_items0}, 1); rc != DOA_OK) return rc;
    const int N = h->tab.N, P = h->tab.P;
    const size_t in_bytes = (size_t)noutput_items * N * N * sizeof(float2);
    const size_t sp_bytes = (size_t)noutput_items * P * sizeof(float);
    doa::HostCall io(*h);
    io.in(h->d_in, input_items0, in_bytes);
    io.out(h->d_out, nullptr, sp_bytes);
    io.out(h->d_q, null_spectrum_out, sp_bytes);
    io.out(h->d_pn, projector_out, in_bytes);
    io.out(h->d_coef, nullptr, (size_t)noutput_items * doa::coef_stride(N) * sizeof(double));
    int rc = io.status();
    doa::EvdOut out;
    if (h->bits == 64) out.coef_d = h->d_coef.as<double>();
    else out.coef = h->d_coef.as<float>();
    out.pn_out = h->d_pn.as<float2>();
    if (rc == DOA_OK) rc = doa::launch_music_evd(N, h->tab.M, noutput_items, h->d_in.p, out, h->bits, h->stream);
    if (rc == DOA_OK) rc = doa::launch_music_scan(h->tab, h->bits, noutput_items, h->d_coef.p, h->d_out.p, h->d_q.p, h->stream);
    return io.finish(rc == DOA_OK ? noutput_items : rc);
}

long long doa_hip_evd_fallback_count(int reset)
{
    doa::clear_error();
    int dev = 0;
    if (doa::ensure_device(&dev) != DOA_OK) return -1;
    return doa::evd_fallback_count(reset != 0);
}

int doa_hip_evd_fallback_counter_device_debug(void)
{
    doa::clear_error();
    int dev = 0;
    if (doa::ensure_device(&dev) != DOA_OK) return -1;
    return doa::evd_fallback_counter_device(doa::evd_fallback_counter());
}

int doa_MUSIC_lin_array_set_internal_precision(doa_MUSIC_lin_array_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("MUSIC_lin_array_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
