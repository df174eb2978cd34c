// wideband_music.hip — incoherent wideband MUSIC on gfx950 (Wax, Shan and Kailath 1984): one spectrum per snapshot from the
// covariance items of all its frequency bins (channel_covariance writes them).  The phase table, the scan kernel and its
// launcher, and the C ABI of doa_wideband_music.  Not a block of the reference; the definition is stated once in
// include/doa_hip.h.
//
// The front is the eigen stage of MUSIC_lin_array, unchanged (spectrum_chain.hpp: spectrum_front over the n * num_bins items
// with a MUSIC / uniform-linear-array / 64-bit description): one double coefficient record per item.  The scan is the kernel
// below.  What it saves against the chain by hand (MUSIC_lin_array over n * num_bins items, then a reduction over the rows):
// num_bins - 1 of every num_bins spectrum rows are never written, and every bin is evaluated at its own spacing in wavelengths.
//
// Structure: "wave over angles", as array_scan.hip.  One workgroup of 256 threads per snapshot; thread t owns the directions
// t + 256 m, four per step in registers.  The loop over the bins runs inside a step, in item order: a bin's weight, count and
// coefficient record are workgroup-uniform, so they travel through scalar loads, a skipped bin costs one uniform branch, and
// the coefficients reach the FMAs of the Horner chain (music_scan_impl.hpp: null_spectrum) as scalar operands.  Row j of the
// table is read with coalesced 16-byte loads (1 MiB at 64 bins of 1024 directions: it lives in L2).  q = (float) Q is parked
// in an LDS row until the row minimum is known; the second pass turns the row into dB with the normalisation of the other
// scans (LeanNorm / db_from_ratio) and writes it to memory ONCE.  Status and NaN rows are decided in front of the scan by
// the same workgroup: there is no follow-up launch.  No atomics.
//   P <= 4096    16 KiB of LDS
//   P <= 16384   64 KiB (gfx950)
#include "kernels.hpp"
#include "music_scan_impl.hpp"

#include <cmath>
#include <vector>

namespace doa {
namespace {

constexpr int kWbThreads = 256;
constexpr int kWbDirs = 4;          // directions per thread and step

// what bin j of the snapshot is: 0 skipped, 1 used, 2 a count that is neither 0 nor a possible source count
__device__ __forceinline__ int wb_bin_state(const float *__restrict__ w, const int *__restrict__ c, size_t item, int n_ant)
{
    const float wf = w ? w[item] : 1.0f;
    if (!bin_weight_used(wf)) return 0;
    if (!c) return 1;
    const int m = c[item];
    if (m == 0) return 0;
    return (m >= 1 && m < n_ant) ? 1 : 2;
}

// NP: the compiled polynomial size (>= n_ant; records are 2 n_ant doubles, the missing high-order coefficients are zero).
// COMBINE: DOA_WIDEBAND_NULL_MEAN / DOA_WIDEBAND_POWER_SUM.
template <int NP, int PMAX, int COMBINE>
__global__ __launch_bounds__(kWbThreads) void wideband_scan_kernel(const double *__restrict__ coef, const double2 *__restrict__ ztab,
                                                                   const float *__restrict__ weights, const int *__restrict__ counts,
                                                                   float *__restrict__ spec, float *__restrict__ qout,
                                                                   int *__restrict__ status, int P, int nb, int n_ant)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "wideband_scan_kernel keeps up to 64 KiB of row plus its reduction slots in LDS: gfx950 (MI355X) only"
#endif
    __shared__ float row[PMAX];
    __shared__ float red[2][kWbThreads / kWave];
    __shared__ int sflags[kWbThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wib = tid / kWave;
    const int snap = blockIdx.x;
    const size_t item0 = (size_t)snap * nb;
    const int rec = 2 * n_ant;
    float *grow = spec + (size_t)snap * P;
    float *qrow = qout ? qout + (size_t)snap * P : nullptr;

    // ---- status: which bins are used, a bad count, a used record that is not finite (element e of the snapshot's records) ----
    int flags = 0;
    for (int j = tid; j < nb; j += kWbThreads) {
        const int s = wb_bin_state(weights, counts, item0 + j, n_ant);
        flags |= (s == 1 ? 1 : 0) | (s == 2 ? 2 : 0);
    }
    for (int e = tid; e < nb * rec; e += kWbThreads) {
        const int j = e / rec;
        if (e - j * rec < rec - 1 && wb_bin_state(weights, counts, item0 + j, n_ant) == 1 && !__builtin_isfinite(coef[item0 * rec + e]))
            flags |= 4;
    }
    {
        const bool any_used = __builtin_amdgcn_ballot_w64((flags & 1) != 0) != 0ull;
        const bool any_bad = __builtin_amdgcn_ballot_w64((flags & 2) != 0) != 0ull;
        const bool any_nan = __builtin_amdgcn_ballot_w64((flags & 4) != 0) != 0ull;
        if (lane == 0) sflags[wib] = (any_used ? 1 : 0) | (any_bad ? 2 : 0) | (any_nan ? 4 : 0);
    }
    __syncthreads();
    const int f = __builtin_amdgcn_readfirstlane(sflags[0] | sflags[1] | sflags[2] | sflags[3]);
    const int st = (f & 2) ? 2 : (f & 4) ? 3 : (f & 1) ? 0 : 1;
    if (tid == 0 && status) status[snap] = st;
    if (st != 0) {                                          // workgroup-uniform
        for (int p = tid; p < P; p += kWbThreads) {
            __builtin_nontemporal_store(NAN, grow + p);
            if (qrow) qrow[p] = NAN;
        }
        return;
    }

    // ---- pass 1: Q_i at this thread's directions, its float image into the LDS row, the row minimum ----
    float mn = INFINITY;
    for (int p0 = 0; p0 < P; p0 += kWbThreads * kWbDirs) {
        int pa[kWbDirs];
#pragma unroll
        for (int a = 0; a < kWbDirs; a++) pa[a] = min(p0 + a * kWbThreads + tid, P - 1);     // clamped: every load is in the table
        double acc[kWbDirs];
#pragma unroll
        for (int a = 0; a < kWbDirs; a++) acc[a] = 0.0;
        double wsum = 0.0;
        const double2 *zrow = ztab;
        for (int j = 0; j < nb; j++, zrow += P) {
            // every branch here is workgroup-uniform (bad counts were refused above)
            if (wb_bin_state(weights, counts, item0 + j, n_ant) != 1) continue;
            const double w = (double)(weights ? weights[item0 + j] : 1.0f);
            const double *cr = coef + (item0 + j) * rec;
            double c[2 * NP];
#pragma unroll
            for (int k = 0; k < 2 * NP; k++) c[k] = (k < rec - 1) ? cr[k] : 0.0;
            double2 z[kWbDirs];
#pragma unroll
            for (int a = 0; a < kWbDirs; a++) z[a] = zrow[pa[a]];
#pragma unroll
            for (int a = 0; a < kWbDirs; a++) {
                const double Q = null_spectrum<NP, double>(c, z[a].x, z[a].y);
                if constexpr (COMBINE == DOA_WIDEBAND_NULL_MEAN) acc[a] = fma(w, Q, acc[a]);
                else acc[a] += w / Q;
            }
            wsum += w;
        }
#pragma unroll
        for (int a = 0; a < kWbDirs; a++) {
            const int p = p0 + a * kWbThreads + tid;
            if (p < P) {
                const float q = (float)(COMBINE == DOA_WIDEBAND_NULL_MEAN ? acc[a] / wsum : wsum / acc[a]);
                mn = fminf(mn, q);
                row[p] = q;
                if (qrow) qrow[p] = q;
            }
        }
    }
    {
        const float m = wave_allreduce_min(mn);
        if (lane == 0) red[0][wib] = m;
    }
    __syncthreads();                                        // the row and the wave minima are in LDS
    // ---- pass 2: dB, one write of the row.  Every branch is workgroup-uniform (the minimum). ----
    const float m = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    if (lean_norm_ok(m)) {
        const LeanNorm nrm(m);
        for (int p = tid; p < P; p += kWbThreads) {
            bool tie;
            __builtin_nontemporal_store(nrm.db(row[p], tie), grow + p);
        }
    } else {
        // a row whose minimum is not a positive normal number: the general semantics (db_from_ratio)
        float mx = -INFINITY;
        for (int p = tid; p < P; p += kWbThreads) mx = fmaxf(mx, 1.0f / row[p]);
        mx = wave_allreduce_max(mx);
        if (lane == 0) red[1][wib] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        const float inv_mx = __builtin_amdgcn_rcpf(mx);
        for (int p = tid; p < P; p += kWbThreads) __builtin_nontemporal_store(db_from_ratio(1.0f / row[p], mx, inv_mx), grow + p);
    }
}

template <int NP, int PMAX>
void launch_wideband_form(const WidebandTables &t, int n, const void *d_coef, const void *d_w, const void *d_counts, void *d_spec,
                          void *d_q, void *d_status, hipStream_t st)
{
#define DOA_WB_LAUNCH(C_)                                                                                                  \
    hipLaunchKernelGGL((wideband_scan_kernel<NP, PMAX, C_>), dim3(n), dim3(kWbThreads), 0, st, (const double *)d_coef,        \
                       t.d_z.as<double2>(), (const float *)d_w, (const int *)d_counts, (float *)d_spec, (float *)d_q,         \
                       (int *)d_status, t.P, t.sel.nb, t.N)
    if (t.combine == DOA_WIDEBAND_NULL_MEAN) DOA_WB_LAUNCH(DOA_WIDEBAND_NULL_MEAN);
    else DOA_WB_LAUNCH(DOA_WIDEBAND_POWER_SUM);
#undef DOA_WB_LAUNCH
}

template <int NP>
void launch_wideband_n(const WidebandTables &t, int n, const void *d_coef, const void *d_w, const void *d_counts, void *d_spec,
                       void *d_q, void *d_status, hipStream_t st)
{
    if (t.P <= 4096) launch_wideband_form<NP, 4096>(t, n, d_coef, d_w, d_counts, d_spec, d_q, d_status, st);
    else launch_wideband_form<NP, 16384>(t, n, d_coef, d_w, d_counts, d_spec, d_q, d_status, st);
}

}  // namespace

int WidebandTables::build(float norm_spacing, int num_targets, int num_ant_ele, int pspectrum_len, const BinSelection &sel_,
                          double rate_over_carrier, int combine_)
{
    N = num_ant_ele; M = num_targets; P = pspectrum_len; sel = sel_; combine = combine_;
    std::vector<float> theta(P);
    ula_theta_grid(P, theta.data());
    std::vector<double2> z((size_t)sel.nb * P);
    for (int j = 0; j < sel.nb; j++)
        ula_phase_row(theta.data(), P, wideband_bin_spacing(norm_spacing, rate_over_carrier, sel.F, sel.bin(j)),
                      z.data() + (size_t)j * P, nullptr);
    const size_t bytes = z.size() * sizeof(double2);
    if (int rc = d_z.reserve(bytes); rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_z.p, z.data(), bytes, hipMemcpyHostToDevice));
    return DOA_OK;
}

int launch_wideband_scan(const WidebandTables &t, int n, const void *d_coef, const void *d_weights, const void *d_counts, void *d_spec,
                         void *d_q, void *d_status, hipStream_t st)
{
    if (n <= 0) return DOA_OK;
    if (t.N < 2 || t.N > DOA_MAX_ANT_ELE || t.P < 1 || t.P > 16384 || t.sel.nb < 1 || !t.d_z.p || !d_coef || !d_spec ||
        (t.combine != DOA_WIDEBAND_NULL_MEAN && t.combine != DOA_WIDEBAND_POWER_SUM)) {
        set_error("wideband scan: bad arguments (N=%d, P=%d, %d bins, combine %d)", t.N, t.P, t.sel.nb, t.combine);
        return DOA_ERR_INVALID_ARG;
    }
    switch (scan_poly_size(t.N)) {
#define DOA_WB_CASE(np) case np: launch_wideband_n<np>(t, n, d_coef, d_weights, d_counts, d_spec, d_q, d_status, st); break;
    DOA_SCAN_SIZES(DOA_WB_CASE)
#undef DOA_WB_CASE
    }
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"
#include "spectrum_chain.hpp"

struct doa_wideband_music : doa::BlockBase {
    doa::SpectrumDesc desc;         // the front's description: MUSIC on a uniform linear array; ula points at the member below
    doa::MusicTables ula;           // the carrier's table (the description names one; the front does not read it)
    doa::WidebandTables tab;
    doa::SpectrumBufs recs;
    doa::DevBuf d_in, d_w, d_counts, d_out, d_status;
};

namespace {

constexpr const char *kWho = "wideband_music";

int wb_args(const char *who, const doa_wideband_music *h, int n, const void *cov, const void *counts, bool counted, const void *spec)
{
    const int rc = counted ? doa::work_args(who, h, n, {cov, counts, spec}) : doa::work_args(who, h, n, {cov, spec});
    if (rc != DOA_OK) return rc;
    if (int irc = doa::snapshot_items(who, n, h->tab.sel.nb); irc != DOA_OK) return irc;
    return doa::need_bits64(who, h->bits, "the wideband scan");
}

int wb_work_dev(const char *who, doa_wideband_music *h, int n, const void *d_cov, const void *d_weights, const void *d_counts,
                bool counted, void *d_spec, void *d_q, void *d_status, void *hip_stream)
{
    doa::clear_error();
    if (int rc = wb_args(who, h, n, d_cov, d_counts, counted, d_spec); rc != DOA_OK) return rc;
    if (n == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int items = n * h->tab.sel.nb;
    const doa::EvdCounts cnt = doa::evd_counts_forced((const int *)d_counts);
    doa::SpectrumDesc d = h->desc;
    d.bits = h->bits;
    d.counts = counted ? &cnt : nullptr;
    const doa::SpectrumPlan plan = doa::spectrum_plan(d);
    int rc = h->recs.reserve(plan, (size_t)items);
    if (rc != DOA_OK) return rc;
    const doa::SpectrumRecords rec = h->recs.view(plan);
    rc = doa::spectrum_front(d, items, d_cov, rec, nullptr, st);
    if (rc == DOA_OK) rc = doa::launch_wideband_scan(h->tab, n, rec.coef, d_weights, counted ? d_counts : nullptr, d_spec, d_q, d_status, st);
    if (rc != DOA_OK) return rc;
    h->items_total += n;
    return n;
}

int wb_work(const char *who, const char *who_dev, doa_wideband_music *h, int n, const void *cov, const void *weights, const void *counts,
            bool counted, void *spec, void *status_out)
{
    doa::clear_error();
    if (int rc = wb_args(who, h, n, cov, counts, counted, spec); rc != DOA_OK) return rc;
    if (n == 0) return 0;
    const size_t items = (size_t)n * h->tab.sel.nb;
    doa::HostCall io(*h);
    io.in(h->d_in, cov, items * h->tab.N * h->tab.N * sizeof(float2));
    if (weights) io.in(h->d_w, weights, items * sizeof(float));
    if (counted) io.in(h->d_counts, counts, items * sizeof(int));
    io.out(h->d_out, spec, (size_t)n * h->tab.P * sizeof(float));
    if (status_out) io.out(h->d_status, status_out, (size_t)n * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = wb_work_dev(who_dev, h, n, h->d_in.p, weights ? h->d_w.p : nullptr, h->d_counts.p, counted, h->d_out.p, nullptr,
                         status_out ? h->d_status.p : nullptr, h->stream);
    return io.finish(rc);
}

}  // namespace

extern "C" {

double doa_wideband_bin_spacing(float norm_spacing, double rate_over_carrier, int fft_len, int bin)
{
    if (fft_len < 1 || bin < 0 || bin >= fft_len) return NAN;
    return doa::wideband_bin_spacing(norm_spacing, rate_over_carrier, fft_len, bin);
}

doa_wideband_music_t *doa_wideband_music_create(float norm_spacing, int num_targets, int num_ant_ele, int pspectrum_len, int fft_len,
                                                int first_bin, int num_bins, double rate_over_carrier, int combine)
{
    doa::clear_error();
    if (num_ant_ele <= 0 || num_targets <= 0 || num_targets >= num_ant_ele) {
        doa::set_error("%s: need 0 < num_targets < num_ant_ele (got %d, %d)", kWho, num_targets, num_ant_ele);
        return nullptr;
    }
    if (num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("%s: num_ant_ele=%d exceeds DOA_MAX_ANT_ELE=%d", kWho, num_ant_ele, DOA_MAX_ANT_ELE);
        return nullptr;
    }
    if (doa::check_norm_spacing(kWho, norm_spacing) != DOA_OK) return nullptr;
    if (pspectrum_len < 1 || pspectrum_len > 16384) {
        doa::set_error("%s: need 1 <= pspectrum_len <= 16384 (got %d)", kWho, pspectrum_len);
        return nullptr;
    }
    if (doa::fft_len_log2(fft_len) < 0) {
        doa::set_error("%s: fft_len must be 16, 32, 64, 128 or 256 (got %d)", kWho, fft_len);
        return nullptr;
    }
    if (doa::check_bin_selection(kWho, fft_len, first_bin, num_bins) != DOA_OK) return nullptr;
    if (doa::check_rate_over_carrier(kWho, rate_over_carrier) != DOA_OK) return nullptr;
    const doa::BinSelection sel{fft_len, first_bin, num_bins};
    if (doa::check_bin_spacings(kWho, norm_spacing, rate_over_carrier, sel) != DOA_OK) return nullptr;
    if (combine != DOA_WIDEBAND_NULL_MEAN && combine != DOA_WIDEBAND_POWER_SUM) {
        doa::set_error("%s: combine must be DOA_WIDEBAND_NULL_MEAN (0) or DOA_WIDEBAND_POWER_SUM (1) (got %d)", kWho, combine);
        return nullptr;
    }
    return doa::create_block<doa_wideband_music>(kWho, [&](doa_wideband_music &h) {
        h.desc.estimator = DOA_ESTIMATOR_MUSIC; h.desc.N = num_ant_ele; h.desc.M = num_targets; h.desc.ula = &h.ula;
        if (int rc = h.ula.build(norm_spacing, num_targets, num_ant_ele, pspectrum_len); rc != DOA_OK) return rc;
        return h.tab.build(norm_spacing, num_targets, num_ant_ele, pspectrum_len, sel, rate_over_carrier, combine);
    });
}
void doa_wideband_music_destroy(doa_wideband_music_t *h) { doa::destroy_block(h); }
long long doa_wideband_music_items_total(const doa_wideband_music_t *h) { return h ? h->items_total : 0; }

int doa_wideband_music_work_dev(doa_wideband_music_t *h, int noutput_items, const void *d_cov_items, const void *d_weights,
                                void *d_spectrum_out, void *d_q_out, void *d_status_out, void *hip_stream)
{
    return wb_work_dev("wideband_music_work_dev", h, noutput_items, d_cov_items, d_weights, nullptr, false, d_spectrum_out, d_q_out,
                       d_status_out, hip_stream);
}
int doa_wideband_music_work(doa_wideband_music_t *h, int noutput_items, const void *cov_items, const float *weights, void *spectrum_out,
                            void *status_out)
{
    return wb_work("wideband_music_work", "wideband_music_work_dev", h, noutput_items, cov_items, weights, nullptr, false, spectrum_out,
                   status_out);
}
int doa_wideband_music_work_dev_counts(doa_wideband_music_t *h, int noutput_items, const void *d_cov_items, const void *d_counts,
                                       const void *d_weights, void *d_spectrum_out, void *d_q_out, void *d_status_out, void *hip_stream)
{
    return wb_work_dev("wideband_music_work_dev_counts", h, noutput_items, d_cov_items, d_weights, d_counts, true, d_spectrum_out,
                       d_q_out, d_status_out, hip_stream);
}
int doa_wideband_music_work_counts(doa_wideband_music_t *h, int noutput_items, const void *cov_items, const void *counts,
                                   const float *weights, void *spectrum_out, void *status_out)
{
    return wb_work("wideband_music_work_counts", "wideband_music_work_dev_counts", h, noutput_items, cov_items, weights, counts, true,
                   spectrum_out, status_out);
}

}  // extern "C"
