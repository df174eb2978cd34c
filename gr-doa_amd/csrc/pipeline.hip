// pipeline.hip — autocorrelate -> MUSIC_lin_array -> find_local_max on device-resident streams.
//
// The batch entry point behind the benchmark: the three blocks exactly as
// apps/run_MUSIC_lin_array_simulation.grc wires them (autocorrelate(N, K, ovl, avg) ->
// MUSIC_lin_array(d, M, N, P) -> find_local_max(M, P, 0.0, 180.0)), as four launches on one
// stream: K1 covariance, K2+K3 EVD/projector/diagonal sums, K4 scan, K5 peak pick.  Intermediates
// (covariances, coefficient records, spectra) stay in HBM-resident buffers owned by the handle
// unless the caller asks for them.
#include "kernels.hpp"
#include "pipeline_lanes.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace doa {
bool find_local_max_fast_ok(int L, const void *d_in);
int launch_find_local_max_serial(const PeakTables &t, int n_items, const void *d_in, void *d_max, void *d_argmax,
                                 void *d_scratch, hipStream_t st);
}  // namespace doa

struct doa_music_pipeline {
    int N = 0, K = 0, ovl = 0, avg = 0;
    int max_batch = 0;
    int bits = 64;
    int device = 0;
    unsigned stages = 7;           // bit 0 K1, bit 1 K2+K3, bit 2 K4+K5 (doa_music_pipeline_set_stages)
    doa::MusicTables music;
    doa::PeakTables peaks;
    doa::DevBuf d_cov, d_coef, d_cheb, d_spec, d_scratch, d_gain;
    bool has_gain = false;
    int format = DOA_SAMPLE_FC32;   // doa_music_pipeline_set_input_format
    float scale = 1.0f;
    int S = 0, fb = 0;              // doa_music_pipeline_set_spatial_smoothing: subarray size (0 = off), forward-backward
    doa::DevBuf d_smooth;           // the smoothed items (S * S per item) between K1 and the eigen stage
    int estimator = DOA_ESTIMATOR_MUSIC;    // doa_music_pipeline_set_estimator
    double loading = 0.0;           // Capon: the diagonal loading
    doa::DevBuf d_status;           // Capon: int32 per item between the inverse launch and the NaN follow-up
    bool has_table = false;         // doa_music_pipeline_set_steering_table: an arbitrary array geometry
    doa::ArrayTable array;          // its table in the scan's form (array_scan.hip)
    doa::DevBuf d_full;             // the full records (N * N doubles per item) between the stage in front and the scan
    // host-pointer entry point only: two copy/compute lanes
    hipStream_t hst[2] = {nullptr, nullptr};
    doa::DevBuf d_in[2], d_res;
    doa::DevBuf d_work[2];          // K1's piece sums (overlapping windows), one per copy/compute lane
    doa::PinnedBuf h_stage;         // scheduler-sized calls: one page-locked staging buffer, one copy each way
    int fail_chunk = -1;            // doa_music_pipeline_inject_failure, host-pointer entry: one-shot, cleared by every call (tests)
    // doa_music_pipeline_work_dev_batches: the library's own overlap lanes (pipeline_lanes.hpp); a lane's buffers:
    enum { kCoef = 0, kCheb, kCov, kSpec, kWork, kScratch, kSmooth, kStatus, kFull };
    doa::PipeLanes lanes;
};

// what one K1 -> EVD -> scan chain needs besides its inputs and outputs
struct PipeWs {
    void *coef;             // coefficient records of the chain's items
    void *cheb;             // N <= 4, double: their pre-transformed twins for the lean scan kernel (else NULL)
    void *spec_scratch;     // P floats per item, used when the caller does not want the spectrum
    void *work;             // K1's piece sums (overlapping windows), or NULL
    void *smooth;           // spatial smoothing on: S * S gr_complex per item (else unused)
    void *status;           // Capon: int32 per item (else unused)
    void *full;             // steering-table handle: N * N doubles per item (else unused)
    doa::DevBuf *scratch;   // grown on demand: the serial peak pick of unusual vector lengths
    size_t scratch_item_off;
};

// K1 -> EVD -> scan (+ peak) for n items on `st` with the workspace `ws`.
// `spec` == nullptr: nobody wants the spectrum (angles-only call): ws.spec_scratch serves as scratch and the lean
// scan kernel neither converts the row to dB nor writes it.
static int run_k1(doa_music_pipeline *h, int n, const void *const *d_in, void *cov, const PipeWs &ws, hipStream_t st)
{
    if (~h->stages & 1u) return DOA_OK;         // doa_music_pipeline_set_stages (profiling aid; all stages in production)
    return doa::launch_autocorrelate(h->N, h->K, h->ovl, h->avg, n, d_in, cov, st, h->has_gain ? h->d_gain.p : nullptr, ws.work,
                                     h->format, h->scale);
}
// the array the eigen stage, the scan and the peak pick see: the subarray of a smoothed handle
static int evd_elements(const doa_music_pipeline *h) { return h->S ? h->S : h->N; }
static int run_evd_scan(doa_music_pipeline *h, int n, void *cov, void *spec, void *mx, void *am, const PipeWs &ws, hipStream_t st)
{
    const bool store_spec = (spec != nullptr);
    if (!spec) spec = ws.spec_scratch;
    const unsigned skip = ~h->stages & 7u;
    int rc = DOA_OK;
    const bool dbl = (h->bits == 64);
    void *coef = ws.coef;
    if (h->S) {                                 // spatial smoothing: one launch, part of stage bit 1; `cov` stays the N x N item
        if (!(skip & 2)) rc = doa::launch_spatial_smooth(h->N, h->S, h->fb, n, cov, ws.smooth, st);
        if (rc != DOA_OK) return rc;
        cov = ws.smooth;
    }
    const bool capon = (h->estimator == DOA_ESTIMATOR_CAPON);
    if (capon && !dbl) {
        doa::set_error("music_pipeline: the Capon estimator needs internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->has_table) {
        // an arbitrary array geometry: the stage in front writes full records, launch_array_scan replaces launch_music_scan,
        // and the peak pick is a launch of its own on the table's axis -- the launches of the blocks MUSIC_array /
        // capon_array and find_local_max
        if (!dbl) {
            doa::set_error("music_pipeline: a steering table needs internal precision 64 (handle is at %d)", h->bits);
            return DOA_ERR_UNSUPPORTED;
        }
        if (!(skip & 2)) {
            if (capon)
                rc = doa::launch_capon_inverse(h->N, n, cov, h->loading, nullptr, nullptr, nullptr, ws.status, st, ws.full);
            else
                rc = doa::launch_music_evd_full(h->N, h->music.M, n, cov, ws.full, nullptr, st);
        }
        if (rc != DOA_OK) return rc;
        if (skip & 4) return n;
        rc = doa::launch_array_scan(h->array, n, ws.full, spec, nullptr, st);
        if (rc != DOA_OK) return rc;
        if (doa::find_local_max_fast_ok(h->peaks.L, spec)) {
            rc = doa::launch_find_local_max(h->peaks, n, spec, mx, am, st);
        } else {
            rc = ws.scratch->reserve((size_t)h->max_batch * h->peaks.L);
            if (rc == DOA_OK)
                rc = doa::launch_find_local_max_serial(h->peaks, n, spec, mx, am,
                                                       static_cast<char *>(ws.scratch->p) + ws.scratch_item_off * h->peaks.L, st);
        }
        if (rc == DOA_OK && capon && !(skip & 2))
            rc = doa::launch_capon_invalid_rows(h->peaks.L, h->peaks.M, n, ws.status, store_spec ? spec : nullptr, mx, am, st);
        return rc == DOA_OK ? n : rc;
    }
    if (!(skip & 2)) {
        if (capon)
            rc = doa::launch_capon_inverse(evd_elements(h), n, cov, h->loading, coef, ws.cheb, nullptr, ws.status, st);
        else
            rc = doa::launch_music_evd(evd_elements(h), h->music.M, n, cov, dbl ? nullptr : coef, dbl ? coef : nullptr, nullptr, h->bits, st, ws.cheb);
    }
    if (rc != DOA_OK) return rc;
    bool peaks_done = false;
    if (skip & 4) return n;
    rc = doa::launch_music_scan(h->music, h->bits, n, coef, spec, nullptr, st, &h->peaks, mx, am, &peaks_done, store_spec, ws.cheb);
    if (rc != DOA_OK) return rc;
    if (!peaks_done) {
        if (doa::find_local_max_fast_ok(h->peaks.L, spec)) {
            rc = doa::launch_find_local_max(h->peaks, n, spec, mx, am, st);
        } else {
            rc = ws.scratch->reserve((size_t)h->max_batch * h->peaks.L);
            if (rc == DOA_OK)
                rc = doa::launch_find_local_max_serial(h->peaks, n, spec, mx, am,
                                                       static_cast<char *>(ws.scratch->p) + ws.scratch_item_off * h->peaks.L, st);
        }
    }
    // Capon: the scan wrote 0.0 dB rows (and the peak pick their peaks) for the NaN records of status-1 items (with the
    // inverse launch dropped by set_stages there is no status of this call to act on)
    if (rc == DOA_OK && capon && !(skip & 2))
        rc = doa::launch_capon_invalid_rows(h->peaks.L, h->peaks.M, n, ws.status, store_spec ? spec : nullptr, mx, am, st);
    return rc == DOA_OK ? n : rc;
}
static int run_ws(doa_music_pipeline *h, int n, const void *const *d_in, void *cov, void *spec, void *mx, void *am,
                  const PipeWs &ws, hipStream_t st)
{
    const int rc = run_k1(h, n, d_in, cov, ws, st);
    return rc != DOA_OK ? rc : run_evd_scan(h, n, cov, spec, mx, am, ws, st);
}

// the handle's own single workspace (work_dev and the host-pointer entry): records / scratch rows at item offset
// `item_off` (chunks in flight on different streams must not share them)
static int run_dev(doa_music_pipeline *h, int n, const void *const *d_in, void *cov, void *spec, void *mx, void *am,
                   size_t item_off, hipStream_t st, int lane = 0)
{
    const bool dbl = (h->bits == 64);
    PipeWs ws;
    ws.coef = static_cast<char *>(h->d_coef.p) + item_off * doa::coef_stride(h->N) * (dbl ? sizeof(double) : sizeof(float));
    ws.cheb = h->d_cheb.p ? static_cast<char *>(h->d_cheb.p) + item_off * doa::kChebRecord * sizeof(double) : nullptr;
    ws.spec_scratch = static_cast<char *>(h->d_spec.p) + item_off * h->peaks.L * sizeof(float);
    ws.work = h->d_work[lane].p;
    ws.smooth = h->S ? h->d_smooth.as<float2>() + item_off * h->S * h->S : nullptr;
    ws.status = h->d_status.p ? h->d_status.as<int>() + item_off : nullptr;
    ws.full = h->d_full.p ? h->d_full.as<double>() + item_off * doa::full_record_len(h->N) : nullptr;
    ws.scratch = &h->d_scratch;
    ws.scratch_item_off = item_off;
    return run_ws(h, n, d_in, cov, spec, mx, am, ws, st);
}

extern "C" {

doa_music_pipeline_t *doa_music_pipeline_create(int inputs, int snapshot_size, int overlap_size, int avg_method,
                                                float norm_spacing, int num_targets, int pspectrum_len, int max_batch)
{
    doa::clear_error();
    if (inputs <= 0 || inputs > DOA_MAX_ANT_ELE || snapshot_size <= 0 || overlap_size < 0 ||
        overlap_size >= snapshot_size) {
        doa::set_error("music_pipeline: bad autocorrelate parameters (inputs=%d snapshot=%d overlap=%d)", inputs,
                       snapshot_size, overlap_size);
        return nullptr;
    }
    if (num_targets <= 0 || num_targets >= inputs || num_targets > DOA_MAX_PEAKS || !(norm_spacing > 0.0f) ||
        norm_spacing > 0.5f || pspectrum_len <= 0 || max_batch <= 0) {
        doa::set_error("music_pipeline: bad MUSIC parameters (norm_spacing=%g num_targets=%d inputs=%d "
                       "pspectrum_len=%d max_batch=%d)", (double)norm_spacing, num_targets, inputs, pspectrum_len,
                       max_batch);
        return nullptr;
    }
    int dev = 0;
    if (doa::ensure_device(&dev) != DOA_OK) return nullptr;
    auto *h = new (std::nothrow) doa_music_pipeline();
    if (!h) { doa::set_error("out of memory"); return nullptr; }
    h->N = inputs; h->K = snapshot_size; h->ovl = overlap_size; h->avg = avg_method;
    h->max_batch = max_batch; h->device = dev;
    h->bits = doa::internal_precision_bits();
    int rc = h->music.build(norm_spacing, num_targets, inputs, pspectrum_len);
    if (rc == DOA_OK) rc = h->peaks.build(num_targets, pspectrum_len, 0.0f, 180.0f);
    if (rc == DOA_OK) rc = h->d_cov.reserve((size_t)max_batch * inputs * inputs * sizeof(float2));
    if (rc == DOA_OK) rc = h->d_coef.reserve((size_t)max_batch * doa::coef_stride(inputs) * sizeof(double));
    if (rc == DOA_OK && doa::music_uses_cheb(inputs, h->bits)) rc = h->d_cheb.reserve((size_t)max_batch * doa::kChebRecord * sizeof(double));
    if (rc == DOA_OK) rc = h->d_spec.reserve((size_t)max_batch * pspectrum_len * sizeof(float));
    if (const size_t ws = doa::autocorrelate_workspace_bytes(inputs, snapshot_size, overlap_size, max_batch); ws && rc == DOA_OK)
        rc = h->d_work[0].reserve(ws);
    if (rc != DOA_OK) {
        doa_music_pipeline_destroy(h);
        return nullptr;
    }
    return h;
}

void doa_music_pipeline_destroy(doa_music_pipeline_t *h)
{
    if (!h) return;
    h->music.release();
    h->peaks.release();
    h->d_cov.release(); h->d_coef.release(); h->d_cheb.release(); h->d_spec.release(); h->d_scratch.release(); h->d_gain.release();
    h->d_smooth.release(); h->d_status.release();
    h->array.release(); h->d_full.release();
    h->d_res.release(); h->h_stage.release();
    for (auto &b : h->d_work) b.release();
    for (auto &b : h->d_in) b.release();
    for (auto st : h->hst)
        if (st) (void)hipStreamDestroy(st);
    h->lanes.release();
    delete h;
}

int doa_music_pipeline_fuse_antenna_correction(doa_music_pipeline_t *h, const float *gains_re_im)
{
    doa::clear_error();
    if (!h) return DOA_ERR_INVALID_ARG;
    if (!gains_re_im) { h->has_gain = false; return DOA_OK; }
    const int N = h->N;
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

int doa_music_pipeline_set_input_format(doa_music_pipeline_t *h, int format, float scale)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_set_input_format: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (const int rc = doa::check_input_format("music_pipeline", format, scale); rc != DOA_OK) return rc;
    h->format = format; h->scale = scale;
    return DOA_OK;
}

int doa_music_pipeline_set_stages(doa_music_pipeline_t *h, int stage_mask)
{
    doa::clear_error();
    if (!h || stage_mask < 0 || stage_mask > 7) { doa::set_error("music_pipeline_set_stages: bad arguments"); return DOA_ERR_INVALID_ARG; }
    h->stages = (unsigned)stage_mask;
    return DOA_OK;
}

int doa_music_pipeline_set_spatial_smoothing(doa_music_pipeline_t *h, int subarray_size, int forward_backward)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_set_spatial_smoothing: bad arguments"); return DOA_ERR_INVALID_ARG; }
    const int S = subarray_size, fb = S ? forward_backward : 0;
    if (S != 0 && (S < 2 || S > h->N || h->music.M >= S || (fb != 0 && fb != 1))) {
        doa::set_error("music_pipeline_set_spatial_smoothing: need subarray_size 0 (off) or 2 <= subarray_size <= inputs with "
                       "num_targets < subarray_size, forward_backward 0 or 1 (got %d, %d; inputs=%d num_targets=%d)", S,
                       forward_backward, h->N, h->music.M);
        return DOA_ERR_INVALID_ARG;
    }
    if (S != 0 && h->has_table) {
        doa::set_error("music_pipeline_set_spatial_smoothing: smoothing assumes a translation-invariant (uniform linear) array; "
                       "this handle has a steering table");
        return DOA_ERR_UNSUPPORTED;
    }
    if (S == h->S && fb == h->fb) return DOA_OK;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int elements = S ? S : h->N;
    int rc = S ? h->d_smooth.reserve((size_t)h->max_batch * S * S * sizeof(float2)) : DOA_OK;
    if (rc == DOA_OK && doa::music_uses_cheb(elements, h->bits)) rc = h->d_cheb.reserve((size_t)h->max_batch * doa::kChebRecord * sizeof(double));
    if (rc != DOA_OK) return rc;
    // the scan's tables for `elements` antennas (the steering phases themselves depend on norm_spacing and pspectrum_len alone)
    const int was = h->music.N;
    rc = h->music.build(h->music.norm_spacing, h->music.M, elements, h->music.P);
    if (rc != DOA_OK) { h->music.N = was; return rc; }
    h->S = S; h->fb = fb;
    return DOA_OK;
}

int doa_music_pipeline_set_estimator(doa_music_pipeline_t *h, int estimator, float diagonal_loading)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_set_estimator: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (estimator != DOA_ESTIMATOR_MUSIC && estimator != DOA_ESTIMATOR_CAPON) {
        doa::set_error("music_pipeline_set_estimator: unknown estimator %d (DOA_ESTIMATOR_MUSIC or DOA_ESTIMATOR_CAPON)", estimator);
        return DOA_ERR_INVALID_ARG;
    }
    if (estimator == DOA_ESTIMATOR_CAPON) {
        if (!std::isfinite(diagonal_loading) || diagonal_loading < 0.0f) {
            doa::set_error("music_pipeline_set_estimator: diagonal_loading must be finite and >= 0 (got %g)", (double)diagonal_loading);
            return DOA_ERR_INVALID_ARG;
        }
        if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
        if (int rc = h->d_status.reserve((size_t)h->max_batch * sizeof(int)); rc != DOA_OK) return rc;
        h->loading = (double)diagonal_loading;
    }
    h->estimator = estimator;
    return DOA_OK;
}

int doa_music_pipeline_set_steering_table(doa_music_pipeline_t *h, const double *steering, float x_min, float x_max)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_set_steering_table: bad arguments"); return DOA_ERR_INVALID_ARG; }
    const int N = h->N, P = h->music.P, M = h->peaks.M;
    if (!steering) {                                     // back to the uniform linear array and its 0 .. 180 axis
        if (!h->has_table) return DOA_OK;
        if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
        doa::PeakTables axis;
        if (int rc = axis.build(M, P, 0.0f, 180.0f); rc != DOA_OK) { axis.release(); return rc; }
        h->peaks.release();
        h->peaks = std::move(axis);
        h->has_table = false;
        return DOA_OK;
    }
    if (!std::isfinite(x_min) || !std::isfinite(x_max) || !(x_max > x_min)) {
        doa::set_error("music_pipeline_set_steering_table: need finite x_min < x_max (got %g, %g)", (double)x_min, (double)x_max);
        return DOA_ERR_INVALID_ARG;
    }
    if (!doa::steering_table_finite(steering, N, P)) {
        doa::set_error("music_pipeline_set_steering_table: the table (%d rows of %d complex doubles) holds a value that is not finite", P, N);
        return DOA_ERR_INVALID_ARG;
    }
    if (h->S) {
        doa::set_error("music_pipeline_set_steering_table: spatial smoothing is on, and it assumes a translation-invariant "
                       "(uniform linear) array");
        return DOA_ERR_UNSUPPORTED;
    }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    // everything is built aside and swapped in at the end: a failure leaves the handle as it was
    doa::ArrayTable table;
    doa::PeakTables axis;
    int rc = table.build(N, P, steering);
    if (rc == DOA_OK) rc = axis.build(M, P, x_min, x_max);
    if (rc == DOA_OK) rc = h->d_full.reserve((size_t)h->max_batch * doa::full_record_len(N) * sizeof(double));
    if (rc != DOA_OK) { table.release(); axis.release(); return rc; }
    h->array.release(); h->peaks.release();
    h->array = std::move(table); h->peaks = std::move(axis);
    h->has_table = true;
    return DOA_OK;
}

int doa_music_pipeline_work_dev(doa_music_pipeline_t *h, int noutput_items, const void *const *d_input_items,
                                void *d_cov_out, void *d_spectrum_out, void *d_max_out, void *d_argmax_out,
                                void *hip_stream)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || !d_input_items || (noutput_items > 0 && (!d_max_out || !d_argmax_out))) {
        doa::set_error("music_pipeline_work_dev: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("music_pipeline_work_dev: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    void *cov = d_cov_out ? d_cov_out : h->d_cov.p;
    void *spec = d_spectrum_out;                       // NULL = angles only (run_dev)
    return run_dev(h, noutput_items, d_input_items, cov, spec, d_max_out, d_argmax_out, 0,
                   static_cast<hipStream_t>(hip_stream));
}

// K1 as work_dev runs it, ONE eigen launch that estimates each item's count and forms its noise set from it, the scan (no
// fused peak pick: its M is launch-uniform), the counted peak pick: four launches, and one more when the caller wants the
// spectrum (launch_music_invalid_rows)
int doa_music_pipeline_work_dev_auto(doa_music_pipeline_t *h, int noutput_items, const void *const *d_input_items, int method,
                                     void *d_cov_out, void *d_spectrum_out, void *d_max_out, void *d_argmax_out,
                                     void *d_count_out, void *d_eig_out, void *hip_stream)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || !d_input_items || (method != DOA_SOURCE_COUNT_MDL && method != DOA_SOURCE_COUNT_AIC) ||
        (noutput_items > 0 && (!d_max_out || !d_argmax_out || !d_count_out))) {
        doa::set_error("music_pipeline_work_dev_auto: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("music_pipeline_work_dev_auto: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    if (h->bits != 64) {
        doa::set_error("music_pipeline_work_dev_auto: per-item counts need internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->estimator != DOA_ESTIMATOR_MUSIC) {
        doa::set_error("music_pipeline_work_dev_auto: the source count needs eigenvalues, which the Capon estimator does not form");
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->has_table) {
        doa::set_error("music_pipeline_work_dev_auto: a count per item is not available on a handle with a steering table");
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->K < 2) {
        doa::set_error("music_pipeline_work_dev_auto: the criterion needs snapshot_size >= 2 (handle has %d)", h->K);
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int n = noutput_items;
    const int elements = evd_elements(h);
    const bool cheb = doa::music_uses_cheb(elements, 64);
    // (a handle created at precision 32 and switched to 64 afterwards has no Chebyshev records yet)
    if (cheb && !h->d_cheb.p)
        if (int rc = h->d_cheb.reserve((size_t)h->max_batch * doa::kChebRecord * sizeof(double)); rc != DOA_OK) return rc;
    void *cov = d_cov_out ? d_cov_out : h->d_cov.p;
    void *spec = d_spectrum_out ? d_spectrum_out : h->d_spec.p;
    PipeWs ws{};
    ws.work = h->d_work[0].p;
    int rc = run_k1(h, n, d_input_items, cov, ws, st);
    if (rc == DOA_OK && h->S) {
        rc = doa::launch_spatial_smooth(h->N, h->S, h->fb, n, cov, h->d_smooth.p, st);
        cov = h->d_smooth.p;
    }
    if (rc == DOA_OK)
        rc = doa::launch_music_evd_counts(elements, n, cov, nullptr, d_count_out, d_eig_out, h->K, method, h->music.M, h->d_coef.p,
                                          cheb ? h->d_cheb.p : nullptr, st);
    if (rc == DOA_OK)
        rc = doa::launch_music_scan(h->music, 64, n, h->d_coef.p, spec, nullptr, st, nullptr, nullptr, nullptr, nullptr, true,
                                    cheb ? h->d_cheb.p : nullptr);
    // a spectrum the caller sees: the row of a count -1 item is NaN, as MUSIC_lin_array_work_dev_counts leaves it (a fifth,
    // one-load-per-item launch; the peak pick below does not read the rows of such items)
    if (rc == DOA_OK && d_spectrum_out) rc = doa::launch_music_invalid_rows(elements, h->peaks.L, n, d_count_out, spec, st);
    if (rc != DOA_OK) return rc;
    if (doa::find_local_max_fast_ok(h->peaks.L, spec)) {
        rc = doa::launch_find_local_max_counts(h->peaks, n, spec, d_count_out, d_max_out, d_argmax_out, st);
    } else {
        rc = h->d_scratch.reserve((size_t)h->max_batch * h->peaks.L);
        if (rc == DOA_OK)
            rc = doa::launch_find_local_max_serial_counts(h->peaks, n, spec, d_count_out, d_max_out, d_argmax_out, h->d_scratch.p, st);
    }
    return rc == DOA_OK ? n : rc;
}

int doa_music_pipeline_set_lanes(doa_music_pipeline_t *h, int n_lanes)
{
    doa::clear_error();
    if (!h || h->lanes.set_count(n_lanes) != DOA_OK) {
        doa::set_error("music_pipeline_set_lanes: need 1 <= n_lanes <= %d", doa::PipeLanes::kMaxLanes);
        return DOA_ERR_INVALID_ARG;
    }
    return DOA_OK;
}

// ---- work_dev_batches: groups of batches -------------------------------------------------------------------------------
// On the lean route (no overlap, N <= 4, double, P = 256 / 512 / 1024, the one-lane EVD) consecutive batches of a call form
// GROUPS, and one K1, one EVD and one scan launch each cover a whole group (kernels.hpp, BatchGroup): the two small kernels
// are slow at 4096 items because the launch is too small for them, not because of their arithmetic, and K1 pays its fixed
// cost per launch once per group.  Every other shape keeps one chain of launches per batch (a group of one).
// Tuning (profiles/grouped_batches.txt; the knobs exist in lab builds only):
//   * groups rotate over at most kGroupLanes = 2 lanes (the handle's lane count stays the upper bound): one lane's K1 hides the
//     other's EVD and scan; more lanes add nothing to hide and measured slower;
//   * on one lane a group takes up to kMaxGroup = 8 batches (the fewer launch boundaries the better); on two lanes up to
//     kLaneGroup = 4, so that the lanes alternate at a finer grain and -- with the benchmark's eight rotating buffer sets --
//     at all: a group that aliases an earlier one has to follow it on its lane, and groups of eight would all chain on one;
//   * a shorter first group (a stagger between the lanes without events) measured within the noise and is not used.
constexpr int kGroupLanes = 2, kLaneGroup = 4;
static int group_lanes() { const int v = DOA_LAB_ENV_INT("DOA_GROUP_LANES", kGroupLanes); return v < 1 ? 1 : v; }
static int group_batches(int lanes)
{
    const int v = DOA_LAB_ENV_INT("DOA_GROUP_BATCHES", 0) > 0 ? DOA_LAB_ENV_INT("DOA_GROUP_BATCHES", 0) : (lanes == 1 ? doa::kMaxGroup : kLaneGroup);
    return v > doa::kMaxGroup ? doa::kMaxGroup : v;
}
static int group_first() { return DOA_LAB_ENV_INT("DOA_GROUP_FIRST", 0); }     // batches in a call's first group (0: a full one)
// Angles-only batches use P floats of scratch per item (rows on the scan's irregular path): their groups are bounded so that a
// lane's scratch rows stay within kAnglesScratchBytes (or one batch's worth)
constexpr size_t kAnglesScratchBytes = (size_t)32 << 20;

namespace {
struct PlanGroup {
    int b0 = 0, nb = 0, cap = 1, lane = -1, req = -1;
    bool lean = false, store = false, vec2 = false;
    bool sync_first = false;        // its outputs alias groups on two different lanes: the lanes are joined on the host first
};
// output pointer -> index of the last group that writes it (open addressing; never shrinks within a call)
struct PtrGroups {
    std::vector<std::pair<const void *, int>> slot;
    size_t mask;
    explicit PtrGroups(size_t n_ptrs) { size_t c = 16; while (c < 2 * n_ptrs) c <<= 1; slot.assign(c, {nullptr, -1}); mask = c - 1; }
    std::pair<const void *, int> &at(const void *p)
    {
        size_t i = (reinterpret_cast<uintptr_t>(p) * 0x9E3779B97F4A7C15ull >> 20) & mask;
        while (slot[i].first && slot[i].first != p) i = (i + 1) & mask;
        return slot[i];
    }
};
}  // namespace

int doa_music_pipeline_work_dev_batches(doa_music_pipeline_t *h, int n_batches, int noutput_items,
                                        const void *const *d_input_items, void *const *d_cov_out,
                                        void *const *d_spectrum_out, void *const *d_max_out, void *const *d_argmax_out,
                                        void *hip_stream)
{
    doa::clear_error();
    if (!h || n_batches < 0 || noutput_items < 0 || !d_input_items || !d_max_out || !d_argmax_out) {
        doa::set_error("music_pipeline_work_dev_batches: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("music_pipeline_work_dev_batches: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    for (int b = 0; b < n_batches; b++)
        if (noutput_items > 0 && (!d_max_out[b] || !d_argmax_out[b])) {
            doa::set_error("music_pipeline_work_dev_batches: batch %d has no peak output pointers", b);
            return DOA_ERR_INVALID_ARG;
        }
    if (n_batches == 0 || noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int N = h->N, n = noutput_items, P = h->peaks.L;
    const int fail_at = h->lanes.fail_batch;
    h->fail_chunk = -1; h->lanes.fail_batch = -1;               // (the test aid is one-shot for whichever entry comes next)
    const bool injected = (fail_at >= 0 && fail_at < n_batches);
    const int n_run = injected ? fail_at : n_batches;           // batches before the injected failure are launched
    const bool solo = (h->lanes.n_lanes == 1 && hip_stream != DOA_STREAM_DETACHED);    // nothing to overlap: the caller's stream itself, no events
    const bool dbl = (h->bits == 64);

    // ---- the plan: groups of consecutive batches and their lanes ----
    const bool lean_shape = h->estimator == DOA_ESTIMATOR_MUSIC && !h->has_table && h->S == 0 && h->ovl == 0 && h->peaks.L == h->music.P && doa::music_group_shape_ok(N, h->music.M, P, h->bits) &&
                            (long long)doa::kMaxGroup * n <= (1 << 28);
    const int L_all = solo ? 1 : h->lanes.n_lanes;
    const int L = (lean_shape && group_lanes() < L_all) ? group_lanes() : L_all;
    const int G = lean_shape ? group_batches(L) : 1;
    const size_t angles_rows = kAnglesScratchBytes / ((size_t)h->max_batch * P * sizeof(float));
    const int G_angles = (int)(angles_rows < 1 ? 1 : (angles_rows > (size_t)G ? (size_t)G : angles_rows));
    int rot = h->lanes.next_lane % L;
    std::vector<PlanGroup> plan;
    plan.reserve((size_t)n_run / G + 8);
    PtrGroups writers((size_t)4 * n_run);
    auto outputs = [&](int b, const void *(&p)[4]) {
        p[0] = d_cov_out ? d_cov_out[b] : nullptr; p[1] = d_spectrum_out ? d_spectrum_out[b] : nullptr;
        p[2] = d_max_out[b]; p[3] = d_argmax_out[b];
    };
    auto close = [&](PlanGroup &g) {
        g.lane = (g.req >= 0) ? g.req : rot++ % L;
    };
    for (int b = 0; b < n_run; b++) {
        const void *out[4];
        outputs(b, out);
        PlanGroup nb;
        nb.b0 = b; nb.nb = 1;
        nb.store = (out[1] != nullptr);
        nb.lean = lean_shape && reinterpret_cast<uintptr_t>(out[1]) % 16 == 0;
        nb.vec2 = nb.lean && doa::autocorrelate_pair_loads(N, h->K, h->ovl, d_input_items + (size_t)b * N, h->format);
        nb.cap = !nb.lean ? 1 : (nb.store ? G : G_angles);
        if (plan.empty() && group_first() > 0 && group_first() < nb.cap) nb.cap = group_first();
        // which earlier groups write this batch's outputs: the open one (-> the batch starts a new group), closed ones (-> their lane)
        const int open = plan.empty() ? -1 : (int)plan.size() - 1;
        auto requirement = [&](int open_index, bool &in_open, bool &conflict) {
            int req = -1;
            in_open = conflict = false;
            for (const void *p : out) {
                if (!p) continue;
                const int gi = writers.at(p).second;
                if (gi < 0) continue;
                if (gi == open_index) { in_open = true; continue; }
                if (req >= 0 && req != plan[gi].lane) conflict = true;
                req = plan[gi].lane;
            }
            return req;
        };
        bool in_open, conflict;
        int req = requirement(open, in_open, conflict);
        bool join = false;
        if (open >= 0) {
            const PlanGroup &g = plan[open];
            join = g.lean && nb.lean && g.nb < g.cap && g.store == nb.store && g.vec2 == nb.vec2 && !in_open && !conflict &&
                   (req < 0 || g.req < 0 || g.req == req);
        }
        if (join) {
            plan[open].nb++;
            if (req >= 0) plan[open].req = req;
        } else {
            if (open >= 0) {
                close(plan[open]);
                req = requirement(-1, in_open, conflict);       // (the group just closed has a lane now)
            }
            nb.req = req; nb.sync_first = conflict;
            plan.push_back(nb);
        }
        for (const void *p : out)
            if (p) writers.at(p) = {p, (int)plan.size() - 1};
    }
    if (!plan.empty()) close(plan.back());
    h->lanes.next_lane = rot % L;

    // ---- workspaces and launches ----
    bool need_cov = !d_cov_out, need_spec = !d_spectrum_out;
    for (int b = 0; b < n_batches && !(need_cov && need_spec); b++) {
        if (d_cov_out && !d_cov_out[b]) need_cov = true;
        if (d_spectrum_out && !d_spectrum_out[b]) need_spec = true;
    }
    const size_t work_bytes = doa::autocorrelate_workspace_bytes(N, h->K, h->ovl, h->max_batch);
    using H = doa_music_pipeline;
    // a lane's buffers hold a whole group: records and covariances are 64-128 B per item; the angles-only scratch rows are bounded (G_angles)
    auto reserve = [&](doa::DevBuf &coef, doa::DevBuf &cheb, doa::DevBuf &cov, doa::DevBuf &spec, doa::DevBuf &work,
                       doa::DevBuf &smooth, doa::DevBuf &status, doa::DevBuf &full) -> int {
        int rc = coef.reserve((size_t)h->max_batch * doa::coef_stride(N) * (dbl ? sizeof(double) : sizeof(float)));
        if (rc == DOA_OK && h->S) rc = smooth.reserve((size_t)h->max_batch * h->S * h->S * sizeof(float2));
        if (rc == DOA_OK && h->estimator == DOA_ESTIMATOR_CAPON) rc = status.reserve((size_t)h->max_batch * sizeof(int));
        if (rc == DOA_OK && h->has_table) rc = full.reserve((size_t)h->max_batch * doa::full_record_len(N) * sizeof(double));
        if (rc == DOA_OK && doa::music_uses_cheb(evd_elements(h), h->bits)) rc = cheb.reserve((size_t)G * h->max_batch * doa::kChebRecord * sizeof(double));
        if (rc == DOA_OK && need_cov) rc = cov.reserve((size_t)G * h->max_batch * N * N * sizeof(float2));
        if (rc == DOA_OK && need_spec) rc = spec.reserve((size_t)G_angles * h->max_batch * P * sizeof(float));
        if (rc == DOA_OK && work_bytes) rc = work.reserve(work_bytes);
        return rc;
    };
    auto launch = [&](const PlanGroup &g, const PipeWs &ws, void *lane_cov, hipStream_t st) -> int {
        if (!g.lean || g.nb == 1) {                              // one batch: the launches of work_dev
            int rc = DOA_OK;
            for (int b = g.b0; b < g.b0 + g.nb && rc >= 0; b++) {
                void *cov = (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : lane_cov;
                rc = run_ws(h, n, d_input_items + (size_t)b * N, cov, d_spectrum_out ? d_spectrum_out[b] : nullptr, d_max_out[b],
                            d_argmax_out[b], ws, st);
            }
            return rc;
        }
        doa::BatchGroup grp;
        grp.n_batches = g.nb; grp.n = n;
        for (int k = 0; k < g.nb; k++) {
            const int b = g.b0 + k;
            grp.in[k] = d_input_items + (size_t)b * N;
            grp.cov[k] = (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : static_cast<char *>(lane_cov) + (size_t)k * n * N * N * sizeof(float2);
            grp.spec[k] = g.store ? d_spectrum_out[b] : static_cast<char *>(ws.spec_scratch) + (size_t)k * n * P * sizeof(float);
            grp.mx[k] = d_max_out[b]; grp.am[k] = d_argmax_out[b];
        }
        const unsigned skip = ~h->stages & 7u;                   // doa_music_pipeline_set_stages
        int rc = DOA_OK;
        if (!(skip & 1)) rc = doa::launch_autocorrelate_group(N, h->K, h->avg, grp, st, h->has_gain ? h->d_gain.p : nullptr, h->format, h->scale);
        if (rc == DOA_OK && !(skip & 2)) rc = doa::launch_music_evd_group(N, h->music.M, grp, nullptr, ws.cheb, st);
        if (rc == DOA_OK && !(skip & 4)) rc = doa::launch_music_scan_group(h->music, h->peaks, grp, ws.cheb, g.store, st);
        return rc;
    };
    if (solo) {
        hipStream_t caller = static_cast<hipStream_t>(hip_stream);
        int rc = reserve(h->d_coef, h->d_cheb, h->d_cov, h->d_spec, h->d_work[0], h->d_smooth, h->d_status, h->d_full);
        if (rc != DOA_OK) return rc;
        PipeWs ws;
        ws.coef = h->d_coef.p; ws.cheb = h->d_cheb.p; ws.spec_scratch = h->d_spec.p; ws.work = h->d_work[0].p;
        ws.smooth = h->d_smooth.p; ws.status = h->d_status.p; ws.full = h->d_full.p;
        ws.scratch = &h->d_scratch; ws.scratch_item_off = 0;
        for (size_t u = 0; u < plan.size() && rc >= 0; u++) rc = launch(plan[u], ws, h->d_cov.p, caller);
        if (rc >= 0 && injected) {
            doa::set_error("music_pipeline_work_dev_batches: injected failure in batch %d", fail_at);
            rc = DOA_ERR_HIP;
        }
        if (rc < 0) {
            const std::string msg = doa_last_error();
            (void)hipStreamSynchronize(caller);                  // the contract of an error return: nothing of the call still runs
            doa::set_error("%s", msg.c_str());
            return rc;
        }
        return n_batches * n;
    }
    auto prepare = [&](doa::PipeLane &ln) -> int {
        return reserve(ln.buf[H::kCoef], ln.buf[H::kCheb], ln.buf[H::kCov], ln.buf[H::kSpec], ln.buf[H::kWork], ln.buf[H::kSmooth],
                       ln.buf[H::kStatus], ln.buf[H::kFull]);
    };
    auto launch_unit = [&](int u, doa::PipeLane &ln) -> int {
        const PlanGroup &g = plan[u];
        if (g.sync_first)
            if (const int rc = h->lanes.synchronize(); rc != DOA_OK) return rc;
        PipeWs ws;
        ws.coef = ln.buf[H::kCoef].p; ws.cheb = ln.buf[H::kCheb].p; ws.spec_scratch = ln.buf[H::kSpec].p; ws.work = ln.buf[H::kWork].p;
        ws.smooth = ln.buf[H::kSmooth].p; ws.status = ln.buf[H::kStatus].p; ws.full = ln.buf[H::kFull].p;
        ws.scratch = &ln.buf[H::kScratch]; ws.scratch_item_off = 0;
        return launch(g, ws, ln.buf[H::kCov].p, ln.st);
    };
    const int rc = h->lanes.run_units("music_pipeline_work_dev_batches", (int)plan.size(), injected ? fail_at : -1, hip_stream, prepare,
                                      [&](int u) { return plan[u].lane; }, launch_unit);
    return rc < 0 ? rc : n_batches * n;
}

int doa_music_pipeline_set_lane_streams(doa_music_pipeline_t *h, int n_lanes, void *const *hip_streams)
{
    doa::clear_error();
    if (!h || n_lanes < 1 || n_lanes > doa::PipeLanes::kMaxLanes || !hip_streams) {
        doa::set_error("music_pipeline_set_lane_streams: need 1 <= n_lanes <= %d and the streams", doa::PipeLanes::kMaxLanes);
        return DOA_ERR_INVALID_ARG;
    }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    return h->lanes.adopt(n_lanes, hip_streams);
}

int doa_music_pipeline_synchronize(doa_music_pipeline_t *h)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_synchronize: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    return h->lanes.synchronize();
}

int doa_music_pipeline_work(doa_music_pipeline_t *h, int noutput_items, const void *const *input_items, void *cov_out,
                            void *spectrum_out, void *max_out, void *argmax_out)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || !input_items || (noutput_items > 0 && (!max_out || !argmax_out))) {
        doa::set_error("music_pipeline_work: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("music_pipeline_work: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items == 0) return 0;
    const int N = h->N, M = h->music.M, P = h->peaks.L;
    for (int k = 0; k < N; k++)
        if (!input_items[k]) { doa::set_error("music_pipeline_work: input_items[%d] is NULL", k); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    if (const int src = doa::ensure_stream_pair(h->hst); src != DOA_OK) return src;
    const size_t nonoverlap = (size_t)(h->K - h->ovl);
    const size_t sb = doa::sample_bytes(h->format);     // bytes per input sample: 8 (fc32) or 4 (sc16)
    // Scheduler-sized calls (a GNU Radio work() hands over a few to a few hundred items): the fixed costs are what
    // counts -- N pageable host-to-device copies, up to four copies back and two stream synchronisations.  Below
    // kSmallCallBytes of input the window of every stream is packed into ONE page-locked staging buffer (the same
    // bytes the driver's pageable path would stage, minus its per-copy set-up), crosses PCIe as ONE transfer, and the
    // angles (+ the optional covariances / spectra) come back as ONE transfer through the same buffer.  Measured: 8 items
    // 105 -> 53 us per call, 64 items 151 -> 116 us; from 8 MiB up the host-side packing costs more than it saves.
    {
        static const size_t kSmallCallBytes = [] { const char *e = getenv("DOA_PIPE_SMALL_CALL_KB"); return (size_t)(e ? atoi(e) : 2048) << 10; }();
        const size_t span = (size_t)(noutput_items - 1) * nonoverlap + h->K;
        const size_t span_al = (span + 1) & ~(size_t)1;       // streams two samples apart: pair-load aligned
        const size_t in_bytes = span_al * N * sb;
        const size_t n = (size_t)noutput_items;
        // sections of the result block [max | argmax | cov | spectrum], each on a 256-byte boundary (the scan kernels'
        // 16-byte stores need aligned spectrum rows)
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t pk_b = n * M * sizeof(float);
        const size_t cov_b = cov_out ? n * N * N * sizeof(float2) : 0, spec_b = spectrum_out ? n * P * sizeof(float) : 0;
        const size_t off_am = up(pk_b), off_cov = off_am + up(pk_b), off_spec = off_cov + up(cov_b);
        const size_t out_bytes = off_spec + spec_b;
        // (the gate looks at BOTH directions: a short-snapshot, long-spectrum call returns n * P * 4 bytes, and staging
        // hundreds of MiB of spectra through the page-locked buffer -- plus a host memcpy each -- is what the chunked
        // path below exists to avoid)
        if (in_bytes <= kSmallCallBytes && out_bytes <= kSmallCallBytes) {
            const size_t res_min = (size_t)h->max_batch * M * 2 * sizeof(float);
            int rc = h->h_stage.reserve(in_bytes > out_bytes ? in_bytes : out_bytes);
            if (rc == DOA_OK) rc = h->d_in[0].reserve(in_bytes);
            if (rc == DOA_OK) rc = h->d_res.reserve(out_bytes > res_min ? out_bytes : res_min);
            if (rc != DOA_OK) return rc;
            hipStream_t st = h->hst[0];
            char *hs = h->h_stage.as<char>();
            const void *d_ptrs[DOA_MAX_ANT_ELE];
            for (int k = 0; k < N; k++) {
                memcpy(hs + (size_t)k * span_al * sb, input_items[k], span * sb);
                d_ptrs[k] = h->d_in[0].as<char>() + (size_t)k * span_al * sb;
            }
            // From the upload on, every exit synchronises the stream first: a copy still reading the staging buffer
            // would race the next call's memcpy into it.
            auto staged = [&]() -> int {
                DOA_HIP_TRY(hipMemcpyAsync(h->d_in[0].p, hs, in_bytes, hipMemcpyHostToDevice, st));
                char *dr = h->d_res.as<char>();
                float *d_mx = reinterpret_cast<float *>(dr), *d_am = reinterpret_cast<float *>(dr + off_am);
                void *d_cov = cov_out ? (void *)(dr + off_cov) : h->d_cov.p;
                void *d_spec = spectrum_out ? (void *)(dr + off_spec) : nullptr;            // NULL = angles only
                const int rr = (h->fail_chunk == 0) ? (doa::set_error("music_pipeline_work: injected failure"), DOA_ERR_HIP)
                                                    : run_dev(h, noutput_items, d_ptrs, d_cov, d_spec, d_mx, d_am, 0, st, 0);
                if (rr < 0) return rr;
                // (the staging buffer is free again: the upload was enqueued before the kernels on the same stream, and
                // the download below is ordered behind them)
                DOA_HIP_TRY(hipMemcpyAsync(hs, dr, out_bytes, hipMemcpyDeviceToHost, st));
                return DOA_OK;
            };
            rc = staged();
            h->fail_chunk = -1; h->lanes.fail_batch = -1;
            const hipError_t se = hipStreamSynchronize(st);
            if (rc < 0) return rc;
            if (se != hipSuccess) { doa::set_error("music_pipeline_work: %s", hipGetErrorString(se)); return DOA_ERR_HIP; }
            memcpy(max_out, hs, pk_b);
            memcpy(argmax_out, hs + off_am, pk_b);
            if (cov_out) memcpy(cov_out, hs + off_cov, cov_b);
            if (spectrum_out) memcpy(spectrum_out, hs + off_spec, spec_b);
            return noutput_items;
        }
    }
    // Chunks of ~32 MiB of new samples alternate over two streams: while one chunk's results travel back
    // the next chunk's samples travel in (PCIe is full duplex; the kernels themselves are ~1 % of a
    // chunk's transfer time).  The overlap needs page-locked caller buffers; pageable ones still work.
    size_t chunk = ((size_t)32 << 20) / (nonoverlap * N * sb);
    chunk = chunk < 1 ? 1 : (chunk > (size_t)noutput_items ? (size_t)noutput_items : chunk);
    const size_t span_max = (chunk - 1) * nonoverlap + h->K;
    // distance between the device copies of the streams: 16-B aligned and staggered against the 8 KiB aliasing period
    const size_t stride = doa::stream_stride_bytes(span_max * sb);
    int rc = h->d_res.reserve((size_t)h->max_batch * M * 2 * sizeof(float));
    for (auto &b : h->d_in)
        if (rc == DOA_OK) rc = b.reserve(stride * N);
    if (const size_t ws = doa::autocorrelate_workspace_bytes(N, h->K, h->ovl, (int)chunk); ws && rc == DOA_OK)
        rc = h->d_work[1].reserve(ws);                 // lane 0 uses the workspace create() sized for max_batch
    if (rc != DOA_OK) return rc;
    float *d_mx = h->d_res.as<float>(), *d_am = d_mx + (size_t)h->max_batch * M;
    int lane = 0, chunk_index = 0;
    // One chunk: uploads, kernels, downloads, all on its lane's stream.  A failure anywhere in it ends the loop, and the
    // loop's exit -- normal or not -- synchronises BOTH lanes: the other lane may still be copying to or from caller-owned
    // host buffers, which must be quiet before this call returns.
    auto enqueue_chunk = [&](size_t s0, size_t n, hipStream_t st) -> int {
        const size_t span = (n - 1) * nonoverlap + h->K;
        const void *d_ptrs[DOA_MAX_ANT_ELE];
        for (int k = 0; k < N; k++) {
            char *dst = h->d_in[lane].as<char>() + k * stride;
            const char *src = static_cast<const char *>(input_items[k]) + s0 * nonoverlap * sb;
            DOA_HIP_TRY(hipMemcpyAsync(dst, src, span * sb, hipMemcpyHostToDevice, st));
            d_ptrs[k] = dst;
        }
        if (h->fail_chunk == chunk_index) { doa::set_error("music_pipeline_work: injected failure in chunk %d", chunk_index); return DOA_ERR_HIP; }
        float2 *cov = h->d_cov.as<float2>() + s0 * N * N;
        float *spec = spectrum_out ? h->d_spec.as<float>() + s0 * P : nullptr;         // NULL = angles only
        const int rr = run_dev(h, (int)n, d_ptrs, cov, spec, d_mx + s0 * M, d_am + s0 * M, s0, st, lane);
        if (rr < 0) return rr;
        if (cov_out)
            DOA_HIP_TRY(hipMemcpyAsync(static_cast<float2 *>(cov_out) + s0 * N * N, cov, n * N * N * sizeof(float2),
                                       hipMemcpyDeviceToHost, st));
        if (spectrum_out)
            DOA_HIP_TRY(hipMemcpyAsync(static_cast<float *>(spectrum_out) + s0 * P, spec, n * P * sizeof(float),
                                       hipMemcpyDeviceToHost, st));
        DOA_HIP_TRY(hipMemcpyAsync(static_cast<float *>(max_out) + s0 * M, d_mx + s0 * M, n * M * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
        DOA_HIP_TRY(hipMemcpyAsync(static_cast<float *>(argmax_out) + s0 * M, d_am + s0 * M, n * M * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
        return DOA_OK;
    };
    for (size_t s0 = 0; s0 < (size_t)noutput_items; s0 += chunk, lane ^= 1, chunk_index++) {
        const size_t n = ((size_t)noutput_items - s0 < chunk) ? (size_t)noutput_items - s0 : chunk;
        rc = enqueue_chunk(s0, n, h->hst[lane]);
        if (rc < 0) break;
    }
    h->fail_chunk = -1; h->lanes.fail_batch = -1;
    for (auto st : h->hst) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess && rc >= 0) { doa::set_error("music_pipeline_work: %s", hipGetErrorString(e)); rc = DOA_ERR_HIP; }
    }
    return rc < 0 ? rc : noutput_items;
}

int doa_music_pipeline_inject_failure(doa_music_pipeline_t *h, int chunk_index)
{
    doa::clear_error();
    if (!h || chunk_index < -1) { doa::set_error("music_pipeline_inject_failure: bad arguments"); return DOA_ERR_INVALID_ARG; }
    h->fail_chunk = chunk_index;            // whichever entry is called next consumes it: the host entry (chunk index) ...
    h->lanes.fail_batch = chunk_index;      // ... or the batches entry (batch index); both clear both
    return DOA_OK;
}

int doa_music_pipeline_lanes_idle(doa_music_pipeline_t *h)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_lanes_idle: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    for (auto st : h->hst)
        if (st && hipStreamQuery(st) != hipSuccess) return 0;
    return h->lanes.idle() ? 1 : 0;
}

int doa_music_pipeline_set_internal_precision(doa_music_pipeline_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("music_pipeline_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    if (doa::music_uses_cheb(evd_elements(h), bits)) {
        if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
        const int rc = h->d_cheb.reserve((size_t)h->max_batch * doa::kChebRecord * sizeof(double));
        if (rc != DOA_OK) return rc;
    }
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
