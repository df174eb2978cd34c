// pipeline.hip — autocorrelate -> MUSIC_lin_array -> find_local_max on device-resident streams.
//
// The batch entry point behind the benchmark: the three blocks exactly as
// apps/run_MUSIC_lin_array_simulation.grc wires them (autocorrelate(N, K, ovl, avg) ->
// MUSIC_lin_array(d, M, N, P) -> find_local_max(M, P, 0.0, 180.0)), as four launches on one
// stream: K1 covariance, K2+K3 EVD/projector/diagonal sums, K4 scan, K5 peak pick.  Intermediates
// (covariances, coefficient records, spectra) stay in HBM-resident buffers owned by the handle
// unless the caller asks for them.
#include "pipeline_front.hpp"
#include "spectrum_chain.hpp"

#include <cmath>
#include <utility>

// the front (K1, smoothing, the host entry's transport, the lanes) is doa::PipeFront's; these are the estimator stage's
struct doa_music_pipeline : doa::PipeFront {
    unsigned stages = 7;           // bit 0 K1, bit 1 K2+K3, bit 2 K4+K5 (doa_music_pipeline_set_stages)
    doa::MusicTables music;
    doa::PeakTables peaks;
    int estimator = DOA_ESTIMATOR_MUSIC;    // doa_music_pipeline_set_estimator
    double loading = 0.0;           // Capon: the diagonal loading
    bool has_table = false;         // doa_music_pipeline_set_steering_table: an arbitrary array geometry
    doa::ArrayTable array;          // its table in the scan's form (array_scan.hip)
    bool has_grid = false;          // doa_pipeline_set_steering_grid: the table's rows are an azimuth x elevation grid (has_table
    doa::Peaks2dTables grid;        // is set too) and the pick is find_local_max_2d's on these axes; argmax is [n][2 M]
    // a lane's slots after the front's: coefficient records, their Chebyshev twins, spectrum rows nobody asked for, the serial
    // peak pick's scratch, Capon's status words (int32 per item between the inverse launch and the NaN follow-up), a
    // steering-table handle's full records (N * N doubles per item between the stage in front and the scan)
    enum { kCoef = kFrontBufs, kCheb, kSpec, kScratch, kStatus, kFull };
};
static_assert(doa_music_pipeline::kFull < doa::PipeLane::kBufs, "a lane has a buffer per slot");

// what one K1 -> front -> scan chain needs besides its inputs and outputs
struct PipeWs {
    void *cov;              // covariance items, for a chain whose caller does not ask for them
    doa::SpectrumRecords rec;   // the records between the front and the scan (spectrum_chain.hpp)
    void *spec_scratch;     // P floats per item, used when the caller does not want the spectrum
    void *work;             // K1's piece sums (overlapping windows), or NULL
    void *smooth;           // spatial smoothing on: S * S gr_complex per item (else unused)
    doa::SpectrumPick pick; // the handle's axes and the scratch of the serial peak pick; a chain adds its two outputs
};

// what sizes a workspace besides the create parameters; a setter passes the configuration it is about to commit, so that a
// failure leaves the handle as it was.  Every setter that changes one of these reserves `self` for the new configuration, so
// `self` always holds the records of the configuration the handle is in.
struct MusicCfg {
    int S, bits, estimator;
    bool has_table;
};
static MusicCfg cfg_of(const doa_music_pipeline *h) { return {h->S, h->bits, h->estimator, h->has_table}; }
static doa::SpectrumPlan plan_of(const doa_music_pipeline *h, const MusicCfg &c)
{
    return doa::spectrum_plan(c.estimator, c.has_table, c.S ? c.S : h->N, c.bits, false);
}
// the chain's description of the handle as it stands (counts: work_dev_auto)
static doa::SpectrumDesc desc_of(const doa_music_pipeline *h, const doa::EvdCounts *counts = nullptr)
{
    doa::SpectrumDesc d;
    d.estimator = h->estimator; d.N = h->elements(); d.M = h->music.M; d.bits = h->bits; d.loading = h->loading;
    if (h->has_table) d.table = &h->array;
    else d.ula = &h->music;
    d.counts = counts;
    return d;
}

// K1 -> front -> scan (+ peak) -> follow-up for n items on `st` with the workspace `ws`.
// `spec` == nullptr: nobody wants the spectrum (angles-only call): ws.spec_scratch serves as scratch and the lean
// scan kernel neither converts the row to dB nor writes it.
static int run_k1(doa_music_pipeline *h, int n, const void *const *d_in, void *cov, const PipeWs &ws, hipStream_t st)
{
    if (~h->stages & 1u) return DOA_OK;         // doa_music_pipeline_set_stages (profiling aid; all stages in production)
    return h->run_k1(n, d_in, cov, ws.work, st);
}
static int run_evd_scan(doa_music_pipeline *h, int n, void *cov, void *spec, void *mx, void *am, const PipeWs &ws, hipStream_t st)
{
    const bool store_spec = (spec != nullptr);
    if (!spec) spec = ws.spec_scratch;
    const unsigned skip = ~h->stages & 7u;
    int rc = DOA_OK;
    // spatial smoothing: one launch, part of stage bit 1; the front reads the smoothed items either way
    if (!(skip & 2)) rc = h->run_smoothing(n, cov, ws.smooth, st);
    else if (h->S) cov = ws.smooth;
    if (rc != DOA_OK) return rc;
    if (h->estimator == DOA_ESTIMATOR_CAPON && h->bits != 64) {
        doa::set_error("music_pipeline: the Capon estimator needs internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->has_table && h->bits != 64) {
        doa::set_error("music_pipeline: a steering table needs internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    const doa::SpectrumDesc d = desc_of(h);
    doa::SpectrumPick pick = ws.pick;
    pick.d_max = mx; pick.d_argmax = am;
    if (!(skip & 2)) rc = doa::spectrum_front(d, n, cov, ws.rec, nullptr, st);
    if (rc == DOA_OK && !(skip & 4)) rc = doa::spectrum_scan(d, n, ws.rec, spec, nullptr, store_spec, &pick, st);
    // (with the front dropped by set_stages there is no status of this call to act on)
    if (rc == DOA_OK && !(skip & 4) && !(skip & 2)) rc = doa::spectrum_follow_up(d, n, ws.rec, store_spec ? spec : nullptr, &pick, st);
    return rc == DOA_OK ? n : rc;
}
static int run_ws(doa_music_pipeline *h, int n, const void *const *d_in, void *cov, void *spec, void *mx, void *am,
                  const PipeWs &ws, hipStream_t st)
{
    const int rc = run_k1(h, n, d_in, cov, ws, st);
    return rc != DOA_OK ? rc : run_evd_scan(h, n, cov, spec, mx, am, ws, st);
}

// The workspace `ln` (the handle's own, or a lane of work_dev_batches) as a chain sees it: records and rows from item `item_off`
// on (the host entry's chunks in flight on different streams must not share them)
static PipeWs view(doa_music_pipeline *h, doa::PipeLane &ln, size_t item_off)
{
    using H = doa_music_pipeline;
    const doa::SpectrumPlan p = plan_of(h, cfg_of(h));
    auto record = [&](int slot, size_t bytes) { return bytes ? ln.at(slot, item_off, bytes) : nullptr; };
    PipeWs ws;
    ws.cov = ln.at(H::kCov, item_off, (size_t)h->N * h->N * sizeof(float2));
    ws.rec = {record(H::kCoef, p.coef), record(H::kCheb, p.cheb), record(H::kFull, p.full), record(H::kStatus, p.status)};
    ws.spec_scratch = ln.at(H::kSpec, item_off, h->peaks.L * sizeof(float));
    ws.work = ln.buf[H::kWork].p;
    ws.smooth = ln.at(H::kSmooth, item_off, (size_t)h->S * h->S * sizeof(float2));
    ws.pick.peaks = &h->peaks; ws.pick.grid = h->has_grid ? &h->grid : nullptr;
    ws.pick.scratch = &ln.buf[H::kScratch]; ws.pick.reserve_items = (size_t)h->max_batch; ws.pick.item_off = item_off;
    return ws;
}

// Sizes `ln` for configuration `c`: records and covariances of up to G batches (64-128 B per item), spectrum rows of up to
// G_angles angles-only batches; need_cov / need_spec: some batch brings no covariance / spectrum buffer of its own.  The
// record slots come from the plan (spectrum_chain.hpp: doubles for the coefficients, G batches of Chebyshev records).
static int reserve(doa_music_pipeline *h, doa::PipeLane &ln, int G, int G_angles, bool need_cov, bool need_spec, const MusicCfg &c)
{
    using H = doa_music_pipeline;
    const size_t items = (size_t)h->max_batch;
    const doa::SpectrumPlan p = plan_of(h, c);
    int rc = h->reserve_front(ln, need_cov ? G : 0, c.S);
    if (rc == DOA_OK) rc = ln.buf[H::kCoef].reserve(items * p.coef_slot);
    if (rc == DOA_OK) rc = ln.buf[H::kCheb].reserve(G * items * p.cheb);
    if (rc == DOA_OK && need_spec) rc = ln.buf[H::kSpec].reserve(G_angles * items * h->peaks.L * sizeof(float));
    if (rc == DOA_OK) rc = ln.buf[H::kStatus].reserve(items * p.status);
    if (rc == DOA_OK) rc = ln.buf[H::kFull].reserve(items * p.full);
    return rc;
}
// the handle's own workspace: one batch, every buffer
static int reserve_self(doa_music_pipeline *h, const MusicCfg &c) { return reserve(h, h->self, 1, 1, true, true, c); }

extern "C" {

doa_music_pipeline_t *doa_music_pipeline_create(int inputs, int snapshot_size, int overlap_size, int avg_method,
                                                float norm_spacing, int num_targets, int pspectrum_len, int max_batch)
{
    doa::clear_error();
    if (!doa::PipeFront::check_create("music_pipeline", inputs, snapshot_size, overlap_size)) return nullptr;
    if (num_targets <= 0 || num_targets >= inputs || num_targets > DOA_MAX_PEAKS || !(norm_spacing > 0.0f) ||
        norm_spacing > 0.5f || pspectrum_len <= 0 || max_batch <= 0) {
        doa::set_error("music_pipeline: bad MUSIC parameters (norm_spacing=%g num_targets=%d inputs=%d "
                       "pspectrum_len=%d max_batch=%d)", (double)norm_spacing, num_targets, inputs, pspectrum_len,
                       max_batch);
        return nullptr;
    }
    return doa::create_pipeline<doa_music_pipeline>(inputs, snapshot_size, overlap_size, avg_method, max_batch, [&](doa_music_pipeline &h) {
        int rc = h.music.build(norm_spacing, num_targets, inputs, pspectrum_len);
        if (rc == DOA_OK) rc = h.peaks.build(num_targets, pspectrum_len, 0.0f, 180.0f);
        if (rc == DOA_OK) rc = reserve_self(&h, cfg_of(&h));
        return rc;
    });
}

void doa_music_pipeline_destroy(doa_music_pipeline_t *h) { doa::PipeFront::destroy(h); }

int doa_music_pipeline_fuse_antenna_correction(doa_music_pipeline_t *h, const float *gains_re_im)
{
    return doa::PipeFront::entry_fuse_antenna_correction(h, gains_re_im);
}

int doa_music_pipeline_set_input_format(doa_music_pipeline_t *h, int format, float scale)
{
    return doa::PipeFront::entry_set_input_format(h, "music_pipeline", format, scale);
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
    if (int rc = h->smoothing_args("music_pipeline_set_spatial_smoothing", h->music.M, S, forward_backward); rc != DOA_OK) return rc;
    if (S != 0 && h->has_table) {
        doa::set_error("music_pipeline_set_spatial_smoothing: smoothing assumes a translation-invariant (uniform linear) array; "
                       "this handle has a steering table");
        return DOA_ERR_UNSUPPORTED;
    }
    int rc = h->smoothing_reserve(S, fb);
    if (rc <= 0) return rc;
    rc = reserve_self(h, {S, h->bits, h->estimator, h->has_table});
    if (rc != DOA_OK) return rc;
    const int elements = S ? S : h->N;
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
    const bool capon = (estimator == DOA_ESTIMATOR_CAPON);
    if (capon && (!std::isfinite(diagonal_loading) || diagonal_loading < 0.0f)) {
        doa::set_error("music_pipeline_set_estimator: diagonal_loading must be finite and >= 0 (got %g)", (double)diagonal_loading);
        return DOA_ERR_INVALID_ARG;
    }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    if (int rc = reserve_self(h, {h->S, h->bits, estimator, h->has_table}); rc != DOA_OK) return rc;
    if (capon) h->loading = (double)diagonal_loading;
    h->estimator = estimator;
    return DOA_OK;
}

int doa_music_pipeline_set_steering_table(doa_music_pipeline_t *h, const double *steering, float x_min, float x_max)
{
    doa::clear_error();
    if (!h) { doa::set_error("music_pipeline_set_steering_table: bad arguments"); return DOA_ERR_INVALID_ARG; }
    const int N = h->N, P = h->music.P, M = h->peaks.M;
    const bool clear = !steering;                        // back to the uniform linear array and its 0 .. 180 axis
    if (clear && !h->has_table) return DOA_OK;
    if (clear) { x_min = 0.0f; x_max = 180.0f; }
    if (!std::isfinite(x_min) || !std::isfinite(x_max) || !(x_max > x_min)) {
        doa::set_error("music_pipeline_set_steering_table: need finite x_min < x_max (got %g, %g)", (double)x_min, (double)x_max);
        return DOA_ERR_INVALID_ARG;
    }
    if (!clear && !doa::steering_table_finite(steering, N, P)) {
        doa::set_error("music_pipeline_set_steering_table: the table (%d rows of %d complex doubles) holds a value that is not finite", P, N);
        return DOA_ERR_INVALID_ARG;
    }
    if (!clear && h->S) {
        doa::set_error("music_pipeline_set_steering_table: spatial smoothing is on, and it assumes a translation-invariant "
                       "(uniform linear) array");
        return DOA_ERR_UNSUPPORTED;
    }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    // everything is built aside and swapped in at the end: a failure leaves the handle as it was
    doa::ArrayTable table;
    doa::PeakTables axis;
    int rc = clear ? DOA_OK : table.build(N, P, steering);
    if (rc == DOA_OK) rc = axis.build(M, P, x_min, x_max);
    if (rc == DOA_OK) rc = reserve_self(h, {h->S, h->bits, h->estimator, !clear});
    if (rc != DOA_OK) return rc;
    h->array = std::move(table); h->peaks = std::move(axis);
    h->has_table = !clear;
    h->has_grid = false; h->grid = doa::Peaks2dTables{};     // a plain table, or none, replaces a grid
    return DOA_OK;
}

int doa_pipeline_set_steering_grid(doa_music_pipeline_t *h, const double *steering, int n_az, int n_el, float az_min, float az_max,
                                   float el_min, float el_max, int wrap_az)
{
    doa::clear_error();
    const char *who = "pipeline_set_steering_grid";
    if (!h) { doa::set_error("%s: bad arguments (NULL handle)", who); return DOA_ERR_INVALID_ARG; }
    const int N = h->N, P = h->music.P, M = h->music.M;
    if (!doa::peaks2d_args_ok(who, M, n_az, n_el, az_min, az_max, el_min, el_max)) return DOA_ERR_INVALID_ARG;
    if ((long long)n_az * n_el != P) {
        doa::set_error("%s: the grid %d x %d does not have the handle's pspectrum_len = %d cells", who, n_az, n_el, P);
        return DOA_ERR_INVALID_ARG;
    }
    if (!doa::steering_table_finite(steering, N, P)) {
        doa::set_error("%s: the table (%d rows of %d complex doubles) is NULL or holds a value that is not finite", who, P, N);
        return DOA_ERR_INVALID_ARG;
    }
    if (h->S) {
        doa::set_error("%s: spatial smoothing is on, and it assumes a translation-invariant (uniform linear) array", who);
        return DOA_ERR_UNSUPPORTED;
    }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    // built aside and swapped in at the end: a failure leaves the handle as it was.  The one-dimensional axis (h->peaks) stays:
    // nothing reads it in grid mode but its length, and both ways out of grid mode rebuild it
    doa::ArrayTable table;
    doa::Peaks2dTables axes;
    int rc = table.build(N, P, steering);
    if (rc == DOA_OK) rc = axes.build(M, n_az, n_el, az_min, az_max, el_min, el_max, wrap_az);
    if (rc == DOA_OK) rc = reserve_self(h, {h->S, h->bits, h->estimator, true});
    if (rc != DOA_OK) return rc;
    h->array = std::move(table); h->grid = std::move(axes);
    h->has_table = true; h->has_grid = true;
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
    const PipeWs ws = view(h, h->self, 0);
    // (no spectrum = angles only)
    return run_ws(h, noutput_items, d_input_items, d_cov_out ? d_cov_out : ws.cov, d_spectrum_out, d_max_out, d_argmax_out, ws,
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
    int rc = reserve_self(h, cfg_of(h));
    if (rc != DOA_OK) return rc;
    const PipeWs ws = view(h, h->self, 0);
    void *cov = d_cov_out ? d_cov_out : ws.cov;
    void *spec = d_spectrum_out ? d_spectrum_out : ws.spec_scratch;
    rc = run_k1(h, n, d_input_items, cov, ws, st);
    if (rc == DOA_OK) rc = h->run_smoothing(n, cov, ws.smooth, st);
    const doa::EvdCounts cnt = doa::evd_counts_estimate((int *)d_count_out, (float *)d_eig_out, h->K, method, h->music.M);
    const doa::SpectrumDesc d = desc_of(h, &cnt);
    if (rc == DOA_OK) rc = doa::spectrum_front(d, n, cov, ws.rec, nullptr, st);
    if (rc == DOA_OK) rc = doa::spectrum_scan(d, n, ws.rec, spec, nullptr, true, nullptr, st);
    // a spectrum the caller sees: the row of a count -1 item is NaN, as MUSIC_lin_array_work_dev_counts leaves it (a fifth,
    // one-load-per-item launch; the peak pick below does not read the rows of such items)
    if (rc == DOA_OK) rc = doa::spectrum_follow_up(d, n, ws.rec, d_spectrum_out, nullptr, st);
    if (rc == DOA_OK)
        rc = doa::launch_peak_pick(h->peaks, n, spec, d_count_out, d_max_out, d_argmax_out, *ws.pick.scratch, (size_t)h->max_batch, 0, st);
    return rc == DOA_OK ? n : rc;
}

int doa_music_pipeline_set_lanes(doa_music_pipeline_t *h, int n_lanes)
{
    return doa::PipeFront::entry_set_lanes(h, "music_pipeline", n_lanes);
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

    // ---- the plan (batch_plan.hpp): what makes a batch lean, and its group cap ----
    const bool lean_shape = h->estimator == DOA_ESTIMATOR_MUSIC && !h->has_table && h->S == 0 && h->ovl == 0 && h->peaks.L == h->music.P && doa::group_routes_accept(N, h->music.M, P, h->bits) &&
                            (long long)doa::kMaxGroup * n <= (1 << 28);
    const int L_all = h->lanes.n_lanes;
    const int L = (lean_shape && group_lanes() < L_all) ? group_lanes() : L_all;
    const int G = lean_shape ? group_batches(L) : 1;
    const size_t angles_rows = kAnglesScratchBytes / ((size_t)h->max_batch * P * sizeof(float));
    const int G_angles = (int)(angles_rows < 1 ? 1 : (angles_rows > (size_t)G ? (size_t)G : angles_rows));
    auto traits = [&](int b, doa::PlanGroup &nb, const void *(&out)[4]) {
        out[0] = d_cov_out ? d_cov_out[b] : nullptr; out[1] = d_spectrum_out ? d_spectrum_out[b] : nullptr;
        out[2] = d_max_out[b]; out[3] = d_argmax_out[b];
        nb.store = (out[1] != nullptr);
        nb.lean = lean_shape && reinterpret_cast<uintptr_t>(out[1]) % 16 == 0;
        nb.vec2 = nb.lean && doa::autocorrelate_pair_loads(N, h->K, h->ovl, d_input_items + (size_t)b * N, h->fmt.format);
        nb.cap = !nb.lean ? 1 : (nb.store ? G : G_angles);
        if (b == 0 && group_first() > 0 && group_first() < nb.cap) nb.cap = group_first();
    };

    // ---- workspaces and launches ----
    const bool need_cov = doa::PipeLanes::lacks(d_cov_out, n_batches), need_spec = doa::PipeLanes::lacks(d_spectrum_out, n_batches);
    // a lane's buffers hold a whole group; the angles-only scratch rows are bounded (G_angles)
    auto prepare = [&](doa::PipeLane &ln) { return reserve(h, ln, G, G_angles, need_cov, need_spec, cfg_of(h)); };
    auto launch = [&](const doa::PlanGroup &g, doa::PipeLane &ln) -> int {
        const PipeWs ws = view(h, ln, 0);
        if (!g.lean || g.nb == 1) {                              // one batch: the launches of work_dev
            int rc = DOA_OK;
            for (int b = g.b0; b < g.b0 + g.nb && rc >= 0; b++) {
                void *cov = (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : ws.cov;
                rc = run_ws(h, n, d_input_items + (size_t)b * N, cov, d_spectrum_out ? d_spectrum_out[b] : nullptr, d_max_out[b],
                            d_argmax_out[b], ws, ln.st);
            }
            return rc;
        }
        doa::BatchGroup grp;
        grp.n_batches = g.nb; grp.n = n;
        for (int k = 0; k < g.nb; k++) {
            const int b = g.b0 + k;
            grp.in[k] = d_input_items + (size_t)b * N;
            grp.cov[k] = (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : static_cast<char *>(ws.cov) + (size_t)k * n * N * N * sizeof(float2);
            grp.spec[k] = g.store ? d_spectrum_out[b] : static_cast<char *>(ws.spec_scratch) + (size_t)k * n * P * sizeof(float);
            grp.mx[k] = d_max_out[b]; grp.am[k] = d_argmax_out[b];
        }
        const unsigned skip = ~h->stages & 7u;                   // doa_music_pipeline_set_stages
        int rc = DOA_OK;
        if (!(skip & 1)) rc = doa::launch_autocorrelate_group(N, h->K, h->avg, grp, ln.st, h->has_gain ? h->d_gain.p : nullptr, h->fmt.format, h->fmt.scale);
        if (rc == DOA_OK && !(skip & 2)) rc = doa::launch_music_evd_group(N, h->music.M, grp, nullptr, ws.rec.cheb, ln.st);
        if (rc == DOA_OK && !(skip & 4)) rc = doa::launch_music_scan_group(h->music, h->peaks, grp, ws.rec.cheb, g.store, ln.st);
        return rc;
    };
    const int rc = h->run_planned("music_pipeline_work_dev_batches", n_batches, L, hip_stream, traits, prepare, launch);
    return rc < 0 ? rc : n_batches * n;
}

int doa_music_pipeline_set_lane_streams(doa_music_pipeline_t *h, int n_lanes, void *const *hip_streams)
{
    return doa::PipeFront::entry_set_lane_streams(h, "music_pipeline", n_lanes, hip_streams);
}

int doa_music_pipeline_synchronize(doa_music_pipeline_t *h)
{
    return doa::PipeFront::entry_synchronize(h, "music_pipeline");
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
    const char *who = "music_pipeline_work";
    if (const int rc = h->host_open(who, input_items); rc != DOA_OK) return rc;
    const size_t N = h->N, M = h->music.M, P = h->peaks.L;
    // [max | argmax | cov | spectrum]; on the chunked path the peaks lie in the transport's result block, the covariances
    // and spectra in the handle's own workspace at their item offsets
    using H = doa_music_pipeline;
    const size_t am_floats = h->has_grid ? 2 * M : M;           // grid mode: M azimuths, then M elevations
    const doa::HostSection sec[4] = {{max_out, M * sizeof(float), nullptr}, {argmax_out, am_floats * sizeof(float), nullptr},
                                     {cov_out, N * N * sizeof(float2), h->self.buf[H::kCov].p},
                                     {spectrum_out, P * sizeof(float), h->self.buf[H::kSpec].p}};
    return h->host_run(who, noutput_items, input_items, sec, 4,
                       [h](int n, const void *const *d_in, size_t item_off, void *const *d_sec, hipStream_t st, int lane) {
                           PipeWs ws = view(h, h->self, item_off);
                           ws.work = h->host_work(lane);
                           // (no spectrum section = angles only)
                           return run_ws(h, n, d_in, d_sec[2] ? d_sec[2] : ws.cov, d_sec[3], d_sec[0], d_sec[1], ws, st);
                       });
}

int doa_music_pipeline_inject_failure(doa_music_pipeline_t *h, int chunk_index)
{
    return doa::PipeFront::entry_inject_failure(h, "music_pipeline", chunk_index);
}

int doa_music_pipeline_lanes_idle(doa_music_pipeline_t *h)
{
    return doa::PipeFront::entry_lanes_idle(h, "music_pipeline");
}

int doa_music_pipeline_set_internal_precision(doa_music_pipeline_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("music_pipeline_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    if (const int rc = reserve_self(h, {h->S, bits, h->estimator, h->has_table}); rc != DOA_OK) return rc;
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
