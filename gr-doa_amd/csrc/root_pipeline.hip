// root_pipeline.hip — autocorrelate -> rootMUSIC_linear_array on device-resident streams: the Root-MUSIC branch of the hot
// path as ONE handle, the chain apps/run_RootMUSIC_lin_array_simulation.grc wires (autocorrelate(N, K, ovl, avg) ->
// rootMUSIC_linear_array(d, M, N); reference work being chained: lib/autocorrelate_impl.cc:83-118 ->
// lib/rootMUSIC_linear_array_impl.cc:90-152).  Three launches per batch -- K1 covariance, K2+K3 EVD / projector / diagonal
// sums (double records), K6 roots + selection -- with the same entry points, lanes, detached form and error contract as
// music_pipeline (pipeline.hip, pipeline_lanes.hpp).  Until round 4 this branch had to be driven as two block handles and
// two calls per batch, which left it host-bound above ~20 us per 4096-snapshot step.
#include "pipeline_front.hpp"

// the front (K1, smoothing, the host entry's transport, the lanes) is doa::PipeFront's; these are the estimator stage's
struct doa_root_pipeline : doa::PipeFront {
    int M = 0;
    float norm_spacing = 0.f;
    doa::DevBuf d_coef, d_status;
    int estimator = DOA_GRIDFREE_ROOT_MUSIC;    // doa_root_pipeline_set_estimator
    doa::DevBuf d_rec;              // ESPRIT mode: the signal-subspace records between the eigen launch and esprit_kernel
    doa::PinnedBuf h_status;        // host-pointer entry point: the items' status words, scanned after the call's copies
    enum { kCoef = 0, kCov, kStatus, kWork, kSmooth, kRec };    // doa_root_pipeline_work_dev_batches: a lane's buffers
};

namespace {
struct RootWs {
    void *coef;       // double coefficient records of the chain's items
    void *status;     // one int per item (1 = no root strictly inside the unit circle), or the caller's buffer
    void *work;       // K1's piece sums (overlapping windows), or NULL
    void *smooth;     // spatial smoothing on: S * S gr_complex per item (else unused)
    void *rec;        // ESPRIT mode: signal-subspace records of the chain's items (else unused)
};
size_t coef_bytes(const doa_root_pipeline *h, size_t items) { return items * doa::coef_stride(h->N) * sizeof(double); }
// (sized for the full array: a later set_spatial_smoothing only makes the records smaller)
size_t rec_bytes(const doa_root_pipeline *h, size_t items) { return items * doa::subspace_record_len(h->N) * sizeof(double); }
bool esprit_mode(const doa_root_pipeline *h) { return h->estimator == DOA_GRIDFREE_ESPRIT; }
int esprit_precision(const char *who, const doa_root_pipeline *h)
{
    if (!esprit_mode(h) || h->bits == 64) return DOA_OK;
    doa::set_error("%s: ESPRIT needs internal precision 64 (handle is at %d)", who, h->bits);
    return DOA_ERR_UNSUPPORTED;
}

// K1 -> EVD -> roots for n items on `st`
int run_chain(doa_root_pipeline *h, int n, const void *const *d_in, void *cov, void *angles, const RootWs &ws, hipStream_t st)
{
    int rc = h->run_k1(n, d_in, cov, ws.work, st);
    if (rc == DOA_OK) rc = h->run_smoothing(n, cov, ws.smooth, st);
    if (rc != DOA_OK) return rc;
    const int elements = h->elements();
    if (esprit_mode(h)) {                       // the eigen launch that writes the record, then esprit_kernel
        rc = doa::launch_music_evd_record(elements, n, cov, ws.rec, st);
        if (rc != DOA_OK) return rc;
        rc = doa::launch_esprit(elements, h->M, h->norm_spacing, n, cov, ws.rec, nullptr, angles, ws.status, st);
        return rc == DOA_OK ? n : rc;
    }
    rc = doa::launch_music_evd(elements, h->M, n, cov, nullptr, ws.coef, nullptr, h->bits, st);
    if (rc != DOA_OK) return rc;
    rc = doa::launch_root_music(elements, h->M, h->norm_spacing, n, ws.coef, angles, ws.status, st);
    return rc == DOA_OK ? n : rc;
}
// first item whose status word is set, or -1
int first_flagged(const int *status, int n)
{
    for (int i = 0; i < n; i++)
        if (status[i] != 0) return i;
    return -1;
}
int numeric_error(const doa_root_pipeline *h, int item, int status)
{
    if (esprit_mode(h)) {
        doa::set_error("root_pipeline: ESPRIT item %d has status %d (1 = not solvable, 3 = eigenvalue iteration cap)", item, status);
        return DOA_ERR_NUMERIC;
    }
    doa::set_error("root_pipeline: item %d has no root strictly inside the unit circle (the reference raises in "
                   "arma::index_min here, lib/rootMUSIC_linear_array_impl.cc:129)", item);
    return DOA_ERR_NUMERIC;
}
}  // namespace

extern "C" {

doa_root_pipeline_t *doa_root_pipeline_create(int inputs, int snapshot_size, int overlap_size, int avg_method,
                                              float norm_spacing, int num_targets, int max_batch)
{
    doa::clear_error();
    if (!doa::PipeFront::check_create("root_pipeline", inputs, snapshot_size, overlap_size)) return nullptr;
    if (inputs < 2 || num_targets <= 0 || num_targets >= inputs || num_targets > DOA_MAX_PEAKS || !(norm_spacing > 0.0f) ||
        norm_spacing > 0.5f || max_batch <= 0) {
        doa::set_error("root_pipeline: bad Root-MUSIC parameters (norm_spacing=%g num_targets=%d inputs=%d max_batch=%d)",
                       (double)norm_spacing, num_targets, inputs, max_batch);
        return nullptr;
    }
    return doa::create_pipeline<doa_root_pipeline>(inputs, snapshot_size, overlap_size, avg_method, max_batch, [&](doa_root_pipeline &h) {
        h.M = num_targets; h.norm_spacing = norm_spacing;
        int rc = h.d_coef.reserve(coef_bytes(&h, (size_t)max_batch));
        if (rc == DOA_OK) rc = h.d_status.reserve((size_t)max_batch * sizeof(int));
        return rc;
    });
}

void doa_root_pipeline_destroy(doa_root_pipeline_t *h) { doa::PipeFront::destroy(h); }

int doa_root_pipeline_fuse_antenna_correction(doa_root_pipeline_t *h, const float *gains_re_im)
{
    doa::clear_error();
    if (!h) return DOA_ERR_INVALID_ARG;
    return h->fuse_antenna_correction(gains_re_im);
}

int doa_root_pipeline_set_input_format(doa_root_pipeline_t *h, int format, float scale)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_set_input_format: bad arguments"); return DOA_ERR_INVALID_ARG; }
    return h->set_input_format("root_pipeline", format, scale);
}

int doa_root_pipeline_set_spatial_smoothing(doa_root_pipeline_t *h, int subarray_size, int forward_backward)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_set_spatial_smoothing: bad arguments"); return DOA_ERR_INVALID_ARG; }
    const int S = subarray_size, fb = S ? forward_backward : 0;
    if (int rc = h->smoothing_args("root_pipeline_set_spatial_smoothing", h->M, S, forward_backward); rc != DOA_OK) return rc;
    if (int rc = h->smoothing_reserve(S, fb); rc <= 0) return rc;
    h->S = S; h->fb = fb;
    return DOA_OK;
}

int doa_root_pipeline_set_estimator(doa_root_pipeline_t *h, int estimator)
{
    doa::clear_error();
    if (!h || (estimator != DOA_GRIDFREE_ROOT_MUSIC && estimator != DOA_GRIDFREE_ESPRIT)) {
        doa::set_error("root_pipeline_set_estimator: need a handle and DOA_GRIDFREE_ROOT_MUSIC or DOA_GRIDFREE_ESPRIT (got %d)", estimator);
        return DOA_ERR_INVALID_ARG;
    }
    if (estimator == h->estimator) return DOA_OK;
    if (estimator == DOA_GRIDFREE_ESPRIT) {
        // work_dev / work_dev_auto and the host entry (whose chunks lie at their item offsets) share this one; the lanes of
        // work_dev_batches have their own (kRec)
        if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
        if (int rc = h->d_rec.reserve(rec_bytes(h, (size_t)h->max_batch)); rc != DOA_OK) return rc;
    }
    h->estimator = estimator;
    return DOA_OK;
}

int doa_root_pipeline_work_dev(doa_root_pipeline_t *h, int noutput_items, const void *const *d_input_items, void *d_cov_out,
                               void *d_angles_out, int *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || !d_input_items || (noutput_items > 0 && !d_angles_out)) {
        doa::set_error("root_pipeline_work_dev: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("root_pipeline_work_dev: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    if (int prc = esprit_precision("root_pipeline_work_dev", h); prc != DOA_OK) return prc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    RootWs ws{h->d_coef.p, d_status_out ? (void *)d_status_out : h->d_status.p, h->d_work[0].p, h->d_smooth.p, h->d_rec.p};
    return run_chain(h, noutput_items, d_input_items, d_cov_out ? d_cov_out : h->d_cov.p, d_angles_out, ws,
                     static_cast<hipStream_t>(hip_stream));
}

// K1 as work_dev runs it, ONE eigen launch that estimates each item's count and writes its record for the noise set that
// count gives, the counted root kernel: three launches, four on a smoothed handle
int doa_root_pipeline_work_dev_auto(doa_root_pipeline_t *h, int noutput_items, const void *const *d_input_items, int method,
                                    void *d_cov_out, void *d_angles_out, void *d_count_out, void *d_eig_out, int *d_status_out,
                                    void *hip_stream)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || !d_input_items || (method != DOA_SOURCE_COUNT_MDL && method != DOA_SOURCE_COUNT_AIC) ||
        (noutput_items > 0 && (!d_angles_out || !d_count_out))) {
        doa::set_error("root_pipeline_work_dev_auto: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("root_pipeline_work_dev_auto: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    if (h->bits != 64) {
        doa::set_error("root_pipeline_work_dev_auto: per-item counts need internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->K < 2) {
        doa::set_error("root_pipeline_work_dev_auto: the criterion needs snapshot_size >= 2 (handle has %d)", h->K);
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int n = noutput_items;
    const int elements = h->elements();
    void *cov = d_cov_out ? d_cov_out : h->d_cov.p;
    int rc = h->run_k1(n, d_input_items, cov, h->d_work[0].p, st);
    if (rc == DOA_OK) rc = h->run_smoothing(n, cov, h->d_smooth.p, st);
    if (rc == DOA_OK && esprit_mode(h)) {       // one estimating eigen launch (counts, eigenvalues, record), the counted ESPRIT kernel
        rc = doa::launch_music_evd_counts(elements, n, cov, nullptr, d_count_out, d_eig_out, h->K, method, h->M, nullptr, nullptr, st,
                                          h->d_rec.p);
        if (rc == DOA_OK)
            rc = doa::launch_esprit(elements, h->M, h->norm_spacing, n, cov, h->d_rec.p, d_count_out, d_angles_out,
                                    d_status_out ? (void *)d_status_out : h->d_status.p, st);
        return rc == DOA_OK ? n : rc;
    }
    if (rc == DOA_OK)
        rc = doa::launch_music_evd_counts(elements, n, cov, nullptr, d_count_out, d_eig_out, h->K, method, h->M, h->d_coef.p, nullptr, st);
    if (rc == DOA_OK)
        rc = doa::launch_root_music_counts(elements, h->M, h->norm_spacing, n, h->d_coef.p, d_count_out, d_angles_out,
                                           d_status_out ? (void *)d_status_out : h->d_status.p, st);
    return rc == DOA_OK ? n : rc;
}

int doa_root_pipeline_set_lanes(doa_root_pipeline_t *h, int n_lanes)
{
    doa::clear_error();
    if (!h || h->lanes.set_count(n_lanes) != DOA_OK) {
        doa::set_error("root_pipeline_set_lanes: need 1 <= n_lanes <= %d", doa::PipeLanes::kMaxLanes);
        return DOA_ERR_INVALID_ARG;
    }
    return DOA_OK;
}

int doa_root_pipeline_set_lane_streams(doa_root_pipeline_t *h, int n_lanes, void *const *hip_streams)
{
    doa::clear_error();
    if (!h || n_lanes < 1 || n_lanes > doa::PipeLanes::kMaxLanes || !hip_streams) {
        doa::set_error("root_pipeline_set_lane_streams: need 1 <= n_lanes <= %d and the streams", doa::PipeLanes::kMaxLanes);
        return DOA_ERR_INVALID_ARG;
    }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    return h->lanes.adopt(n_lanes, hip_streams);
}

int doa_root_pipeline_synchronize(doa_root_pipeline_t *h)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_synchronize: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    return h->lanes.synchronize();
}

int doa_root_pipeline_work_dev_batches(doa_root_pipeline_t *h, int n_batches, int noutput_items, const void *const *d_input_items,
                                       void *const *d_cov_out, void *const *d_angles_out, int *const *d_status_out,
                                       void *hip_stream)
{
    doa::clear_error();
    if (!h || n_batches < 0 || noutput_items < 0 || !d_input_items || !d_angles_out) {
        doa::set_error("root_pipeline_work_dev_batches: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("root_pipeline_work_dev_batches: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    for (int b = 0; b < n_batches; b++)
        if (noutput_items > 0 && !d_angles_out[b]) {
            doa::set_error("root_pipeline_work_dev_batches: batch %d has no angle output pointer", b);
            return DOA_ERR_INVALID_ARG;
        }
    if (int prc = esprit_precision("root_pipeline_work_dev_batches", h); prc != DOA_OK) return prc;
    if (n_batches == 0 || noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int N = h->N;
    const int fail_at = h->lanes.fail_batch;
    h->fail_chunk = -1;
    if (h->lanes.n_lanes == 1 && hip_stream != DOA_STREAM_DETACHED) {     // nothing to overlap: the caller's stream itself, no events
        hipStream_t caller = static_cast<hipStream_t>(hip_stream);
        h->lanes.fail_batch = -1;
        for (int b = 0; b < n_batches; b++) {
            if (fail_at == b) {
                doa::set_error("root_pipeline_work_dev_batches: injected failure in batch %d", b);
                (void)hipStreamSynchronize(caller);
                return DOA_ERR_HIP;
            }
            RootWs ws{h->d_coef.p, (d_status_out && d_status_out[b]) ? (void *)d_status_out[b] : h->d_status.p, h->d_work[0].p,
                      h->d_smooth.p, h->d_rec.p};
            const int rc = run_chain(h, noutput_items, d_input_items + (size_t)b * N,
                                     (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : h->d_cov.p, d_angles_out[b], ws, caller);
            if (rc < 0) { (void)hipStreamSynchronize(caller); return rc; }
        }
        return n_batches * noutput_items;
    }
    bool need_cov = !d_cov_out, need_status = !d_status_out;
    for (int b = 0; b < n_batches && !(need_cov && need_status); b++) {
        if (d_cov_out && !d_cov_out[b]) need_cov = true;
        if (d_status_out && !d_status_out[b]) need_status = true;
    }
    const size_t work_bytes = doa::autocorrelate_workspace_bytes(N, h->K, h->ovl, h->max_batch);
    using H = doa_root_pipeline;
    auto prepare = [&](doa::PipeLane &ln) -> int {
        int rc = ln.buf[H::kCoef].reserve(coef_bytes(h, (size_t)h->max_batch));
        if (rc == DOA_OK && need_cov) rc = ln.buf[H::kCov].reserve((size_t)h->max_batch * N * N * sizeof(float2));
        if (rc == DOA_OK && need_status) rc = ln.buf[H::kStatus].reserve((size_t)h->max_batch * sizeof(int));
        if (rc == DOA_OK && work_bytes) rc = ln.buf[H::kWork].reserve(work_bytes);
        if (rc == DOA_OK && h->S) rc = ln.buf[H::kSmooth].reserve((size_t)h->max_batch * h->S * h->S * sizeof(float2));
        if (rc == DOA_OK && esprit_mode(h)) rc = ln.buf[H::kRec].reserve(rec_bytes(h, (size_t)h->max_batch));
        return rc;
    };
    auto launch = [&](int b, doa::PipeLane &ln) -> int {
        RootWs ws{ln.buf[H::kCoef].p, (d_status_out && d_status_out[b]) ? (void *)d_status_out[b] : ln.buf[H::kStatus].p,
                  ln.buf[H::kWork].p, ln.buf[H::kSmooth].p, ln.buf[H::kRec].p};
        return run_chain(h, noutput_items, d_input_items + (size_t)b * N,
                         (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : ln.buf[H::kCov].p, d_angles_out[b], ws, ln.st);
    };
    const int rc = h->lanes.run_batches("root_pipeline_work_dev_batches", n_batches, hip_stream, prepare, launch);
    return rc < 0 ? rc : n_batches * noutput_items;
}

int doa_root_pipeline_work(doa_root_pipeline_t *h, int noutput_items, const void *const *input_items, void *cov_out,
                           void *angles_out)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || !input_items || (noutput_items > 0 && !angles_out)) {
        doa::set_error("root_pipeline_work: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items > h->max_batch) {
        doa::set_error("root_pipeline_work: noutput_items=%d exceeds max_batch=%d", noutput_items, h->max_batch);
        return DOA_ERR_INVALID_ARG;
    }
    if (int prc = esprit_precision("root_pipeline_work", h); prc != DOA_OK) return prc;
    if (noutput_items == 0) return 0;
    const char *who = "root_pipeline_work";
    if (const int rc = h->host_open(who, input_items); rc != DOA_OK) return rc;
    if (const int rc = h->h_status.reserve((size_t)noutput_items * sizeof(int)); rc != DOA_OK) return rc;
    const size_t N = h->N;
    // [angles | status | cov]; on the chunked path angles and status words lie in the transport's result block, the
    // covariances in the handle's own d_cov at their item offsets
    const doa::HostSection sec[3] = {{angles_out, h->M * sizeof(float), nullptr}, {h->h_status.p, sizeof(int), nullptr},
                                     {cov_out, N * N * sizeof(float2), h->d_cov.p}};
    const int rc = h->host_run(who, noutput_items, input_items, sec, 3,
                               [h](int n, const void *const *d_in, size_t item_off, void *const *d_sec, hipStream_t st, int lane) {
        // (the two copy/compute lanes write disjoint item ranges of the handle's records and smoothed items)
        RootWs ws{h->d_coef.as<char>() + coef_bytes(h, item_off), d_sec[1], h->d_work[lane].p,
                  h->S ? (void *)(h->d_smooth.as<float2>() + item_off * h->S * h->S) : nullptr,
                  esprit_mode(h) ? (void *)(h->d_rec.as<char>() + rec_bytes(h, item_off)) : nullptr};
        void *cov = d_sec[2] ? d_sec[2] : h->d_cov.as<float2>() + item_off * h->N * h->N;
        return run_chain(h, n, d_in, cov, d_sec[0], ws, st);
    });
    if (rc < 0) return rc;
    // the other items' outputs are valid
    if (const int bad = first_flagged(h->h_status.as<int>(), noutput_items); bad >= 0) return numeric_error(h, bad, h->h_status.as<int>()[bad]);
    return noutput_items;
}

int doa_root_pipeline_inject_failure(doa_root_pipeline_t *h, int chunk_index)
{
    doa::clear_error();
    if (!h || chunk_index < -1) { doa::set_error("root_pipeline_inject_failure: bad arguments"); return DOA_ERR_INVALID_ARG; }
    return h->inject_failure(chunk_index);
}

int doa_root_pipeline_lanes_idle(doa_root_pipeline_t *h)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_lanes_idle: bad arguments"); return DOA_ERR_INVALID_ARG; }
    return h->lanes_idle();
}

int doa_root_pipeline_set_internal_precision(doa_root_pipeline_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("root_pipeline_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
