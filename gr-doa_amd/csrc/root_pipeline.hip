// root_pipeline.hip — autocorrelate -> rootMUSIC_linear_array on device-resident streams: the Root-MUSIC branch of the hot
// path as ONE handle, the chain apps/run_RootMUSIC_lin_array_simulation.grc wires (autocorrelate(N, K, ovl, avg) ->
// rootMUSIC_linear_array(d, M, N); reference work being chained: lib/autocorrelate_impl.cc:83-118 ->
// lib/rootMUSIC_linear_array_impl.cc:90-152).  Three launches per batch -- K1 covariance, K2+K3 EVD / projector / diagonal
// sums (double records), K6 roots + selection -- with the same entry points, lanes, detached form and error contract as
// music_pipeline (pipeline.hip, pipeline_lanes.hpp).  Until round 4 this branch had to be driven as two block handles and
// two calls per batch, which left it host-bound above ~20 us per 4096-snapshot step.
#include "kernels.hpp"
#include "pipeline_lanes.hpp"

#include <cstdlib>
#include <cstring>

struct doa_root_pipeline {
    int N = 0, K = 0, ovl = 0, avg = 0, M = 0;
    float norm_spacing = 0.f;
    int max_batch = 0;
    int bits = 64;
    int device = 0;
    doa::DevBuf d_cov, d_coef, d_status, d_gain;
    bool has_gain = false;
    int format = DOA_SAMPLE_FC32;   // doa_root_pipeline_set_input_format
    float scale = 1.0f;
    int S = 0, fb = 0;              // doa_root_pipeline_set_spatial_smoothing: subarray size (0 = off), forward-backward
    doa::DevBuf d_smooth;           // the smoothed items (S * S per item) between K1 and the eigen stage (max_batch items)
    int estimator = DOA_GRIDFREE_ROOT_MUSIC;    // doa_root_pipeline_set_estimator
    doa::DevBuf d_rec;              // ESPRIT mode: the signal-subspace records between the eigen launch and esprit_kernel
    // host-pointer entry point only: two copy/compute lanes
    hipStream_t hst[2] = {nullptr, nullptr};
    doa::DevBuf d_in[2], d_res;
    doa::DevBuf d_work[2];
    doa::PinnedBuf h_stage, h_status;
    int fail_chunk = -1;
    enum { kCoef = 0, kCov, kStatus, kWork, kSmooth, kRec };
    doa::PipeLanes lanes;
};

namespace {
struct RootWs {
    void *coef;       // double coefficient records of the chain's items
    void *status;     // one int per item (1 = no root strictly inside the unit circle), or the caller's buffer
    void *work;       // K1's piece sums (overlapping windows), or NULL
    void *smooth;     // spatial smoothing on: S * S gr_complex per item (else unused)
    void *rec;        // ESPRIT mode: signal-subspace records of the chain's items (else unused)
};
// the array the eigen stage and the root finder see: the subarray of a smoothed handle
int evd_elements(const doa_root_pipeline *h) { return h->S ? h->S : h->N; }
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
    int rc = doa::launch_autocorrelate(h->N, h->K, h->ovl, h->avg, n, d_in, cov, st, h->has_gain ? h->d_gain.p : nullptr, ws.work,
                                       h->format, h->scale);
    if (rc != DOA_OK) return rc;
    if (h->S) {                                 // spatial smoothing: one launch; `cov` stays the N x N item
        rc = doa::launch_spatial_smooth(h->N, h->S, h->fb, n, cov, ws.smooth, st);
        if (rc != DOA_OK) return rc;
        cov = ws.smooth;
    }
    const int elements = evd_elements(h);
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
    if (inputs <= 0 || inputs > DOA_MAX_ANT_ELE || snapshot_size <= 0 || overlap_size < 0 || overlap_size >= snapshot_size) {
        doa::set_error("root_pipeline: bad autocorrelate parameters (inputs=%d snapshot=%d overlap=%d)", inputs, snapshot_size,
                       overlap_size);
        return nullptr;
    }
    if (inputs < 2 || num_targets <= 0 || num_targets >= inputs || num_targets > DOA_MAX_PEAKS || !(norm_spacing > 0.0f) ||
        norm_spacing > 0.5f || max_batch <= 0) {
        doa::set_error("root_pipeline: bad Root-MUSIC parameters (norm_spacing=%g num_targets=%d inputs=%d max_batch=%d)",
                       (double)norm_spacing, num_targets, inputs, max_batch);
        return nullptr;
    }
    int dev = 0;
    if (doa::ensure_device(&dev) != DOA_OK) return nullptr;
    auto *h = new (std::nothrow) doa_root_pipeline();
    if (!h) { doa::set_error("out of memory"); return nullptr; }
    h->N = inputs; h->K = snapshot_size; h->ovl = overlap_size; h->avg = avg_method; h->M = num_targets;
    h->norm_spacing = norm_spacing; h->max_batch = max_batch; h->device = dev;
    h->bits = doa::internal_precision_bits();
    int rc = h->d_cov.reserve((size_t)max_batch * inputs * inputs * sizeof(float2));
    if (rc == DOA_OK) rc = h->d_coef.reserve(coef_bytes(h, (size_t)max_batch));
    if (rc == DOA_OK) rc = h->d_status.reserve((size_t)max_batch * sizeof(int));
    if (const size_t ws = doa::autocorrelate_workspace_bytes(inputs, snapshot_size, overlap_size, max_batch); ws && rc == DOA_OK)
        rc = h->d_work[0].reserve(ws);
    if (rc != DOA_OK) {
        doa_root_pipeline_destroy(h);
        return nullptr;
    }
    return h;
}

void doa_root_pipeline_destroy(doa_root_pipeline_t *h)
{
    if (!h) return;
    h->d_cov.release(); h->d_coef.release(); h->d_status.release(); h->d_gain.release(); h->d_res.release();
    h->h_stage.release(); h->h_status.release();
    h->d_smooth.release(); h->d_rec.release();
    for (auto &b : h->d_work) b.release();
    for (auto &b : h->d_in) b.release();
    for (auto st : h->hst)
        if (st) (void)hipStreamDestroy(st);
    h->lanes.release();
    delete h;
}

int doa_root_pipeline_fuse_antenna_correction(doa_root_pipeline_t *h, const float *gains_re_im)
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
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    int rc = h->d_gain.reserve(sizeof(float2) * N * N);
    if (rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(h->d_gain.p, w, sizeof(float2) * N * N, hipMemcpyHostToDevice));
    h->has_gain = true;
    return DOA_OK;
}

int doa_root_pipeline_set_input_format(doa_root_pipeline_t *h, int format, float scale)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_set_input_format: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (const int rc = doa::check_input_format("root_pipeline", format, scale); rc != DOA_OK) return rc;
    h->format = format; h->scale = scale;
    return DOA_OK;
}

int doa_root_pipeline_set_spatial_smoothing(doa_root_pipeline_t *h, int subarray_size, int forward_backward)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_set_spatial_smoothing: bad arguments"); return DOA_ERR_INVALID_ARG; }
    const int S = subarray_size, fb = S ? forward_backward : 0;
    if (S != 0 && (S < 2 || S > h->N || h->M >= S || (fb != 0 && fb != 1))) {
        doa::set_error("root_pipeline_set_spatial_smoothing: need subarray_size 0 (off) or 2 <= subarray_size <= inputs with "
                       "num_targets < subarray_size, forward_backward 0 or 1 (got %d, %d; inputs=%d num_targets=%d)", S,
                       forward_backward, h->N, h->M);
        return DOA_ERR_INVALID_ARG;
    }
    if (S == h->S && fb == h->fb) return DOA_OK;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    // work_dev / work_dev_auto and the host entry (whose chunks lie at their item offsets) share this one; the lanes of
    // work_dev_batches have their own (kSmooth)
    if (S)
        if (int rc = h->d_smooth.reserve((size_t)h->max_batch * S * S * sizeof(float2)); rc != DOA_OK) return rc;
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
    const int elements = evd_elements(h);
    void *cov = d_cov_out ? d_cov_out : h->d_cov.p;
    int rc = doa::launch_autocorrelate(h->N, h->K, h->ovl, h->avg, n, d_input_items, cov, st, h->has_gain ? h->d_gain.p : nullptr,
                                       h->d_work[0].p, h->format, h->scale);
    if (rc == DOA_OK && h->S) {
        rc = doa::launch_spatial_smooth(h->N, h->S, h->fb, n, cov, h->d_smooth.p, st);
        cov = h->d_smooth.p;
    }
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
    const int N = h->N, M = h->M;
    for (int k = 0; k < N; k++)
        if (!input_items[k]) { doa::set_error("root_pipeline_work: input_items[%d] is NULL", k); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    if (const int src = doa::ensure_stream_pair(h->hst); src != DOA_OK) return src;
    const size_t nonoverlap = (size_t)(h->K - h->ovl);
    const size_t n_all = (size_t)noutput_items;
    const size_t sb = doa::sample_bytes(h->format);     // bytes per input sample: 8 (fc32) or 4 (sc16)
    // result block on the device: [angles | status] per call, sections 256-byte aligned
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t ang_b = n_all * M * sizeof(float), st_b = n_all * sizeof(int);
    // Scheduler-sized calls: one page-locked staging buffer, one copy each way (as music_pipeline; pipeline.hip has the
    // measurements)
    {
        static const size_t kSmallCallBytes = [] { const char *e = getenv("DOA_PIPE_SMALL_CALL_KB"); return (size_t)(e ? atoi(e) : 2048) << 10; }();
        const size_t span = (n_all - 1) * nonoverlap + h->K;
        const size_t span_al = (span + 1) & ~(size_t)1;       // streams two samples apart: pair-load aligned
        const size_t in_bytes = span_al * N * sb;
        const size_t cov_b = cov_out ? n_all * N * N * sizeof(float2) : 0;
        const size_t off_st = up(ang_b), off_cov = off_st + up(st_b);
        const size_t out_bytes = off_cov + cov_b;
        if (in_bytes <= kSmallCallBytes && out_bytes <= kSmallCallBytes) {
            int rc = h->h_stage.reserve(in_bytes > out_bytes ? in_bytes : out_bytes);
            if (rc == DOA_OK) rc = h->d_in[0].reserve(in_bytes);
            if (rc == DOA_OK) rc = h->d_res.reserve(out_bytes);
            if (rc != DOA_OK) return rc;
            hipStream_t st = h->hst[0];
            char *hs = h->h_stage.as<char>();
            const void *d_ptrs[DOA_MAX_ANT_ELE];
            for (int k = 0; k < N; k++) {
                memcpy(hs + (size_t)k * span_al * sb, input_items[k], span * sb);
                d_ptrs[k] = h->d_in[0].as<char>() + (size_t)k * span_al * sb;
            }
            // from the upload on, every exit synchronises the stream first (a copy still reading the staging buffer would
            // race the next call's memcpy into it)
            auto staged = [&]() -> int {
                DOA_HIP_TRY(hipMemcpyAsync(h->d_in[0].p, hs, in_bytes, hipMemcpyHostToDevice, st));
                char *dr = h->d_res.as<char>();
                if (h->fail_chunk == 0) { doa::set_error("root_pipeline_work: injected failure"); return DOA_ERR_HIP; }
                RootWs ws{h->d_coef.p, dr + off_st, h->d_work[0].p, h->d_smooth.p, h->d_rec.p};
                const int rr = run_chain(h, noutput_items, d_ptrs, cov_out ? (void *)(dr + off_cov) : h->d_cov.p, dr, ws, st);
                if (rr < 0) return rr;
                DOA_HIP_TRY(hipMemcpyAsync(hs, dr, out_bytes, hipMemcpyDeviceToHost, st));
                return DOA_OK;
            };
            rc = staged();
            h->fail_chunk = -1; h->lanes.fail_batch = -1;
            const hipError_t se = hipStreamSynchronize(st);
            if (rc < 0) return rc;
            if (se != hipSuccess) { doa::set_error("root_pipeline_work: %s", hipGetErrorString(se)); return DOA_ERR_HIP; }
            memcpy(angles_out, hs, ang_b);
            if (cov_out) memcpy(cov_out, hs + off_cov, cov_b);
            if (const int bad = first_flagged(reinterpret_cast<const int *>(hs + off_st), noutput_items); bad >= 0)
                return numeric_error(h, bad, reinterpret_cast<const int *>(hs + off_st)[bad]);
            return noutput_items;
        }
    }
    // chunks of ~32 MiB of new samples alternating over two streams (as music_pipeline)
    size_t chunk = ((size_t)32 << 20) / (nonoverlap * N * sb);
    chunk = chunk < 1 ? 1 : (chunk > n_all ? n_all : chunk);
    const size_t span_max = (chunk - 1) * nonoverlap + h->K;
    const size_t stride = doa::stream_stride_bytes(span_max * sb);
    int rc = h->d_res.reserve(up(ang_b) + st_b);
    if (rc == DOA_OK) rc = h->h_status.reserve(st_b);
    for (auto &b : h->d_in)
        if (rc == DOA_OK) rc = b.reserve(stride * N);
    if (const size_t ws = doa::autocorrelate_workspace_bytes(N, h->K, h->ovl, (int)chunk); ws && rc == DOA_OK)
        rc = h->d_work[1].reserve(ws);
    if (rc != DOA_OK) return rc;
    float *d_ang = h->d_res.as<float>();
    int *d_st = reinterpret_cast<int *>(h->d_res.as<char>() + up(ang_b));
    int lane = 0, chunk_index = 0;
    auto enqueue_chunk = [&](size_t s0, size_t n, hipStream_t st) -> int {
        const size_t span = (n - 1) * nonoverlap + h->K;
        const void *d_ptrs[DOA_MAX_ANT_ELE];
        for (int k = 0; k < N; k++) {
            char *dst = h->d_in[lane].as<char>() + k * stride;
            const char *src = static_cast<const char *>(input_items[k]) + s0 * nonoverlap * sb;
            DOA_HIP_TRY(hipMemcpyAsync(dst, src, span * sb, hipMemcpyHostToDevice, st));
            d_ptrs[k] = dst;
        }
        if (h->fail_chunk == chunk_index) { doa::set_error("root_pipeline_work: injected failure in chunk %d", chunk_index); return DOA_ERR_HIP; }
        float2 *cov = h->d_cov.as<float2>() + s0 * N * N;
        // (the two copy/compute lanes write disjoint item ranges of the handle's records and smoothed items)
        RootWs ws{static_cast<char *>(h->d_coef.p) + coef_bytes(h, s0), d_st + s0, h->d_work[lane].p,
                  h->S ? (void *)(h->d_smooth.as<float2>() + s0 * h->S * h->S) : nullptr,
                  esprit_mode(h) ? (void *)(h->d_rec.as<char>() + rec_bytes(h, s0)) : nullptr};
        const int rr = run_chain(h, (int)n, d_ptrs, cov, d_ang + s0 * M, ws, st);
        if (rr < 0) return rr;
        if (cov_out)
            DOA_HIP_TRY(hipMemcpyAsync(static_cast<float2 *>(cov_out) + s0 * N * N, cov, n * N * N * sizeof(float2),
                                       hipMemcpyDeviceToHost, st));
        DOA_HIP_TRY(hipMemcpyAsync(static_cast<float *>(angles_out) + s0 * M, d_ang + s0 * M, n * M * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
        DOA_HIP_TRY(hipMemcpyAsync(h->h_status.as<int>() + s0, d_st + s0, n * sizeof(int), hipMemcpyDeviceToHost, st));
        return DOA_OK;
    };
    for (size_t s0 = 0; s0 < n_all; s0 += chunk, lane ^= 1, chunk_index++) {
        const size_t n = (n_all - s0 < chunk) ? n_all - s0 : chunk;
        rc = enqueue_chunk(s0, n, h->hst[lane]);
        if (rc < 0) break;
    }
    h->fail_chunk = -1; h->lanes.fail_batch = -1;
    // the loop's exit -- normal or not -- synchronises BOTH lanes: caller-owned host buffers must be quiet when this returns
    for (auto st : h->hst) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess && rc >= 0) { doa::set_error("root_pipeline_work: %s", hipGetErrorString(e)); rc = DOA_ERR_HIP; }
    }
    if (rc < 0) return rc;
    if (const int bad = first_flagged(h->h_status.as<int>(), noutput_items); bad >= 0) return numeric_error(h, bad, h->h_status.as<int>()[bad]);
    return noutput_items;
}

int doa_root_pipeline_inject_failure(doa_root_pipeline_t *h, int chunk_index)
{
    doa::clear_error();
    if (!h || chunk_index < -1) { doa::set_error("root_pipeline_inject_failure: bad arguments"); return DOA_ERR_INVALID_ARG; }
    h->fail_chunk = chunk_index;
    h->lanes.fail_batch = chunk_index;
    return DOA_OK;
}

int doa_root_pipeline_lanes_idle(doa_root_pipeline_t *h)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_lanes_idle: bad arguments"); return DOA_ERR_INVALID_ARG; }
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    for (auto st : h->hst)
        if (st && hipStreamQuery(st) != hipSuccess) return 0;
    return h->lanes.idle() ? 1 : 0;
}

int doa_root_pipeline_set_internal_precision(doa_root_pipeline_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("root_pipeline_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
