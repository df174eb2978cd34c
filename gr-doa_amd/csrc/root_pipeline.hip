// root_pipeline.hip — autocorrelate -> rootMUSIC_linear_array on device-resident streams: the Root-MUSIC branch of the hot
// path as ONE handle, the chain apps/run_RootMUSIC_lin_array_simulation.grc wires (autocorrelate(N, K, ovl, avg) ->
// rootMUSIC_linear_array(d, M, N); reference work being chained: lib/autocorrelate_impl.cc:83-118 ->
// lib/rootMUSIC_linear_array_impl.cc:90-152).  Three launches per batch -- K1 covariance, K2+K3 EVD / projector / diagonal
// sums (double records), K6 roots + selection -- with the same entry points, lanes, detached form and error contract as
// music_pipeline (pipeline.hip, pipeline_lanes.hpp).  Until round 4 this branch had to be driven as two block handles and
// two calls per batch, which left it host-bound above ~20 us per 4096-snapshot step.
#include "gridfree_chain.hpp"
#include "pipeline_front.hpp"

// the front (K1, smoothing, the host entry's transport, the lanes) is doa::PipeFront's; these are the estimator stage's
struct doa_root_pipeline : doa::PipeFront {
    int M = 0;
    float norm_spacing = 0.f;
    int estimator = DOA_GRIDFREE_ROOT_MUSIC;    // doa_root_pipeline_set_estimator
    doa::PinnedBuf h_status;        // host-pointer entry point: the items' status words, scanned after the call's copies
    // a lane's slots after the front's: coefficient records, status words nobody asked for, ESPRIT mode's signal-subspace
    // records between the eigen launch and esprit_kernel
    enum { kCoef = kFrontBufs, kStatus, kRec };
    // what the chain runs: the estimator on the elements the eigen stage sees
    doa::GridfreeDesc desc() const { return {estimator, elements(), M, norm_spacing, bits}; }
};

namespace {
struct RootWs {
    void *cov;        // covariance items, for a chain whose caller does not ask for them
    void *work;       // K1's piece sums (overlapping windows), or NULL
    void *smooth;     // spatial smoothing on: S * S gr_complex per item (else unused)
    doa::GridfreeRecords rec;   // the lane's records; status: one int per item, for a chain whose caller brings no buffer
};
// a lane's record slots, per item: an estimator's records at 64 bits
// (sized for the full array: a later set_spatial_smoothing only makes the records smaller)
doa::GridfreePlan slot_plan(const doa_root_pipeline *h, int estimator) { return doa::gridfree_plan(estimator, h->N, 64, false); }
bool esprit_mode(const doa_root_pipeline *h) { return h->estimator == DOA_GRIDFREE_ESPRIT; }
// The workspace `ln` (the handle's own, or a lane of work_dev_batches) as a chain sees it, from item `item_off` on (the host
// entry's two copy/compute lanes write disjoint item ranges)
RootWs view(doa_root_pipeline *h, doa::PipeLane &ln, size_t item_off)
{
    using H = doa_root_pipeline;
    const doa::GridfreePlan root = slot_plan(h, DOA_GRIDFREE_ROOT_MUSIC), esprit = slot_plan(h, DOA_GRIDFREE_ESPRIT);
    return {ln.at(H::kCov, item_off, (size_t)h->N * h->N * sizeof(float2)), ln.buf[H::kWork].p,
            ln.at(H::kSmooth, item_off, (size_t)h->S * h->S * sizeof(float2)),
            {ln.at(H::kCoef, item_off, root.coef), ln.at(H::kRec, item_off, esprit.rec), ln.at(H::kStatus, item_off, root.status)}};
}
// Sizes `ln` for one batch with smoothing S and estimator `estimator` (a setter passes what it is about to commit);
// need_cov / need_status: some batch brings no covariance / status buffer of its own.  The coefficient slot is kept in
// either mode, so that a return to Root-MUSIC reserves nothing.
int reserve(doa_root_pipeline *h, doa::PipeLane &ln, bool need_cov, bool need_status, int S, int estimator)
{
    using H = doa_root_pipeline;
    const size_t items = (size_t)h->max_batch;
    const doa::GridfreePlan root = slot_plan(h, DOA_GRIDFREE_ROOT_MUSIC);
    int rc = h->reserve_front(ln, need_cov ? 1 : 0, S);
    if (rc == DOA_OK) rc = ln.buf[H::kCoef].reserve(items * root.coef);
    if (rc == DOA_OK && need_status) rc = ln.buf[H::kStatus].reserve(items * root.status);
    if (rc == DOA_OK && estimator == DOA_GRIDFREE_ESPRIT) rc = ln.buf[H::kRec].reserve(items * slot_plan(h, estimator).rec);
    return rc;
}
int esprit_precision(const char *who, const doa_root_pipeline *h)
{
    return esprit_mode(h) ? doa::need_bits64(who, h->bits, "ESPRIT") : DOA_OK;
}

// K1 -> smoothing -> eigen launch -> solver for n items on `st`; counts: work_dev_auto's estimate, or NULL; status: the
// caller's words, or NULL for the lane's
int run_chain(doa_root_pipeline *h, int n, const void *const *d_in, void *cov, void *angles, const doa::EvdCounts *counts,
              void *status, const RootWs &ws, hipStream_t st)
{
    int rc = h->run_k1(n, d_in, cov, ws.work, st);
    if (rc == DOA_OK) rc = h->run_smoothing(n, cov, ws.smooth, st);
    if (rc == DOA_OK) rc = doa::gridfree_run(h->desc(), n, cov, counts, ws.rec, angles, status, st);
    return rc == DOA_OK ? n : rc;
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
        return reserve(&h, h.self, true, true, h.S, h.estimator);
    });
}

void doa_root_pipeline_destroy(doa_root_pipeline_t *h) { doa::PipeFront::destroy(h); }

int doa_root_pipeline_fuse_antenna_correction(doa_root_pipeline_t *h, const float *gains_re_im)
{
    return doa::PipeFront::entry_fuse_antenna_correction(h, gains_re_im);
}

int doa_root_pipeline_set_input_format(doa_root_pipeline_t *h, int format, float scale)
{
    return doa::PipeFront::entry_set_input_format(h, "root_pipeline", format, scale);
}

int doa_root_pipeline_set_spatial_smoothing(doa_root_pipeline_t *h, int subarray_size, int forward_backward)
{
    doa::clear_error();
    if (!h) { doa::set_error("root_pipeline_set_spatial_smoothing: bad arguments"); return DOA_ERR_INVALID_ARG; }
    const int S = subarray_size, fb = S ? forward_backward : 0;
    if (int rc = h->smoothing_args("root_pipeline_set_spatial_smoothing", h->M, S, forward_backward); rc != DOA_OK) return rc;
    if (int rc = h->smoothing_reserve(S, fb); rc <= 0) return rc;
    if (int rc = reserve(h, h->self, true, true, S, h->estimator); rc != DOA_OK) return rc;
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
        if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
        if (int rc = reserve(h, h->self, true, true, h->S, estimator); rc != DOA_OK) return rc;
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
    const RootWs ws = view(h, h->self, 0);
    return run_chain(h, noutput_items, d_input_items, d_cov_out ? d_cov_out : ws.cov, d_angles_out, nullptr, d_status_out, ws,
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
    if (h->bits != 64) {                        // (need_bits64's rule, in this entry's own words: "need", not "needs")
        doa::set_error("root_pipeline_work_dev_auto: per-item counts need internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    if (h->K < 2) {
        doa::set_error("root_pipeline_work_dev_auto: the criterion needs snapshot_size >= 2 (handle has %d)", h->K);
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const RootWs ws = view(h, h->self, 0);
    const doa::EvdCounts cnt = doa::evd_counts_estimate((int *)d_count_out, (float *)d_eig_out, h->K, method, h->M);
    return run_chain(h, noutput_items, d_input_items, d_cov_out ? d_cov_out : ws.cov, d_angles_out, &cnt, d_status_out, ws,
                     static_cast<hipStream_t>(hip_stream));
}

int doa_root_pipeline_set_lanes(doa_root_pipeline_t *h, int n_lanes)
{
    return doa::PipeFront::entry_set_lanes(h, "root_pipeline", n_lanes);
}

int doa_root_pipeline_set_lane_streams(doa_root_pipeline_t *h, int n_lanes, void *const *hip_streams)
{
    return doa::PipeFront::entry_set_lane_streams(h, "root_pipeline", n_lanes, hip_streams);
}

int doa_root_pipeline_synchronize(doa_root_pipeline_t *h)
{
    return doa::PipeFront::entry_synchronize(h, "root_pipeline");
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
    // the plan (batch_plan.hpp): no groups here, and a batch that writes what an earlier one wrote follows it on its lane
    auto traits = [&](int b, doa::PlanGroup &, const void *(&out)[4]) {
        out[0] = d_cov_out ? d_cov_out[b] : nullptr; out[1] = d_angles_out[b]; out[2] = d_status_out ? d_status_out[b] : nullptr;
    };
    const bool need_cov = doa::PipeLanes::lacks(d_cov_out, n_batches), need_status = doa::PipeLanes::lacks(d_status_out, n_batches);
    auto prepare = [&](doa::PipeLane &ln) { return reserve(h, ln, need_cov, need_status, h->S, h->estimator); };
    auto launch = [&](const doa::PlanGroup &g, doa::PipeLane &ln) -> int {
        const int b = g.b0;                                          // (groups of one)
        const RootWs ws = view(h, ln, 0);
        return run_chain(h, noutput_items, d_input_items + (size_t)b * N, (d_cov_out && d_cov_out[b]) ? d_cov_out[b] : ws.cov,
                         d_angles_out[b], nullptr, d_status_out ? d_status_out[b] : nullptr, ws, ln.st);
    };
    const int rc = h->run_planned("root_pipeline_work_dev_batches", n_batches, h->lanes.n_lanes, hip_stream, traits, prepare, launch);
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
    // covariances in the handle's own workspace at their item offsets
    const doa::HostSection sec[3] = {{angles_out, h->M * sizeof(float), nullptr}, {h->h_status.p, sizeof(int), nullptr},
                                     {cov_out, N * N * sizeof(float2), h->self.buf[doa_root_pipeline::kCov].p}};
    const int rc = h->host_run(who, noutput_items, input_items, sec, 3,
                               [h](int n, const void *const *d_in, size_t item_off, void *const *d_sec, hipStream_t st, int lane) {
        RootWs ws = view(h, h->self, item_off);
        ws.work = h->host_work(lane);
        return run_chain(h, n, d_in, d_sec[2] ? d_sec[2] : ws.cov, d_sec[0], nullptr, d_sec[1], ws, st);
    });
    if (rc < 0) return rc;
    // the other items' outputs are valid
    if (const int bad = doa::gridfree_first_error(h->h_status.as<int>(), noutput_items); bad >= 0) return numeric_error(h, bad, h->h_status.as<int>()[bad]);
    return noutput_items;
}

int doa_root_pipeline_inject_failure(doa_root_pipeline_t *h, int chunk_index)
{
    return doa::PipeFront::entry_inject_failure(h, "root_pipeline", chunk_index);
}

int doa_root_pipeline_lanes_idle(doa_root_pipeline_t *h)
{
    return doa::PipeFront::entry_lanes_idle(h, "root_pipeline");
}

int doa_root_pipeline_set_internal_precision(doa_root_pipeline_t *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("root_pipeline_set_internal_precision: need a handle and bits = 32 or 64"); return DOA_ERR_INVALID_ARG; }
    h->bits = bits;
    return DOA_OK;
}

}  // extern "C"
