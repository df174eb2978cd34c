// pipeline_front.hip — the bodies of pipeline_front.hpp that are not small: create / destroy, the front's setters, the C
// entries the two handles share whole, and the transport of the host-buffer `work` entries of the fused handles.  Host-only.
#include "pipeline_front.hpp"

#include <cstdlib>
#include <cstring>

namespace doa {

bool PipeFront::check_create(const char *who, int inputs, int snapshot_size, int overlap_size)
{
    if (inputs > 0 && inputs <= DOA_MAX_ANT_ELE && snapshot_size > 0 && overlap_size >= 0 && overlap_size < snapshot_size) return true;
    set_error("%s: bad autocorrelate parameters (inputs=%d snapshot=%d overlap=%d)", who, inputs, snapshot_size, overlap_size);
    return false;
}

int PipeFront::open(int dev, int inputs, int snapshot_size, int overlap_size, int avg_method, int max_batch_)
{
    N = inputs; K = snapshot_size; ovl = overlap_size; avg = avg_method;
    max_batch = max_batch_; device = dev;
    bits = internal_precision_bits();
    self.own_stream = false;
    return DOA_OK;
}

int PipeFront::reserve_front(PipeLane &ln, int cov_batches, int S_)
{
    int rc = ln.buf[kCov].reserve((size_t)cov_batches * max_batch * N * N * sizeof(float2));
    if (const size_t ws = cov_workspace_bytes(N, K, ovl, max_batch); ws && rc == DOA_OK) rc = ln.buf[kWork].reserve(ws);
    if (rc == DOA_OK && S_) rc = ln.buf[kSmooth].reserve((size_t)max_batch * S_ * S_ * sizeof(float2));
    return rc;
}

void PipeFront::destroy(PipeFront *h)
{
    if (!h) return;
    for (auto st : h->hst)
        if (st) (void)hipStreamDestroy(st);
    h->lanes.release();
    delete h;
}

int PipeFront::fuse_antenna_correction(const float *gains_re_im)
{
    if (!gains_re_im) { has_gain = false; return DOA_OK; }
    float2 w[DOA_MAX_ANT_ELE * DOA_MAX_ANT_ELE];
    for (int b = 0; b < N; b++)
        for (int a = 0; a < N; a++) {
            const float ar = gains_re_im[2 * a], ai = gains_re_im[2 * a + 1], br = gains_re_im[2 * b], bi = gains_re_im[2 * b + 1];
            w[a + b * N] = make_float2(ar * br + ai * bi, ai * br - ar * bi);   // g_a conj(g_b)
        }
    if (int brc = bind_device(device); brc != DOA_OK) return brc;
    int rc = d_gain.reserve(sizeof(float2) * N * N);
    if (rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_gain.p, w, sizeof(float2) * N * N, hipMemcpyHostToDevice));
    has_gain = true;
    return DOA_OK;
}

int PipeFront::smoothing_args(const char *who, int M, int S_, int forward_backward) const
{
    if (S_ == 0 || (S_ >= 2 && S_ <= N && M < S_ && (forward_backward == 0 || forward_backward == 1))) return DOA_OK;
    set_error("%s: need subarray_size 0 (off) or 2 <= subarray_size <= inputs with "
              "num_targets < subarray_size, forward_backward 0 or 1 (got %d, %d; inputs=%d num_targets=%d)", who, S_,
              forward_backward, N, M);
    return DOA_ERR_INVALID_ARG;
}

int PipeFront::smoothing_reserve(int S_, int fb_)
{
    if (S_ == S && fb_ == fb) return 0;
    if (int brc = bind_device(device); brc != DOA_OK) return brc;
    return 1;
}

int PipeFront::inject_failure(int chunk_index)
{
    fail_chunk = chunk_index;           // whichever entry is called next consumes it: the host entry (chunk index) ...
    lanes.fail_batch = chunk_index;     // ... or the batches entry (batch index); both clear both
    return DOA_OK;
}

int PipeFront::lanes_idle()
{
    if (int brc = bind_device(device); brc != DOA_OK) return brc;
    for (auto st : hst)
        if (st && hipStreamQuery(st) != hipSuccess) return 0;
    return lanes.idle() ? 1 : 0;
}

int PipeFront::entry_fuse_antenna_correction(PipeFront *h, const float *gains_re_im)
{
    clear_error();
    if (!h) return DOA_ERR_INVALID_ARG;
    return h->fuse_antenna_correction(gains_re_im);
}

// clears the error; a refused call: false, with "<pre>_<entry>: bad arguments" set
static bool entry_args(bool ok, const char *pre, const char *entry)
{
    clear_error();
    if (!ok) set_error("%s_%s: bad arguments", pre, entry);
    return ok;
}

int PipeFront::entry_set_input_format(PipeFront *h, const char *pre, int format, float scale)
{
    if (!entry_args(h, pre, "set_input_format")) return DOA_ERR_INVALID_ARG;
    return h->set_input_format(pre, format, scale);
}

int PipeFront::entry_set_lanes(PipeFront *h, const char *pre, int n_lanes)
{
    clear_error();
    if (h && h->lanes.set_count(n_lanes) == DOA_OK) return DOA_OK;
    set_error("%s_set_lanes: need 1 <= n_lanes <= %d", pre, PipeLanes::kMaxLanes);
    return DOA_ERR_INVALID_ARG;
}

int PipeFront::entry_set_lane_streams(PipeFront *h, const char *pre, int n_lanes, void *const *hip_streams)
{
    clear_error();
    if (!h || n_lanes < 1 || n_lanes > PipeLanes::kMaxLanes || !hip_streams) {
        set_error("%s_set_lane_streams: need 1 <= n_lanes <= %d and the streams", pre, PipeLanes::kMaxLanes);
        return DOA_ERR_INVALID_ARG;
    }
    if (int brc = bind_device(h->device); brc != DOA_OK) return brc;
    return h->lanes.adopt(n_lanes, hip_streams);
}

int PipeFront::entry_synchronize(PipeFront *h, const char *pre)
{
    if (!entry_args(h, pre, "synchronize")) return DOA_ERR_INVALID_ARG;
    if (int brc = bind_device(h->device); brc != DOA_OK) return brc;
    return h->lanes.synchronize();
}

int PipeFront::entry_inject_failure(PipeFront *h, const char *pre, int chunk_index)
{
    if (!entry_args(h && chunk_index >= -1, pre, "inject_failure")) return DOA_ERR_INVALID_ARG;
    return h->inject_failure(chunk_index);
}

int PipeFront::entry_lanes_idle(PipeFront *h, const char *pre)
{
    if (!entry_args(h, pre, "lanes_idle")) return DOA_ERR_INVALID_ARG;
    return h->lanes_idle();
}

int PipeFront::host_open(const char *who, const void *const *input_items)
{
    for (int k = 0; k < N; k++)
        if (!input_items[k]) { set_error("%s: input_items[%d] is NULL", who, k); return DOA_ERR_INVALID_ARG; }
    if (int brc = bind_device(device); brc != DOA_OK) return brc;
    return ensure_stream_pair(hst);
}

int PipeFront::host_run(const char *who, int n_items, const void *const *input_items, const HostSection *sec, int n_sec,
                        const HostChain &chain)
{
    constexpr int kMaxSections = 4;
    if (n_sec > kMaxSections) { set_error("%s: more than %d output sections", who, kMaxSections); return DOA_ERR_INVALID_ARG; }
    const int fail_at = fail_chunk;
    fail_chunk = -1; lanes.fail_batch = -1;             // one-shot: armed for THIS call only, wherever it ends
    const size_t n_all = (size_t)n_items;
    const size_t nonoverlap = (size_t)(K - ovl);
    const size_t sb = fmt.sample_bytes();            // bytes per input sample: 8 (fc32) or 4 (sc16)
    // The result block of the staged path holds the present sections in the order given, each on a 256-byte boundary (the
    // scan kernels' 16-byte stores need aligned spectrum rows); the chunked path keeps the sections without a device area of
    // their own in d_res, laid out the same way for max_batch items.
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t bytes[kMaxSections], off[kMaxSections], res_off[kMaxSections];
    size_t out_bytes = 0, res_bytes = 0;
    for (int i = 0; i < n_sec; i++) {
        bytes[i] = sec[i].host ? n_all * sec[i].item_bytes : 0;
        off[i] = i ? off[i - 1] + up(bytes[i - 1]) : 0;
        out_bytes = off[i] + bytes[i];
        res_off[i] = res_bytes;
        if (!sec[i].area) res_bytes += up((size_t)max_batch * sec[i].item_bytes);
    }
    void *d_sec[kMaxSections];
    // Scheduler-sized calls (a GNU Radio work() hands over a few to a few hundred items): the fixed costs are what
    // counts -- N pageable host-to-device copies, up to four copies back and two stream synchronisations.  Below
    // kSmallCallBytes of input the window of every stream is packed into ONE page-locked staging buffer (the same
    // bytes the driver's pageable path would stage, minus its per-copy set-up), crosses PCIe as ONE transfer, and the
    // results (with the optional covariances / spectra) come back as ONE transfer through the same buffer.  Measured on the
    // music handle: 8 items 105 -> 53 us per call, 64 items 151 -> 116 us; from 8 MiB up the host-side packing costs more
    // than it saves.
    {
        static const size_t kSmallCallBytes = [] { const char *e = getenv("DOA_PIPE_SMALL_CALL_KB"); return (size_t)(e ? atoi(e) : 2048) << 10; }();
        const size_t span = (n_all - 1) * nonoverlap + K;
        const size_t span_al = (span + 1) & ~(size_t)1;       // streams two samples apart: pair-load aligned
        const size_t in_bytes = span_al * N * sb;
        // (the gate looks at BOTH directions: a short-snapshot, long-spectrum call returns n * P * 4 bytes, and staging
        // hundreds of MiB of spectra through the page-locked buffer -- plus a host memcpy each -- is what the chunked
        // path below exists to avoid)
        if (in_bytes <= kSmallCallBytes && out_bytes <= kSmallCallBytes) {
            int rc = h_stage.reserve(in_bytes > out_bytes ? in_bytes : out_bytes);
            if (rc == DOA_OK) rc = d_in[0].reserve(in_bytes);
            if (rc == DOA_OK) rc = d_res.reserve(out_bytes > res_bytes ? out_bytes : res_bytes);
            if (rc != DOA_OK) return rc;
            hipStream_t st = hst[0];
            char *hs = h_stage.as<char>();
            const void *d_ptrs[DOA_MAX_ANT_ELE];
            for (int k = 0; k < N; k++) {
                memcpy(hs + (size_t)k * span_al * sb, input_items[k], span * sb);
                d_ptrs[k] = d_in[0].as<char>() + (size_t)k * span_al * sb;
            }
            // From the upload on, every exit synchronises the stream first: a copy still reading the staging buffer
            // would race the next call's memcpy into it.
            auto staged = [&]() -> int {
                DOA_HIP_TRY(hipMemcpyAsync(d_in[0].p, hs, in_bytes, hipMemcpyHostToDevice, st));
                if (fail_at == 0) { set_error("%s: injected failure", who); return DOA_ERR_HIP; }
                char *dr = d_res.as<char>();
                for (int i = 0; i < n_sec; i++) d_sec[i] = sec[i].host ? dr + off[i] : nullptr;
                const int rr = chain(n_items, d_ptrs, 0, d_sec, st, 0);
                if (rr < 0) return rr;
                // (the staging buffer is free again: the upload was enqueued before the kernels on the same stream, and
                // the download below is ordered behind them)
                DOA_HIP_TRY(hipMemcpyAsync(hs, dr, out_bytes, hipMemcpyDeviceToHost, st));
                return DOA_OK;
            };
            rc = staged();
            const hipError_t se = hipStreamSynchronize(st);
            if (rc < 0) return rc;
            if (se != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(se)); return DOA_ERR_HIP; }
            for (int i = 0; i < n_sec; i++)
                if (sec[i].host) memcpy(sec[i].host, hs + off[i], bytes[i]);
            return n_items;
        }
    }
    // Chunks of ~32 MiB of new samples alternate over two streams: while one chunk's results travel back
    // the next chunk's samples travel in (PCIe is full duplex; the kernels themselves are ~1 % of a
    // chunk's transfer time).  The overlap needs page-locked caller buffers; pageable ones still work.
    size_t chunk = ((size_t)32 << 20) / (nonoverlap * N * sb);
    chunk = chunk < 1 ? 1 : (chunk > n_all ? n_all : chunk);
    const size_t span_max = (chunk - 1) * nonoverlap + K;
    // distance between the device copies of the streams: 16-B aligned and staggered against the 8 KiB aliasing period
    const size_t stride = stream_stride_bytes(span_max * sb);
    int rc = d_res.reserve(res_bytes);
    for (auto &b : d_in)
        if (rc == DOA_OK) rc = b.reserve(stride * N);
    if (const size_t ws = cov_workspace_bytes(N, K, ovl, (int)chunk); ws && rc == DOA_OK)
        rc = d_work1.reserve(ws);                      // lane 0 uses the workspace create() sized for max_batch
    if (rc != DOA_OK) return rc;
    int lane = 0, chunk_index = 0;
    // One chunk: uploads, kernels, downloads, all on its lane's stream.  A failure anywhere in it ends the loop, and the
    // loop's exit -- normal or not -- synchronises BOTH lanes: the other lane may still be copying to or from caller-owned
    // host buffers, which must be quiet before this call returns.
    auto enqueue_chunk = [&](size_t s0, size_t n, hipStream_t st) -> int {
        const size_t span = (n - 1) * nonoverlap + K;
        const void *d_ptrs[DOA_MAX_ANT_ELE];
        for (int k = 0; k < N; k++) {
            char *dst = d_in[lane].as<char>() + k * stride;
            const char *src = static_cast<const char *>(input_items[k]) + s0 * nonoverlap * sb;
            DOA_HIP_TRY(hipMemcpyAsync(dst, src, span * sb, hipMemcpyHostToDevice, st));
            d_ptrs[k] = dst;
        }
        if (fail_at == chunk_index) { set_error("%s: injected failure in chunk %d", who, chunk_index); return DOA_ERR_HIP; }
        for (int i = 0; i < n_sec; i++) {
            char *base = sec[i].area ? static_cast<char *>(sec[i].area) : d_res.as<char>() + res_off[i];
            d_sec[i] = sec[i].host ? base + s0 * sec[i].item_bytes : nullptr;
        }
        const int rr = chain((int)n, d_ptrs, s0, d_sec, st, lane);
        if (rr < 0) return rr;
        // one download per present section: the ones with an area of their own (the large ones) first, then those in d_res
        for (int own = 1; own >= 0; own--)
            for (int i = 0; i < n_sec; i++)
                if (sec[i].host && (sec[i].area != nullptr) == (own == 1))
                    DOA_HIP_TRY(hipMemcpyAsync(static_cast<char *>(sec[i].host) + s0 * sec[i].item_bytes, d_sec[i],
                                               n * sec[i].item_bytes, hipMemcpyDeviceToHost, st));
        return DOA_OK;
    };
    for (size_t s0 = 0; s0 < n_all; s0 += chunk, lane ^= 1, chunk_index++) {
        const size_t n = (n_all - s0 < chunk) ? n_all - s0 : chunk;
        rc = enqueue_chunk(s0, n, hst[lane]);
        if (rc < 0) break;
    }
    for (auto st : hst) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess && rc >= 0) { set_error("%s: %s", who, hipGetErrorString(e)); rc = DOA_ERR_HIP; }
    }
    return rc < 0 ? rc : n_items;
}

}  // namespace doa

// the plan of a work_dev_batches call on flat arrays, for the CPU tests: no handle, no device
extern "C" int doa_hip_batch_plan_debug(int n_batches, const void *const *outputs, const unsigned char *flags, const int *caps,
                                        int n_lanes, int rotation_in, int *group_out, int *lane_out, int *sync_first_out,
                                        int *rotation_out)
{
    doa::clear_error();
    bool ok = n_batches >= 0 && outputs && flags && caps && group_out && lane_out && sync_first_out && rotation_out &&
              n_lanes >= 1 && n_lanes <= doa::PipeLanes::kMaxLanes && rotation_in >= 0 && rotation_in < n_lanes;
    for (int b = 0; ok && b < n_batches; b++) ok = flags[b] < 8 && caps[b] >= 1;
    if (!ok) {
        doa::set_error("hip_batch_plan_debug: bad arguments (every array, 1 <= n_lanes <= %d, 0 <= rotation_in < n_lanes, flags < 8, caps >= 1)",
                       doa::PipeLanes::kMaxLanes);
        return DOA_ERR_INVALID_ARG;
    }
    std::vector<doa::PlanGroup> plan;
    *rotation_out = doa::plan_batches(n_batches, n_lanes, rotation_in, [&](int b, doa::PlanGroup &nb, const void *(&out)[4]) {
        for (int k = 0; k < 4; k++) out[k] = outputs[4 * b + k];
        nb.lean = flags[b] & 1; nb.store = flags[b] & 2; nb.vec2 = flags[b] & 4;
        nb.cap = caps[b];
    }, plan);
    for (size_t g = 0; g < plan.size(); g++)
        for (int b = plan[g].b0; b < plan[g].b0 + plan[g].nb; b++) {
            group_out[b] = (int)g; lane_out[b] = plan[g].lane; sync_first_out[b] = plan[g].sync_first;
        }
    return (int)plan.size();
}
