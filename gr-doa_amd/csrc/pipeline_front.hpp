// pipeline_front.hpp — what the fused handles (music_pipeline: pipeline.hip; root_pipeline: root_pipeline.hip) have in
// common: the autocorrelate front of every chain (K1 with the fused antenna correction and the fc32 / sc16 input, optional
// spatial smoothing), create and destroy, the front's setters, and the transport of the host-buffer `work` entries.  A
// handle adds its estimator stage: its own members, a callback that queues its chain, and the list of its output sections.
// Host-only; the kernels are launched through kernels.hpp.  INTEGRATION.md ("Adding a block") shows what a handle writes.
#pragma once
#include "block_host.hpp"
#include "kernels.hpp"
#include "pipeline_lanes.hpp"

#include <functional>

namespace doa {

// One output of a host `work` entry, n items of item_bytes each.  host: the caller's buffer (NULL = an absent optional
// port).  area: the device area that holds the section's items at their item offsets on the chunked path (max_batch items;
// NULL = the transport's own result block).
struct HostSection {
    void *host;
    size_t item_bytes;
    void *area;
};
// Queues a handle's chain for n items on `st`: d_in are the device copies of the input streams, item_off the offset of the
// first item within the call (the chunks in flight on the two lanes must not share per-item records), d_sec[i] where
// section i's items go (NULL for an absent one), lane the copy/compute lane (its K1 workspace is host_work(lane)).
// Returns < 0 on failure.
using HostChain = std::function<int(int n, const void *const *d_in, size_t item_off, void *const *d_sec, hipStream_t st, int lane)>;

struct PipeFront {
    int N = 0, K = 0, ovl = 0, avg = 0;
    int max_batch = 0;
    int bits = 64;
    int device = 0;
    DevBuf d_gain;
    bool has_gain = false;
    InputFormat fmt;                // set_input_format
    int S = 0, fb = 0;              // spatial smoothing: subarray size (0 = off), forward-backward
    // The handle's own workspace is a lane without a stream of its own (a call sets self.st to the caller's stream): work_dev,
    // work_dev_auto, the host entry and a solo work_dev_batches call use it, every other work_dev_batches call the lanes below.
    // A lane's slots: the front's three -- covariance items, K1's piece sums (overlapping windows), the smoothed items (S * S
    // per item) between K1 and the eigen stage -- and after them the handle's.
    enum { kCov = 0, kWork, kSmooth, kFrontBufs };
    PipeLane self;
    // host-pointer entry point only: two copy/compute lanes
    hipStream_t hst[2] = {nullptr, nullptr};
    DevBuf d_in[2], d_res;
    DevBuf d_work1;                 // K1's piece sums of the second copy/compute lane (the first: self.buf[kWork])
    PinnedBuf h_stage;              // scheduler-sized calls: one page-locked staging buffer, one copy each way
    int fail_chunk = -1;            // inject_failure, host-pointer entry: one-shot, cleared by every call (tests)
    PipeLanes lanes;                // work_dev_batches: the library's own overlap lanes (pipeline_lanes.hpp)

    virtual ~PipeFront() = default; // (DevBuf / PinnedBuf / table members free themselves)

    // create: the autocorrelate parameters are refused before a device is looked for
    static bool check_create(const char *who, int inputs, int snapshot_size, int overlap_size);
    // create, after the caller's checks: the front's parameters and precision (the handle's init reserves `self`)
    int open(int dev, int inputs, int snapshot_size, int overlap_size, int avg_method, int max_batch_);
    static void destroy(PipeFront *h);

    int fuse_antenna_correction(const float *gains_re_im);
    int set_input_format(const char *who, int format, float scale) { return fmt.set(who, format, scale); }
    // set_spatial_smoothing in two steps, with room for a handle's own refusals between them and its own tables after them.
    // smoothing_args: the range and flag check (M = the handle's source count).  smoothing_reserve: 0 = the handle has
    // (S_, fb_) already, nothing to do; 1 = device bound, the caller reserves `self` for S_, finishes and stores S and fb.
    int smoothing_args(const char *who, int M, int S_, int forward_backward) const;
    int smoothing_reserve(int S_, int fb_);
    // the front's slots of a lane: covariance items for `cov_batches` batches (0: every batch brings its own), K1's piece
    // sums, the smoothed items of subarray size S_ (a handle's reserve function calls this, then sizes its own slots)
    int reserve_front(PipeLane &ln, int cov_batches, int S_);
    void *host_work(int lane) const { return lane ? d_work1.p : self.buf[kWork].p; }
    // work_dev_batches behind a handle's argument checks: the batches in front of an armed inject_failure are planned over L
    // lanes (traits: batch_plan.hpp) from where the rotation stands, and the plan runs (pipeline_lanes.hpp: run_units)
    template <class Traits, class Prepare, class Launch>
    int run_planned(const char *who, int n_batches, int L, void *hip_stream, Traits traits, Prepare prepare, Launch launch)
    {
        const int fail_at = lanes.fail_batch < n_batches ? lanes.fail_batch : -1;
        fail_chunk = -1; lanes.fail_batch = -1;             // (the test aid is one-shot for whichever entry comes next)
        std::vector<PlanGroup> plan;
        plan.reserve((size_t)n_batches);
        lanes.next_lane = plan_batches(fail_at >= 0 ? fail_at : n_batches, L, lanes.next_lane % L, traits, plan);
        return lanes.run_units(who, plan, fail_at, hip_stream, self, prepare, launch);
    }
    int inject_failure(int chunk_index);
    int lanes_idle();

    // the array the eigen stage and what follows it see: the subarray of a smoothed handle
    int elements() const { return S ? S : N; }
    // the front of a chain: K1 for n items on `st` into `cov` (`work`: its piece sums, or NULL) ...
    int run_k1(int n, const void *const *d_in_ptrs, void *cov, void *work, hipStream_t st) const
    {
        return launch_autocorrelate(N, K, ovl, avg, n, d_in_ptrs, cov, st, has_gain ? d_gain.p : nullptr, work, fmt.format, fmt.scale);
    }
    // ... and the smoothing launch into `smooth` (none when it is off); `cov` stays the N x N item and is returned as what the
    // eigen stage reads
    int run_smoothing(int n, void *&cov, void *smooth, hipStream_t st) const
    {
        if (!S) return DOA_OK;
        const int rc = launch_spatial_smooth(N, S, fb, n, cov, smooth, st);
        cov = smooth;
        return rc;
    }

    // The host-buffer `work` entry.  host_open: the NULL-stream check, the device, the two streams.  host_run: the samples go
    // up, chain() queues the handle's launches, the sections come down into their host buffers -- staged through h_stage for
    // scheduler-sized calls, in chunks over the two lanes otherwise (pipeline_front.hip).  Returns n, or < 0 with every copy of
    // the call finished.
    int host_open(const char *who, const void *const *input_items);
    int host_run(const char *who, int n, const void *const *input_items, const HostSection *sec, int n_sec, const HostChain &chain);

    // The C entries the two handles share word for word, whole: h may be NULL, pre is "music_pipeline" / "root_pipeline".
    static int entry_fuse_antenna_correction(PipeFront *h, const float *gains_re_im);
    static int entry_set_input_format(PipeFront *h, const char *pre, int format, float scale);
    static int entry_set_lanes(PipeFront *h, const char *pre, int n_lanes);
    static int entry_set_lane_streams(PipeFront *h, const char *pre, int n_lanes, void *const *hip_streams);
    static int entry_synchronize(PipeFront *h, const char *pre);
    static int entry_inject_failure(PipeFront *h, const char *pre, int chunk_index);
    static int entry_lanes_idle(PipeFront *h, const char *pre);
};

// The tail of a handle's create: device, handle, the front, then init(*h) -> DOA_OK or an error (the handle's tables and records)
template <class H, class Init>
H *create_pipeline(int inputs, int snapshot_size, int overlap_size, int avg_method, int max_batch, Init &&init)
{
    int dev = 0;
    if (ensure_device(&dev) != DOA_OK) return nullptr;
    H *h = new (std::nothrow) H();
    if (!h) { set_error("out of memory"); return nullptr; }
    if (h->open(dev, inputs, snapshot_size, overlap_size, avg_method, max_batch) != DOA_OK || init(*h) != DOA_OK) {
        PipeFront::destroy(h);
        return nullptr;
    }
    return h;
}

}  // namespace doa
