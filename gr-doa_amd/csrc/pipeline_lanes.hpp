// pipeline_lanes.hpp — the overlap lanes shared by the fused pipeline handles (music_pipeline: pipeline.hip; root_pipeline:
// root_pipeline.hip): a HIP stream plus a private set of workspace buffers each, batches of one call spread over them in
// rotation (batch_plan.hpp), one fork and one join per call when the call is attached to a caller stream, none in the detached form.
// The reference has nothing of the kind: GNU Radio runs its blocks on one thread each, which is where its overlap comes from.
#pragma once
#include "batch_plan.hpp"
#include "common.hpp"

#include <string>

namespace doa {

// n_new streams that were seen to run their kernels beside each other and beside the n_have given ones (lane_streams.hip)
int create_lane_streams(const hipStream_t *have, int n_have, hipStream_t *out, int n_new);

// the two copy / compute streams of the host-buffer entries, created on first use: the second is probed against the first
inline int ensure_stream_pair(hipStream_t (&st)[2])
{
    for (int i = 0; i < 2; i++) {
        if (st[i]) continue;
        if (const int rc = create_lane_streams(&st[1 - i], st[1 - i] ? 1 : 0, &st[i], 1); rc != DOA_OK) return rc;
    }
    return DOA_OK;
}

struct PipeLane {
    hipStream_t st = nullptr;
    bool own_stream = true;         // false: adopted from the caller (doa_*_pipeline_set_lane_streams)
    hipEvent_t done = nullptr;
    static constexpr int kBufs = 9;
    DevBuf buf[kBufs];              // what they hold is the owning pipeline's business
    // a slot's items from item `item_off` on (NULL while the slot is empty)
    void *at(int slot, size_t item_off, size_t item_bytes) const { return buf[slot].p ? buf[slot].as<char>() + item_off * item_bytes : nullptr; }
};

struct PipeLanes {
    static constexpr int kMaxLanes = 8;
    PipeLane lanes[kMaxLanes];
    int n_lanes = 4;
    int next_lane = 0;              // lanes keep rotating across calls
    hipEvent_t fork_ev = nullptr;
    int fail_batch = -1;            // test aid (doa_*_pipeline_inject_failure): one-shot, cleared by every call

    void release()
    {
        for (auto &l : lanes) {
            for (auto &b : l.buf) b.release();
            if (l.done) (void)hipEventDestroy(l.done);
            if (l.st && l.own_stream) (void)hipStreamDestroy(l.st);
            l = PipeLane();
        }
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        fork_ev = nullptr;
    }
    int set_count(int n)
    {
        if (n < 1 || n > kMaxLanes) return DOA_ERR_INVALID_ARG;
        n_lanes = n;
        next_lane = 0;
        return DOA_OK;
    }
    int adopt(int n, void *const *hip_streams)
    {
        if (n < 1 || n > kMaxLanes || !hip_streams) return DOA_ERR_INVALID_ARG;
        for (int l = 0; l < n; l++) {
            auto &ln = lanes[l];
            if (ln.st) { (void)hipStreamSynchronize(ln.st); if (ln.own_stream) (void)hipStreamDestroy(ln.st); }
            ln.st = static_cast<hipStream_t>(hip_streams[l]);
            ln.own_stream = false;
        }
        n_lanes = n;
        next_lane = 0;
        return DOA_OK;
    }
    int synchronize()
    {
        for (auto &l : lanes)
            if (l.st) DOA_HIP_TRY(hipStreamSynchronize(l.st));
        return DOA_OK;
    }
    bool idle() const
    {
        for (auto &l : lanes)
            if (l.st && hipStreamQuery(l.st) != hipSuccess) return false;
        return true;
    }

    // does an optional array of n optional pointers leave some batch without a buffer of its own?
    template <class P> static bool lacks(P *const *arr, int n)
    {
        for (int b = 0; arr && b < n; b++)
            if (!arr[b]) return true;
        return !arr;
    }
    // a call with nothing to overlap: its units run on the caller's stream itself
    bool solo(void *hip_stream) const { return n_lanes == 1 && hip_stream != DOA_STREAM_DETACHED; }

    // Group g of the plan (batch_plan.hpp; lanes < n_lanes) runs launch(g, lane) on lane g.lane, the groups of one lane in order,
    // behind a host join of all lanes where g.sync_first asks for it.  `prepare(lane)` sizes a lane's buffers (first use /
    // growth); `launch` returns < 0 on failure.
    // failed_batch >= 0: after the groups the call fails as "injected failure in batch <failed_batch>" (the test aid; the caller
    // has left that batch and the ones behind it out of the plan).  Attached to a stream, the call forks (every lane it uses
    // waits for what the caller's stream holds now: one event) and joins (the caller's stream waits for every such lane: one
    // event per lane) ONCE, whatever the number of groups is: cross-stream events cost tens of microseconds on this runtime and
    // an event per batch degrades the lanes to the serial rate -- hence also the detached form (caller ==
    // DETACHED: no event at all, the caller joins with synchronize()).
    // Error contract: whatever fails, from the first lane operation on, the join is still enqueued and -- on an error return --
    // every lane the call used has been synchronised: "nothing of a failed call is still running", the detached form included.
    // A solo() call runs its groups in order on `self` (the handle's own workspace, pipeline_front.hpp) with the caller's stream
    // as its one lane: no lane stream, no event; on failure the caller's stream is synchronised.
    template <class Prepare, class Launch>
    int run_units(const char *what, const std::vector<PlanGroup> &plan, int failed_batch, void *hip_stream, PipeLane &self,
                  Prepare prepare, Launch launch)
    {
        const bool detached = (hip_stream == DOA_STREAM_DETACHED), alone = solo(hip_stream);
        const bool events = !detached && !alone;           // the fork and the join
        hipStream_t caller = detached ? nullptr : static_cast<hipStream_t>(hip_stream);
        PipeLane *const lane = alone ? &self : lanes;      // solo: the one lane is the handle's own workspace
        const int L = n_lanes;
        // set-up that cannot leave work behind: failures here return at once
        if (events && !fork_ev) DOA_HIP_TRY(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        if (alone) {
            self.st = caller;
        } else {
            hipStream_t have[kMaxLanes], fresh[kMaxLanes];
            int n_have = 0, n_new = 0;
            for (int l = 0; l < L; l++)
                if (lane[l].st) have[n_have++] = lane[l].st;
            if (n_have < L) {
                if (const int rc = create_lane_streams(have, n_have, fresh, L - n_have); rc != DOA_OK) return rc;
                for (int l = 0; l < L; l++)
                    if (!lane[l].st) { lane[l].st = fresh[n_new++]; lane[l].own_stream = true; }
            }
        }
        unsigned used = alone ? 1u : 0u;                   // bit l: lane l runs a unit of this call
        for (const PlanGroup &g : plan) used |= 1u << g.lane;
        for (int l = 0; l < L; l++) {
            auto &ln = lane[l];
            if (events && !ln.done) DOA_HIP_TRY(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
            if (!((used >> l) & 1u)) continue;
            if (const int rc = prepare(ln); rc != DOA_OK) return rc;
        }
        int rc = DOA_OK;
        auto fail = [&](hipError_t e, const char *step) {
            if (e != hipSuccess && rc >= 0) { set_error("%s: %s failed: %s", what, step, hipGetErrorString(e)); rc = DOA_ERR_HIP; }
        };
        // fork: from here on every exit goes through the join and, on failure, the lane synchronisation below
        if (events && used) {
            fail(hipEventRecord(fork_ev, caller), "fork record");
            for (int l = 0; l < L && rc >= 0; l++)
                if ((used >> l) & 1u) fail(hipStreamWaitEvent(lane[l].st, fork_ev, 0), "fork wait");
        }
        for (size_t u = 0; u < plan.size() && rc >= 0; u++) {
            const int r = plan[u].sync_first ? synchronize() : DOA_OK;
            rc = r != DOA_OK ? r : launch(plan[u], lane[plan[u].lane]);
        }
        if (rc >= 0 && failed_batch >= 0) {
            set_error("%s: injected failure in batch %d", what, failed_batch);
            rc = DOA_ERR_HIP;
        }
        for (int l = 0; l < L && events; l++) {
            if (!((used >> l) & 1u)) continue;
            auto &ln = lane[l];
            const hipError_t e1 = hipEventRecord(ln.done, ln.st);
            fail(e1 == hipSuccess ? hipStreamWaitEvent(caller, ln.done, 0) : e1, "join");
        }
        if (rc < 0) {
            const std::string msg = doa_last_error();
            for (int l = 0; l < L; l++)
                if ((used >> l) & 1u) (void)hipStreamSynchronize(lane[l].st);
            set_error("%s", msg.c_str());
        }
        return rc;
    }
};

}  // namespace doa
