// batch_plan.hpp — the plan of a work_dev_batches call (pipeline.hip, root_pipeline.hip): which consecutive batches form a
// group (one K1, one EVD and one scan launch each), which lane a group runs on, and which groups have to wait for the lanes
// to be joined first.  It is what include/doa_hip.h promises under GROUPS and ORDER.  Pure host logic on pointer values and
// flags: no HIP, no handle; what makes a batch `lean` and which cap it gets is the handle's business.
// tests/test_cpu_batch_plan.py drives it through doa_hip_batch_plan_debug.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace doa {

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

// Plans n_batches batches over L lanes; `rot` is the lane rotation on entry.  traits(b, nb, out) describes batch b: its up to
// four output pointers (NULL = absent; compared, never dereferenced) and nb.lean / nb.store / nb.vec2 / nb.cap.  Consecutive
// lean batches of equal store and vec2 join the open group up to its first batch's cap, unless they write a pointer the group
// writes already or their outputs tie them to another lane.  A group that writes what an earlier group wrote last runs on that
// group's lane (ORDER: the lane's stream keeps the two in call order); one tied to two lanes takes the lane of the pointer
// seen last and gets sync_first; every other group takes the next lane of the rotation.  Returns the rotation on exit.
template <class Traits>
int plan_batches(int n_batches, int L, int rot, Traits &&traits, std::vector<PlanGroup> &plan)
{
    plan.clear();
    PtrGroups writers((size_t)4 * n_batches);
    auto close = [&](PlanGroup &g) {
        g.lane = (g.req >= 0) ? g.req : rot++ % L;
    };
    for (int b = 0; b < n_batches; b++) {
        const void *out[4] = {nullptr, nullptr, nullptr, nullptr};
        PlanGroup nb;
        nb.b0 = b; nb.nb = 1;
        traits(b, nb, out);
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
    return rot % L;
}

}  // namespace doa
