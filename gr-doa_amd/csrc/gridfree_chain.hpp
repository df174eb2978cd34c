// gridfree_chain.hpp — the one description of a grid-free estimator (Root-MUSIC, ESPRIT) and its two steps: the EIGEN launch
// that turns covariance items into per-item records, and the SOLVER kernel that turns records into angles and status words.
// The two blocks (root_music.hip, esprit.hip) and root_pipeline (root_pipeline.hip) run gridfree_run; which record which
// estimator needs, at which precision and with which kind of source count, is stated here, once, and a new grid-free
// estimator is added here.  Host-only: the launches are kernels.hpp's.
#pragma once
#include "kernels.hpp"

namespace doa {

// What is being computed.
struct GridfreeDesc {
    int estimator = DOA_GRIDFREE_ROOT_MUSIC;
    int N = 0, M = 0;                   // N: the elements the eigen stage sees (a smoothed handle's subarray); M: num_targets,
                                        // and the item width of the counted forms
    float norm_spacing = 0.f;
    int bits = 64;
};
// The source count of a run is an optional EvdCounts (kernels.hpp): NULL = M sources for every item; evd_counts_forced = a
// count per item from the caller; evd_counts_estimate = a count per item from its eigenvalues, written to count_out.

// The records between the eigen launch and the solver, in bytes per item; 0 = the record does not exist.
struct GridfreePlan {
    bool ok = false;                    // false: the entries refuse this combination, and the chain does not run it
    size_t coef = 0;                    // Root-MUSIC: coef_stride(N) doubles (at 32 bits too: the root finder reads doubles)
    size_t rec = 0;                     // ESPRIT: subspace_record_len(N) doubles
    size_t status = 0;                  // one int32
};
// Pure: no HIP call, no device.
inline GridfreePlan gridfree_plan(int estimator, int N, int bits, bool counted)
{
    GridfreePlan p;
    const bool esprit = (estimator == DOA_GRIDFREE_ESPRIT);
    p.ok = (esprit || estimator == DOA_GRIDFREE_ROOT_MUSIC) && N >= 2 && N <= DOA_MAX_ANT_ELE && (bits == 64 || bits == 32) &&
           !(bits == 32 && (esprit || counted));
    if (!p.ok) return p;
    if (esprit) p.rec = subspace_record_len(N) * sizeof(double);
    else p.coef = coef_stride(N) * sizeof(double);
    p.status = sizeof(int);
    return p;
}
inline GridfreePlan gridfree_plan(const GridfreeDesc &d, bool counted) { return gridfree_plan(d.estimator, d.N, d.bits, counted); }

// The only thing a caller hands from the eigen launch to the solver (device pointers; NULL = no such record).
struct GridfreeRecords {
    void *coef = nullptr, *rec = nullptr, *status = nullptr;
};

// The three records as a block owns them.  own_status = false: every item's status word goes to the caller's buffer.
struct GridfreeBufs {
    DevBuf coef, rec, status;
    int reserve(const GridfreePlan &p, size_t n, bool own_status = true)
    {
        int rc = coef.reserve(n * p.coef);
        if (rc == DOA_OK) rc = rec.reserve(n * p.rec);
        if (rc == DOA_OK && own_status) rc = status.reserve(n * p.status);
        return rc;
    }
    GridfreeRecords view(const GridfreePlan &p) const { return {p.coef ? coef.p : nullptr, p.rec ? rec.p : nullptr, status.p}; }
};

// The eigen launch for the description and the count mode, then the solver launch: DOA_OK or the launcher's error; a
// description the plan refuses gives DOA_ERR_UNSUPPORTED and no launch.  d_status: the caller's status words, or NULL for
// rec.status (ESPRIT runs with neither: its kernel skips the store).  d_roots (optional, Root-MUSIC's diagnostics): the
// roots found per item.
int gridfree_run(const GridfreeDesc &d, int n, const void *d_cov, const EvdCounts *counts, const GridfreeRecords &rec,
                 void *d_angles, void *d_status, hipStream_t st, void *d_roots = nullptr);

// A host entry's scan of the status words it copied back: the first item whose word is an error, or -1.  Any non-zero word
// is one; counted (the counted host entry of the Root-MUSIC block): only 1 is, because 2 = no usable count is what the
// caller asked for.  The message is the caller's.
inline int gridfree_first_error(const int *status, int n, bool counted = false)
{
    for (int i = 0; i < n; i++)
        if (counted ? status[i] == 1 : status[i] != 0) return i;
    return -1;
}

}  // namespace doa
