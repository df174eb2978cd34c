// gridfree_chain.hip — the eigen launch and the solver launch of a grid-free estimator (gridfree_chain.hpp).  Host-only.
#include "gridfree_chain.hpp"

namespace doa {

int gridfree_run(const GridfreeDesc &d, int n, const void *d_cov, const EvdCounts *counts, const GridfreeRecords &rec,
                 void *d_angles, void *d_status, hipStream_t st, void *d_roots)
{
    if (!gridfree_plan(d, counts != nullptr).ok) {
        set_error("grid-free chain: no launch for estimator %d at %d elements, internal precision %d%s", d.estimator, d.N, d.bits,
                  counts ? ", per-item counts" : "");
        return DOA_ERR_UNSUPPORTED;
    }
    if (!d_status) d_status = rec.status;
    // the counts the solver reads: the caller's, or the ones the eigen launch is about to estimate
    const void *d_counts = !counts ? nullptr : counts->counts_in ? (const void *)counts->counts_in : counts->count_out;
    const bool estimate = counts && !counts->counts_in;
    EvdOut out;
    int rc;
    if (d.estimator == DOA_GRIDFREE_ESPRIT) {
        // the record does not depend on a count: only an estimate needs the counting launch
        out.es_rec = (double *)rec.rec;
        rc = estimate ? launch_music_evd_counts(d.N, n, d_cov, *counts, out, st) : launch_music_evd_record(d.N, n, d_cov, rec.rec, st);
        if (rc != DOA_OK) return rc;
        return launch_esprit(d.N, d.M, d.norm_spacing, n, d_cov, rec.rec, d_counts, d_angles, d_status, st);
    }
    // each item's record for its own noise set (a count outside 0..N-1: a NaN record, which the root kernel does not read)
    out.coef_d = (double *)rec.coef;
    rc = counts ? launch_music_evd_counts(d.N, n, d_cov, *counts, out, st) : launch_music_evd(d.N, d.M, n, d_cov, out, d.bits, st);
    if (rc != DOA_OK) return rc;
    if (counts) return launch_root_music_counts(d.N, d.M, d.norm_spacing, n, rec.coef, d_counts, d_angles, d_status, st, d_roots);
    return launch_root_music(d.N, d.M, d.norm_spacing, n, rec.coef, d_angles, d_status, st, d_roots);
}

}  // namespace doa

// ---- the plan of a description, for the tests (include/doa_hip_test.h): no handle, no device ------------------------------
extern "C" int doa_hip_gridfree_plan_debug(int estimator, int num_ant_ele, int bits, int counted, long long *bytes_out)
{
    doa::clear_error();
    if (!bytes_out || (counted != 0 && counted != 1)) {
        doa::set_error("hip_gridfree_plan_debug: bad arguments (bytes_out, counted = 0 or 1)");
        return DOA_ERR_INVALID_ARG;
    }
    const doa::GridfreePlan p = doa::gridfree_plan(estimator, num_ant_ele, bits, counted != 0);
    const size_t v[3] = {p.coef, p.rec, p.status};
    for (int k = 0; k < 3; k++) bytes_out[k] = (long long)v[k];
    if (p.ok) return DOA_OK;
    doa::set_error("hip_gridfree_plan_debug: no entry runs estimator %d at %d elements, internal precision %d, counted %d", estimator,
                   num_ant_ele, bits, counted);
    return DOA_ERR_UNSUPPORTED;
}
