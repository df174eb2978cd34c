// source_count.hip — the number of sources per covariance item (Wax-Kailath MDL / AIC on the eigenvalues): C ABI.
//
// Not a block of the reference (gr-doa takes num_targets as a flowgraph parameter).  The work is one launch of the eigen
// stage in its per-item-count form (music_evd.hip: launch_music_evd_counts, estimate mode, no coefficient records): the
// double Jacobi kernels of MUSIC_lin_array with the criterion (jacobi.hpp: source_count_from_eigenvalues) in their epilogues.
#include "kernels.hpp"

#include "block_host.hpp"

struct doa_source_count : doa::BlockBase {             // bits: 32 is not supported
    int N = 0, K = 0, method = 0, kmax = 0;
    doa::DevBuf d_in, d_count, d_eig;
};

extern "C" {

doa_source_count_t *doa_source_count_create(int num_ant_ele, int num_snapshots, int method, int max_sources)
{
    doa::clear_error();
    if (num_ant_ele < 2 || num_snapshots < 2 || (method != DOA_SOURCE_COUNT_MDL && method != DOA_SOURCE_COUNT_AIC) ||
        max_sources < 1 || max_sources > num_ant_ele - 1) {
        doa::set_error("source_count: need num_ant_ele >= 2, num_snapshots >= 2, method 0 (MDL) or 1 (AIC), "
                       "1 <= max_sources < num_ant_ele (got %d, %d, %d, %d)", num_ant_ele, num_snapshots, method, max_sources);
        return nullptr;
    }
    if (num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("source_count: num_ant_ele=%d exceeds DOA_MAX_ANT_ELE=%d", num_ant_ele, DOA_MAX_ANT_ELE);
        return nullptr;
    }
    return doa::create_block<doa_source_count>("source_count", [&](doa_source_count &h) {
        h.N = num_ant_ele; h.K = num_snapshots; h.method = method; h.kmax = max_sources;
        return DOA_OK;
    });
}

void doa_source_count_destroy(doa_source_count_t *h) { doa::destroy_block(h); }

int doa_source_count_work_dev(doa_source_count_t *h, int noutput_items, const void *d_cov_items, void *d_count_out,
                              void *d_eig_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("source_count_work_dev", h, noutput_items, {d_cov_items, d_count_out}); rc != DOA_OK) return rc;
    if (int rc = doa::need_bits64("source_count_work_dev", h->bits, "the criterion"); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const doa::EvdCounts cnt = doa::evd_counts_estimate((int *)d_count_out, (float *)d_eig_out, h->K, h->method, h->kmax);
    const int rc = doa::launch_music_evd_counts(h->N, noutput_items, d_cov_items, cnt, doa::EvdOut{}, static_cast<hipStream_t>(hip_stream));
    return rc == DOA_OK ? noutput_items : rc;
}

int doa_source_count_work(doa_source_count_t *h, int noutput_items, const void *cov_items, void *count_out, void *eig_out)
{
    doa::clear_error();
    if (int rc = doa::work_args("source_count_work", h, noutput_items, {cov_items, count_out}); rc != DOA_OK) return rc;
    if (noutput_items == 0) return 0;
    doa::HostCall io(*h);
    io.in(h->d_in, cov_items, (size_t)noutput_items * h->N * h->N * sizeof(float2));
    io.out(h->d_count, count_out, (size_t)noutput_items * sizeof(int));
    if (eig_out) io.out(h->d_eig, eig_out, (size_t)noutput_items * h->N * sizeof(float));
    int rc = io.status();
    // (work_dev refuses a handle at internal precision 32)
    if (rc == DOA_OK) rc = doa_source_count_work_dev(h, noutput_items, h->d_in.p, h->d_count.p, eig_out ? h->d_eig.p : nullptr, h->stream);
    return io.finish(rc);
}

}  // extern "C"
