// source_count.hip — the number of sources per covariance item (Wax-Kailath MDL / AIC on the eigenvalues): C ABI.
//
// Not a block of the reference (gr-doa takes num_targets as a flowgraph parameter).  The work is one launch of the eigen
// stage in its per-item-count form (music_evd.hip: launch_music_evd_counts, estimate mode, no coefficient records): the
// double Jacobi kernels of MUSIC_lin_array with the criterion (jacobi.hpp: source_count_from_eigenvalues) in their epilogues.
#include "kernels.hpp"

struct doa_source_count {
    int N = 0, K = 0, method = 0, kmax = 0;
    int bits = 64;          // the process default at create (doa_set_internal_precision): 32 is not supported
    int device = 0;
    hipStream_t stream = nullptr;
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
    int dev = 0;
    if (doa::ensure_device(&dev) != DOA_OK) return nullptr;
    auto *h = new (std::nothrow) doa_source_count();
    if (!h) { doa::set_error("out of memory"); return nullptr; }
    h->N = num_ant_ele; h->K = num_snapshots; h->method = method; h->kmax = max_sources; h->device = dev;
    h->bits = doa::internal_precision_bits();
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        doa::set_error("source_count: device setup failed");
        doa_source_count_destroy(h);
        return nullptr;
    }
    return h;
}

void doa_source_count_destroy(doa_source_count_t *h)
{
    if (!h) return;
    h->d_in.release(); h->d_count.release(); h->d_eig.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int doa_source_count_work_dev(doa_source_count_t *h, int noutput_items, const void *d_cov_items, void *d_count_out,
                              void *d_eig_out, void *hip_stream)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || (noutput_items > 0 && (!d_cov_items || !d_count_out))) {
        doa::set_error("source_count_work_dev: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (h->bits != 64) {
        doa::set_error("source_count: the criterion needs internal precision 64 (handle is at %d)", h->bits);
        return DOA_ERR_UNSUPPORTED;
    }
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const int rc = doa::launch_music_evd_counts(h->N, noutput_items, d_cov_items, nullptr, d_count_out, d_eig_out, h->K, h->method,
                                                h->kmax, nullptr, nullptr, static_cast<hipStream_t>(hip_stream));
    return rc == DOA_OK ? noutput_items : rc;
}

int doa_source_count_work(doa_source_count_t *h, int noutput_items, const void *cov_items, void *count_out, void *eig_out)
{
    doa::clear_error();
    if (!h || noutput_items < 0 || (noutput_items > 0 && (!cov_items || !count_out))) {
        doa::set_error("source_count_work: bad arguments");
        return DOA_ERR_INVALID_ARG;
    }
    if (noutput_items == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    const size_t in_bytes = (size_t)noutput_items * h->N * h->N * sizeof(float2);
    const size_t cnt_bytes = (size_t)noutput_items * sizeof(int);
    const size_t eig_bytes = (size_t)noutput_items * h->N * sizeof(float);
    int rc = h->d_in.reserve(in_bytes);
    if (rc == DOA_OK) rc = h->d_count.reserve(cnt_bytes);
    if (rc == DOA_OK && eig_out) rc = h->d_eig.reserve(eig_bytes);
    if (rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpyAsync(h->d_in.p, cov_items, in_bytes, hipMemcpyHostToDevice, h->stream));
    rc = doa_source_count_work_dev(h, noutput_items, h->d_in.p, h->d_count.p, eig_out ? h->d_eig.p : nullptr, h->stream);
    if (rc < 0) return rc;
    DOA_HIP_TRY(hipMemcpyAsync(count_out, h->d_count.p, cnt_bytes, hipMemcpyDeviceToHost, h->stream));
    if (eig_out) DOA_HIP_TRY(hipMemcpyAsync(eig_out, h->d_eig.p, eig_bytes, hipMemcpyDeviceToHost, h->stream));
    DOA_HIP_TRY(hipStreamSynchronize(h->stream));
    return noutput_items;
}

}  // extern "C"
