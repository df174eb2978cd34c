// spectrum_blocks.hip — the C ABI of the four spectrum blocks: MUSIC_lin_array and capon_lin_array (a uniform linear array),
// MUSIC_array and capon_array (a steering table).  One handle base and one copy of work_dev, work and the two debug shapes;
// what differs between the blocks is their description (spectrum_chain.hpp), which the chain's three steps turn into launches.
// The kernels, launchers and tables are in music.hip, music_evd.hip, capon.hip and array_scan.hip.  Host-only.
#include "block_host.hpp"
#include "spectrum_chain.hpp"

#include <cmath>
#include <vector>

struct SpectrumBlock : doa::BlockBase {
    doa::SpectrumDesc desc;         // ula / table point at the member the block built; bits is filled in per call
    doa::MusicTables ula;
    doa::ArrayTable table;
    doa::SpectrumBufs recs;
    doa::DevBuf d_in, d_out, d_q, d_diag, d_counts;
};
struct doa_MUSIC_lin_array : SpectrumBlock {};
struct doa_capon_lin_array : SpectrumBlock {};
struct doa_MUSIC_array : SpectrumBlock {};
struct doa_capon_array : SpectrumBlock {};

namespace {

int block_args(const char *who, const SpectrumBlock *h, int n, std::initializer_list<const void *> required, int min_n = 0,
               const char *what = nullptr)
{
    if (int rc = doa::work_args(who, h, n, required, min_n); rc != DOA_OK) return rc;
    // what of the block needs internal precision 64 (MUSIC on a ULA runs at 32 too)
    if (!what) what = h->desc.table ? "the steering-table scan" : h->desc.estimator == DOA_ESTIMATOR_CAPON ? "the Capon inverse" : nullptr;
    return what ? doa::need_bits64(who, h->bits, what) : DOA_OK;
}

doa::SpectrumDesc desc_of(const SpectrumBlock *h, const doa::EvdCounts *counts = nullptr)
{
    doa::SpectrumDesc d = h->desc;
    d.bits = h->bits;
    d.counts = counts;
    return d;
}

size_t cov_bytes(const SpectrumBlock *h, int n) { return (size_t)n * h->desc.N * h->desc.N * sizeof(float2); }
size_t spec_bytes(const SpectrumBlock *h, int n) { return (size_t)n * h->desc.P() * sizeof(float); }

// the checks of a work entry; counted: the *_counts entries, which require the counts and internal precision 64
int work_entry_args(const char *who, const SpectrumBlock *h, int n, const void *cov, const void *counts, bool counted, const void *spec)
{
    return counted ? block_args(who, h, n, {cov, counts, spec}, 0, "per-item counts") : block_args(who, h, n, {cov, spec});
}

// work_dev of the four blocks and work_dev_counts; d_status_out: Capon's optional port
int block_work_dev(const char *who, SpectrumBlock *h, int n, const void *d_cov, const void *d_counts, bool counted, void *d_spec,
                   void *d_status_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = work_entry_args(who, h, n, d_cov, d_counts, counted, d_spec); rc != DOA_OK) return rc;
    if (n == 0) return 0;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const doa::EvdCounts cnt = doa::evd_counts_forced((const int *)d_counts);
    const doa::SpectrumDesc d = desc_of(h, counted ? &cnt : nullptr);
    doa::SpectrumPlan plan = doa::spectrum_plan(d);
    if (d_status_out) plan.status = 0;                   // the caller's status words serve
    int rc = h->recs.reserve(plan, (size_t)n);
    if (rc != DOA_OK) return rc;
    doa::SpectrumRecords rec = h->recs.view(plan);
    if (d_status_out) rec.status = d_status_out;
    rc = doa::spectrum_front(d, n, d_cov, rec, nullptr, st);
    if (rc == DOA_OK) rc = doa::spectrum_scan(d, n, rec, d_spec, nullptr, true, nullptr, st);
    if (rc == DOA_OK) rc = doa::spectrum_follow_up(d, n, rec, d_spec, nullptr, st);
    if (rc != DOA_OK) return rc;
    h->items_total += n;
    return n;
}

// the host entries: who_dev names the device entry that does the work (and the checks again, under its own name)
int block_work(const char *who, const char *who_dev, SpectrumBlock *h, int n, const void *cov, const void *counts, bool counted,
               void *spec, void *status_out)
{
    doa::clear_error();
    if (int rc = work_entry_args(who, h, n, cov, counts, counted, spec); rc != DOA_OK) return rc;
    if (n == 0) return 0;
    const bool capon = (h->desc.estimator == DOA_ESTIMATOR_CAPON);
    doa::HostCall io(*h);
    io.in(h->d_in, cov, cov_bytes(h, n));
    if (counted) io.in(h->d_counts, counts, (size_t)n * sizeof(int));
    io.out(h->d_out, spec, spec_bytes(h, n));
    if (capon) io.out(h->recs.status, status_out, (size_t)n * sizeof(int));
    int rc = io.status();
    if (rc == DOA_OK)
        rc = block_work_dev(who_dev, h, n, h->d_in.p, h->d_counts.p, counted, h->d_out.p, capon ? h->recs.status.p : nullptr, h->stream);
    return io.finish(rc);
}

// The body of the debug entries: items up, the front (no status port), the scan with its null spectrum, `matrix` and the null
// spectrum down (either host pointer may be NULL).  matrix: the buffer of matrix_bytes that comes down as the front's matrix
// -- the diagnostic N x N float2 output (front_writes_it), or the full records themselves
int debug_run(SpectrumBlock *h, int n, const void *cov, doa::DevBuf &matrix, void *matrix_host, size_t matrix_bytes,
              bool front_writes_it, void *null_spectrum_out)
{
    const doa::SpectrumDesc d = desc_of(h);
    doa::SpectrumPlan plan = doa::spectrum_plan(d);
    plan.status = 0;
    doa::HostCall io(*h);
    io.in(h->d_in, cov, cov_bytes(h, n));
    io.out(h->d_out, nullptr, spec_bytes(h, n));
    io.out(h->d_q, null_spectrum_out, spec_bytes(h, n));
    io.out(matrix, matrix_host, matrix_bytes);
    int rc = io.status();
    if (rc == DOA_OK) rc = h->recs.reserve(plan, (size_t)n);
    const doa::SpectrumRecords rec = h->recs.view(plan);
    if (rc == DOA_OK) rc = doa::spectrum_front(d, n, h->d_in.p, rec, front_writes_it ? matrix.p : nullptr, h->stream);
    if (rc == DOA_OK) rc = doa::spectrum_scan(d, n, rec, h->d_out.p, h->d_q.p, true, nullptr, h->stream);
    return io.finish(rc == DOA_OK ? n : rc);
}

// debug on a uniform linear array: the front's matrix (projector / inverse) as N x N float2
int ula_debug(const char *who, SpectrumBlock *h, int n, const void *cov, void *matrix_out, void *null_spectrum_out)
{
    doa::clear_error();
    if (int rc = block_args(who, h, n, {cov}, 1); rc != DOA_OK) return rc;
    return debug_run(h, n, cov, h->d_diag, matrix_out, cov_bytes(h, n), true, null_spectrum_out);
}

// full records (host) -> N x N complex128, column-major
void unpack_full_records(const std::vector<double> &rec, int N, int n, double *out)
{
    const size_t NN = (size_t)N * N;
    for (int it = 0; it < n; it++) {
        const double *f = rec.data() + (size_t)it * NN;
        double *o = out + 2 * (size_t)it * NN;
        for (int c = 0; c < N; c++) {
            o[2 * (c + c * N)] = f[c + c * N]; o[2 * (c + c * N) + 1] = 0.0;
            for (int r = 0; r < c; r++) {
                const double re = f[r + c * N], im = f[c + r * N];
                o[2 * (r + c * N)] = re; o[2 * (r + c * N) + 1] = im;
                o[2 * (c + r * N)] = re; o[2 * (c + r * N) + 1] = -im;
            }
        }
    }
}

// debug on a steering table: the block's full records, unpacked to complex128
int table_debug(const char *who, SpectrumBlock *h, int n, const void *cov, void *matrix_out, void *null_spectrum_out)
{
    doa::clear_error();
    if (int rc = block_args(who, h, n, {cov}, 1); rc != DOA_OK) return rc;
    const int N = h->desc.N;
    std::vector<double> rec(matrix_out ? (size_t)n * doa::full_record_len(N) : 0);
    const int rc = debug_run(h, n, cov, h->recs.full, matrix_out ? rec.data() : nullptr,
                             (size_t)n * doa::full_record_len(N) * sizeof(double), false, null_spectrum_out);
    if (rc >= 0 && matrix_out) unpack_full_records(rec, N, n, static_cast<double *>(matrix_out));
    return rc;
}

int set_bits(const char *who, SpectrumBlock *h, int bits)
{
    doa::clear_error();
    if (!h || (bits != 32 && bits != 64)) { doa::set_error("%s: need a handle and bits = 32 or 64", who); return DOA_ERR_INVALID_ARG; }
    h->bits = bits;
    return DOA_OK;
}

bool loading_ok(const char *who, float diagonal_loading)
{
    if (std::isfinite(diagonal_loading) && diagonal_loading >= 0.0f) return true;
    doa::set_error("%s: diagonal_loading must be finite and >= 0 (got %g)", who, (double)diagonal_loading);
    return false;
}

// the tail of the four creates: the description, then the table it points at
template <class H> H *create(const char *who, int estimator, int N, int M, double loading, float norm_spacing,
                             int pspectrum_len, const double *steering)
{
    return doa::create_block<H>(who, [&](H &h) {
        h.desc.estimator = estimator; h.desc.N = N; h.desc.M = M; h.desc.loading = loading;
        if (steering) { h.desc.table = &h.table; return h.table.build(N, pspectrum_len, steering); }
        h.desc.ula = &h.ula;
        return h.ula.build(norm_spacing, M, N, pspectrum_len);      // (Capon passes M = 1: the scan does not use it)
    });
}

}  // namespace

extern "C" {

// ---- MUSIC_lin_array ----------------------------------------------------------------------------------------------------
doa_MUSIC_lin_array_t *doa_MUSIC_lin_array_create(float norm_spacing, int num_targets, int num_ant_ele, int pspectrum_len)
{
    doa::clear_error();
    // grc/doa_MUSIC_lin_array.xml:33-35 (inputs > 0, inputs > num_targets, norm_spacing <= 0.5); the reference ctor does not
    // validate (num_targets >= N would index cols(0,-1)), so create fails here.
    if (num_ant_ele <= 0 || num_targets <= 0 || num_targets >= num_ant_ele) {
        doa::set_error("MUSIC_lin_array: need 0 < num_targets < num_ant_ele (got %d, %d)", num_targets, num_ant_ele);
        return nullptr;
    }
    if (!(norm_spacing > 0.0f) || norm_spacing > 0.5f) {
        doa::set_error("MUSIC_lin_array: need 0 < norm_spacing <= 0.5 (got %g)", (double)norm_spacing);
        return nullptr;
    }
    if (num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("MUSIC_lin_array: num_ant_ele=%d exceeds DOA_MAX_ANT_ELE=%d", num_ant_ele, DOA_MAX_ANT_ELE);
        return nullptr;
    }
    if (pspectrum_len <= 0) {
        doa::set_error("MUSIC_lin_array: pspectrum_len must be > 0 (got %d)", pspectrum_len);
        return nullptr;
    }
    return create<doa_MUSIC_lin_array>("MUSIC_lin_array", DOA_ESTIMATOR_MUSIC, num_ant_ele, num_targets, 0.0, norm_spacing,
                                       pspectrum_len, nullptr);
}
void doa_MUSIC_lin_array_destroy(doa_MUSIC_lin_array_t *h) { doa::destroy_block(h); }
long long doa_MUSIC_lin_array_items_total(const doa_MUSIC_lin_array_t *h) { return h ? h->items_total : 0; }
int doa_MUSIC_lin_array_set_internal_precision(doa_MUSIC_lin_array_t *h, int bits)
{
    return set_bits("MUSIC_lin_array_set_internal_precision", h, bits);
}
int doa_MUSIC_lin_array_work_dev(doa_MUSIC_lin_array_t *h, int noutput_items, const void *d_input_items0, void *d_output_items0,
                                 void *hip_stream)
{
    return block_work_dev("MUSIC_lin_array_work_dev", h, noutput_items, d_input_items0, nullptr, false, d_output_items0, nullptr, hip_stream);
}
int doa_MUSIC_lin_array_work(doa_MUSIC_lin_array_t *h, int noutput_items, const void *input_items0, void *output_items0)
{
    return block_work("MUSIC_lin_array_work", "MUSIC_lin_array_work_dev", h, noutput_items, input_items0, nullptr, false, output_items0, nullptr);
}
int doa_MUSIC_lin_array_work_dev_counts(doa_MUSIC_lin_array_t *h, int noutput_items, const void *d_cov_items, const void *d_counts,
                                        void *d_spectrum_out, void *hip_stream)
{
    return block_work_dev("MUSIC_lin_array_work_dev_counts", h, noutput_items, d_cov_items, d_counts, true, d_spectrum_out, nullptr, hip_stream);
}
int doa_MUSIC_lin_array_work_counts(doa_MUSIC_lin_array_t *h, int noutput_items, const void *cov_items, const void *counts,
                                    void *spectrum_out)
{
    return block_work("MUSIC_lin_array_work_counts", "MUSIC_lin_array_work_dev_counts", h, noutput_items, cov_items, counts, true,
                      spectrum_out, nullptr);
}
int doa_MUSIC_lin_array_debug(doa_MUSIC_lin_array_t *h, int noutput_items, const void *input_items0, void *projector_out,
                              void *null_spectrum_out)
{
    return ula_debug("MUSIC_lin_array_debug", h, noutput_items, input_items0, projector_out, null_spectrum_out);
}

// ---- capon_lin_array ----------------------------------------------------------------------------------------------------
doa_capon_lin_array_t *doa_capon_lin_array_create(float norm_spacing, int num_ant_ele, int pspectrum_len, float diagonal_loading)
{
    doa::clear_error();
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("capon_lin_array: need 2 <= num_ant_ele <= %d (got %d)", DOA_MAX_ANT_ELE, num_ant_ele);
        return nullptr;
    }
    if (!(norm_spacing > 0.0f) || norm_spacing > 0.5f) {
        doa::set_error("capon_lin_array: need 0 < norm_spacing <= 0.5 (got %g)", (double)norm_spacing);
        return nullptr;
    }
    if (pspectrum_len <= 0) {
        doa::set_error("capon_lin_array: pspectrum_len must be > 0 (got %d)", pspectrum_len);
        return nullptr;
    }
    if (!loading_ok("capon_lin_array", diagonal_loading)) return nullptr;
    return create<doa_capon_lin_array>("capon_lin_array", DOA_ESTIMATOR_CAPON, num_ant_ele, 1, (double)diagonal_loading,
                                       norm_spacing, pspectrum_len, nullptr);
}
void doa_capon_lin_array_destroy(doa_capon_lin_array_t *h) { doa::destroy_block(h); }
long long doa_capon_lin_array_items_total(const doa_capon_lin_array_t *h) { return h ? h->items_total : 0; }
int doa_capon_lin_array_work_dev(doa_capon_lin_array_t *h, int noutput_items, const void *d_cov_items, void *d_spectrum_out,
                                 void *d_status_out, void *hip_stream)
{
    return block_work_dev("capon_lin_array_work_dev", h, noutput_items, d_cov_items, nullptr, false, d_spectrum_out, d_status_out, hip_stream);
}
int doa_capon_lin_array_work(doa_capon_lin_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out, void *status_out)
{
    return block_work("capon_lin_array_work", "capon_lin_array_work_dev", h, noutput_items, cov_items, nullptr, false, spectrum_out, status_out);
}
int doa_capon_lin_array_debug(doa_capon_lin_array_t *h, int noutput_items, const void *cov_items, void *inverse_out,
                              void *null_spectrum_out)
{
    return ula_debug("capon_lin_array_debug", h, noutput_items, cov_items, inverse_out, null_spectrum_out);
}

// ---- MUSIC_array and capon_array ----------------------------------------------------------------------------------------
doa_MUSIC_array_t *doa_MUSIC_array_create(int num_targets, int num_ant_ele, int pspectrum_len, const double *steering)
{
    doa::clear_error();
    if (doa::steering_table_args("MUSIC_array", num_ant_ele, pspectrum_len, steering) != DOA_OK) return nullptr;
    if (num_targets < 1 || num_targets >= num_ant_ele) {
        doa::set_error("MUSIC_array: need 0 < num_targets < num_ant_ele (got %d, %d)", num_targets, num_ant_ele);
        return nullptr;
    }
    return create<doa_MUSIC_array>("MUSIC_array", DOA_ESTIMATOR_MUSIC, num_ant_ele, num_targets, 0.0, 0.f,
                                   pspectrum_len, steering);
}
void doa_MUSIC_array_destroy(doa_MUSIC_array_t *h) { doa::destroy_block(h); }
long long doa_MUSIC_array_items_total(const doa_MUSIC_array_t *h) { return h ? h->items_total : 0; }
int doa_MUSIC_array_set_internal_precision(doa_MUSIC_array_t *h, int bits) { return set_bits("MUSIC_array_set_internal_precision", h, bits); }
int doa_MUSIC_array_work_dev(doa_MUSIC_array_t *h, int noutput_items, const void *d_cov_items, void *d_spectrum_out, void *hip_stream)
{
    return block_work_dev("MUSIC_array_work_dev", h, noutput_items, d_cov_items, nullptr, false, d_spectrum_out, nullptr, hip_stream);
}
int doa_MUSIC_array_work(doa_MUSIC_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out)
{
    return block_work("MUSIC_array_work", "MUSIC_array_work_dev", h, noutput_items, cov_items, nullptr, false, spectrum_out, nullptr);
}
int doa_MUSIC_array_debug(doa_MUSIC_array_t *h, int noutput_items, const void *cov_items, void *projector_out, void *null_spectrum_out)
{
    return table_debug("MUSIC_array_debug", h, noutput_items, cov_items, projector_out, null_spectrum_out);
}

doa_capon_array_t *doa_capon_array_create(int num_ant_ele, int pspectrum_len, const double *steering, float diagonal_loading)
{
    doa::clear_error();
    if (doa::steering_table_args("capon_array", num_ant_ele, pspectrum_len, steering) != DOA_OK) return nullptr;
    if (!loading_ok("capon_array", diagonal_loading)) return nullptr;
    return create<doa_capon_array>("capon_array", DOA_ESTIMATOR_CAPON, num_ant_ele, 0, (double)diagonal_loading, 0.f,
                                   pspectrum_len, steering);
}
void doa_capon_array_destroy(doa_capon_array_t *h) { doa::destroy_block(h); }
long long doa_capon_array_items_total(const doa_capon_array_t *h) { return h ? h->items_total : 0; }
int doa_capon_array_work_dev(doa_capon_array_t *h, int noutput_items, const void *d_cov_items, void *d_spectrum_out,
                             void *d_status_out, void *hip_stream)
{
    return block_work_dev("capon_array_work_dev", h, noutput_items, d_cov_items, nullptr, false, d_spectrum_out, d_status_out, hip_stream);
}
int doa_capon_array_work(doa_capon_array_t *h, int noutput_items, const void *cov_items, void *spectrum_out, void *status_out)
{
    return block_work("capon_array_work", "capon_array_work_dev", h, noutput_items, cov_items, nullptr, false, spectrum_out, status_out);
}
int doa_capon_array_debug(doa_capon_array_t *h, int noutput_items, const void *cov_items, void *inverse_out, void *null_spectrum_out)
{
    return table_debug("capon_array_debug", h, noutput_items, cov_items, inverse_out, null_spectrum_out);
}

// ---- the plan of a description, for the tests (include/doa_hip_test.h): no handle, no device ------------------------------
int doa_hip_spectrum_plan_debug(int estimator, int steering_table, int num_ant_ele, int bits, int counted, long long *bytes_out)
{
    doa::clear_error();
    if (!bytes_out || (steering_table != 0 && steering_table != 1) || (counted != 0 && counted != 1)) {
        doa::set_error("hip_spectrum_plan_debug: bad arguments (bytes_out, steering_table = 0 or 1, counted = 0 or 1)");
        return DOA_ERR_INVALID_ARG;
    }
    const doa::SpectrumPlan p = doa::spectrum_plan(estimator, steering_table != 0, num_ant_ele, bits, counted != 0);
    const size_t v[5] = {p.coef, p.cheb, p.full, p.status, p.coef_slot};
    for (int k = 0; k < 5; k++) bytes_out[k] = (long long)v[k];
    if (p.ok) return DOA_OK;
    doa::set_error("hip_spectrum_plan_debug: no entry runs estimator %d at %d elements, internal precision %d, steering_table %d, counted %d",
                   estimator, num_ant_ele, bits, steering_table, counted);
    return DOA_ERR_UNSUPPORTED;
}

}  // extern "C"
