// spectrum_chain.hip — the front, the scan and the follow-up of a spectrum estimator (spectrum_chain.hpp).  Host-only.
#include "spectrum_chain.hpp"

namespace doa {

static int check(const SpectrumDesc &d)
{
    if (spectrum_plan(d).ok && (d.ula != nullptr) != (d.table != nullptr)) return DOA_OK;
    set_error("spectrum chain: no launch for estimator %d at %d elements, internal precision %d%s%s", d.estimator, d.N, d.bits,
              d.table ? ", a steering table" : "", d.counts ? ", per-item counts" : "");
    return DOA_ERR_UNSUPPORTED;
}

int spectrum_front(const SpectrumDesc &d, int n, const void *d_R, const SpectrumRecords &rec, void *d_matrix, hipStream_t st)
{
    if (int rc = check(d); rc != DOA_OK) return rc;
    if (d.estimator == DOA_ESTIMATOR_CAPON) {
        CaponOut out;
        out.coef_d = (double *)rec.coef; out.cheb_d = (double *)rec.cheb; out.w_out = (float2 *)d_matrix;
        out.full = (double *)rec.full; out.status = (int *)rec.status;
        return launch_capon_inverse(d.N, n, d_R, d.loading, out, st);
    }
    if (d.table) return launch_music_evd_full(d.N, d.M, n, d_R, rec.full, d_matrix, st);
    EvdOut out;
    if (d.bits == 64) out.coef_d = (double *)rec.coef;
    else out.coef = (float *)rec.coef;
    out.cheb_d = (double *)rec.cheb;
    out.pn_out = (float2 *)d_matrix;
    if (d.counts) return launch_music_evd_counts(d.N, n, d_R, *d.counts, out, st);
    return launch_music_evd(d.N, d.M, n, d_R, out, d.bits, st);
}

int spectrum_scan(const SpectrumDesc &d, int n, const SpectrumRecords &rec, void *d_spec, void *d_q, bool store_spectrum,
                  const SpectrumPick *pick, hipStream_t st)
{
    if (int rc = check(d); rc != DOA_OK) return rc;
    if (pick && pick->grid) {
        // grid mode: the scan and find_local_max_2d's pick on the row in LDS are ONE launch, which stores a row only for a
        // caller that asked for it (a grid too large for LDS is two launches and borrows the scratch rows)
        const int M = pick->grid->M;
        void *rows = (store_spectrum || d.table->P > kArrayGridFusedMax) ? d_spec : nullptr;
        float *az = static_cast<float *>(pick->d_argmax);
        return launch_array_scan_peaks2d(*d.table, *pick->grid, n, rec.full, rows, pick->d_max, az, az + M, 2 * M, st);
    }
    bool peaks_done = false;
    int rc;
    if (d.table) rc = launch_array_scan(*d.table, n, rec.full, d_spec, d_q, st);
    else
        rc = launch_music_scan(*d.ula, d.bits, n, rec.coef, d_spec, d_q, st, pick ? pick->peaks : nullptr, pick ? pick->d_max : nullptr,
                               pick ? pick->d_argmax : nullptr, &peaks_done, store_spectrum, rec.cheb);
    if (rc == DOA_OK && pick && !peaks_done)
        rc = launch_peak_pick(*pick->peaks, n, d_spec, nullptr, pick->d_max, pick->d_argmax, *pick->scratch, pick->reserve_items,
                              pick->item_off, st);
    return rc;
}

// The scan kernels write 0.0 dB rows (and the peak pick their peaks) for a NaN record: a Capon item of status 1, or an item
// whose count is outside 0..N-1.  These launches leave NaN there instead.
int spectrum_follow_up(const SpectrumDesc &d, int n, const SpectrumRecords &rec, void *d_spec, const SpectrumPick *pick, hipStream_t st)
{
    if (int rc = check(d); rc != DOA_OK) return rc;
    if (d.counts) {
        const void *counts = d.counts->counts_in ? (const void *)d.counts->counts_in : d.counts->count_out;
        return d_spec ? launch_music_invalid_rows(d.N, d.P(), n, counts, d_spec, st) : DOA_OK;
    }
    if (d.estimator != DOA_ESTIMATOR_CAPON) return DOA_OK;
    // the row and the peaks; in grid mode (3 M values per item) a second launch covers the 2 M wide argmax
    const bool grid = pick && pick->grid;
    const int M = !pick ? 0 : grid ? pick->grid->M : pick->peaks->M;
    void *mx = pick ? pick->d_max : nullptr, *am = pick ? pick->d_argmax : nullptr;
    const struct { int P, M; void *spec, *mx, *am; } launch[2] = {{d.P(), M, d_spec, mx, grid ? nullptr : am}, {0, 2 * M, nullptr, nullptr, am}};
    int rc = DOA_OK;
    for (int k = 0; k < (grid ? 2 : 1) && rc == DOA_OK; k++)
        rc = launch_capon_invalid_rows(launch[k].P, launch[k].M, n, rec.status, launch[k].spec, launch[k].mx, launch[k].am, st);
    return rc;
}

}  // namespace doa
