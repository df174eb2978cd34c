// spectrum_chain.hpp — the one description of a spectrum estimator and its three steps: a stage in FRONT that turns covariance
// items into per-item records (the eigen stage, or the Capon inverse), a SCAN that turns records into spectrum rows (the
// polynomial scan of a uniform linear array, or the steering-table scan), and a FOLLOW-UP that writes NaN into what the scan
// and the peak pick left for items without a usable record.  The four spectrum blocks (spectrum_blocks.hip) and music_pipeline
// (pipeline.hip) run these functions; a new estimator or geometry is added here, once.  Host-only: the launches are kernels.hpp's.
#pragma once
#include "kernels.hpp"

namespace doa {

// What is being computed.  Exactly one of `ula` and `table` is set.
struct SpectrumDesc {
    int estimator = DOA_ESTIMATOR_MUSIC;
    int N = 0, M = 0, bits = 64;        // N: the elements the front sees (a smoothed handle's subarray); M: MUSIC's source count
    double loading = 0.0;               // Capon
    const MusicTables *ula = nullptr;
    const ArrayTable *table = nullptr;
    const EvdCounts *counts = nullptr;  // a source count per item (MUSIC on a ULA, double)
    int P() const { return table ? table->P : ula->P; }
};

// The records between the front and the scan, in bytes per item; 0 = the record does not exist.  Two facts about slots sized
// from a plan: coefficient slots are sized as doubles (coef_slot) whatever `bits` is, so that a change of the internal
// precision never grows them; and music_pipeline sizes its Chebyshev slots for the G batches of a group on the lean route
// (the group launches write no other record).
struct SpectrumPlan {
    bool ok = false;                    // false: the entries refuse this combination, and the chain does not run it
    size_t coef = 0, coef_slot = 0;     // ULA: coef_stride(N) floats or doubles
    size_t cheb = 0;                    // ULA, N <= 4, double: kChebRecord doubles
    size_t full = 0;                    // table: full_record_len(N) doubles
    size_t status = 0;                  // Capon: one int32
};
// Pure: no HIP call, no device.
inline SpectrumPlan spectrum_plan(int estimator, bool table, int N, int bits, bool counted)
{
    SpectrumPlan p;
    const bool capon = (estimator == DOA_ESTIMATOR_CAPON);
    p.ok = (capon || estimator == DOA_ESTIMATOR_MUSIC) && N >= 2 && N <= DOA_MAX_ANT_ELE && (bits == 64 || bits == 32) &&
           !(bits == 32 && (capon || table || counted)) && !(counted && (capon || table));
    if (!p.ok) return p;
    if (table) p.full = full_record_len(N) * sizeof(double);
    else {
        p.coef = coef_stride(N) * (bits == 64 ? sizeof(double) : sizeof(float));
        p.coef_slot = coef_stride(N) * sizeof(double);
        if (scan_reads_cheb(N, bits)) p.cheb = kChebRecord * sizeof(double);
    }
    if (capon) p.status = sizeof(int);
    return p;
}
inline SpectrumPlan spectrum_plan(const SpectrumDesc &d)
{
    return spectrum_plan(d.estimator, d.table != nullptr, d.N, d.bits, d.counts != nullptr);
}

// The only thing a caller hands from one step to the next (device pointers; NULL = no such record).
struct SpectrumRecords {
    void *coef = nullptr, *cheb = nullptr, *full = nullptr, *status = nullptr;
};

// The four records as a block owns them.
struct SpectrumBufs {
    DevBuf coef, cheb, full, status;
    int reserve(const SpectrumPlan &p, size_t n)
    {
        int rc = coef.reserve(n * p.coef_slot);
        if (rc == DOA_OK) rc = cheb.reserve(n * p.cheb);
        if (rc == DOA_OK) rc = full.reserve(n * p.full);
        if (rc == DOA_OK) rc = status.reserve(n * p.status);
        return rc;
    }
    SpectrumRecords view(const SpectrumPlan &p) const
    {
        return {p.coef ? coef.p : nullptr, p.cheb ? cheb.p : nullptr, p.full ? full.p : nullptr, p.status ? status.p : nullptr};
    }
};

// music_pipeline's peak pick behind the scan: the one-dimensional axis, or the azimuth x elevation grid (then d_argmax holds
// grid->M azimuths and grid->M elevations per item); `scratch` serves the serial pick of unusual vector lengths.
struct SpectrumPick {
    const PeakTables *peaks = nullptr;
    const Peaks2dTables *grid = nullptr;
    void *d_max = nullptr, *d_argmax = nullptr;
    DevBuf *scratch = nullptr;
    size_t reserve_items = 0, item_off = 0;
};

// Each step returns DOA_OK or an error; a description the plan refuses gives DOA_ERR_UNSUPPORTED and no launch.
// Front: d_matrix (optional, diagnostics of a ULA): the projector / the inverse as N x N float2 per item.
int spectrum_front(const SpectrumDesc &d, int n, const void *d_R, const SpectrumRecords &rec, void *d_matrix, hipStream_t st);
// Scan: d_spec = the rows (with a pick and !store_spectrum: scratch rows nobody reads afterwards); d_q (optional): the
// un-normalised null spectrum.
int spectrum_scan(const SpectrumDesc &d, int n, const SpectrumRecords &rec, void *d_spec, void *d_q, bool store_spectrum,
                  const SpectrumPick *pick, hipStream_t st);
// Follow-up: d_spec (optional) = rows a caller sees; pick (optional) = the peak outputs to cover.
int spectrum_follow_up(const SpectrumDesc &d, int n, const SpectrumRecords &rec, void *d_spec, const SpectrumPick *pick, hipStream_t st);

}  // namespace doa
