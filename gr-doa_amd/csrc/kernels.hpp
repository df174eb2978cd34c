// kernels.hpp — launch entry points shared between the per-block C-ABI files and the pipeline.
#pragma once
#include "bin_plan.hpp"
#include "common.hpp"
#include "launch_routes.hpp"

namespace doa {

// K1  (autocorrelate.hip)
// d_gain_outer: optional N*N float2 table w[a + b*N] = g_a conj(g_b) (fused antenna correction), or NULL
// d_workspace: optional piece sums of the read-once path, cov_workspace_bytes(N, K, ovl, n_out) bytes (launch_routes.hpp)
// format / scale: DOA_SAMPLE_FC32 (scale unused) or DOA_SAMPLE_SC16 (widened in registers as __fmul_rn((float)q, scale))
int launch_autocorrelate(int N, int K, int ovl, int avg, int n_out, const void *const *d_in, void *d_out,
                         hipStream_t st, const void *d_gain_outer = nullptr, void *d_workspace = nullptr,
                         int format = DOA_SAMPLE_FC32, float scale = 1.0f);

// ---- multi-batch ("grouped") launches of the lean route: the shapes evd_route and scan_route accept in their group modes -----
// One K1, one EVD and one scan launch each cover a GROUP of up to kMaxGroup batches of `n` items each: item
// g = batch * n + local, 0 <= g < n_batches * n.  The kernels get the group's pointers BY VALUE in their arguments (no
// device-side table); the records between them (coefficients, Chebyshev form) are packed densely by g in one workspace.
// The per-item code is the single-batch kernels' own (the same templates), so results do not depend on the grouping.
// kMaxGroup: profiles/grouped_batches.txt (lab builds carry room for the largest size measured there).
#ifdef DOA_LAB
constexpr int kMaxGroup = 16;
#else
constexpr int kMaxGroup = 8;
#endif
struct BatchGroup {
    int n_batches = 0, n = 0;
    const void *const *in[kMaxGroup];   // batch b: its N input stream pointers (host array of device pointers)
    void *cov[kMaxGroup];               // covariance items of batch b (written by K1, read by the EVD)
    void *spec[kMaxGroup];              // spectrum rows (or P-float scratch rows per item in the angles-only mode)
    void *mx[kMaxGroup], *am[kMaxGroup];
};
// g -> (batch, local) without a division: magic = floor(2^32 / n) under-estimates the quotient by at most one for
// g < 2^32 (g (1/n - magic / 2^32) < g / 2^32 < 1), which one compare corrects
struct GroupSplit {
    unsigned n, magic;
    static GroupSplit make(int n_) { return {(unsigned)n_, (unsigned)((1ull << 32) / (unsigned)n_ - (n_ == 1 ? 1 : 0))}; }
    __device__ __forceinline__ void operator()(unsigned g, unsigned &batch, unsigned &local) const
    {
        unsigned q = __umulhi(g, magic);
        unsigned r = g - q * n;
        if (r >= n) { q++; r -= n; }
        batch = q; local = r;
    }
};
// the pair-load route of K1 (all streams aligned to two samples, even step): a group must be uniform in it, because the
// two routes sum in different orders
bool autocorrelate_pair_loads(int N, int K, int ovl, const void *const *d_in, int format);
int launch_autocorrelate_group(int N, int K, int avg, const BatchGroup &grp, hipStream_t st, const void *d_gain_outer,
                               int format, float scale);
// the one-lane EVD kernel over a group (evd_route's group mode says which shapes)
int launch_music_evd_group(int N, int M, const BatchGroup &grp, void *d_coef_d, void *d_cheb, hipStream_t st);

// Host-built tables of MUSIC_lin_array (music.hip): z_i = exp(j*psi_i), psi_i = k_i * d with
// k_i = float(-2*pi*cos(theta_i)) on the reference's float-accumulated theta grid.
struct MusicTables {
    int N = 0, M = 0, P = 0;
    float norm_spacing = 0.f;
    DevBuf d_z;   // P float2  (float scan)
    DevBuf d_zd;  // P double2 (double scan)
    int build(float norm_spacing, int num_targets, int num_ant_ele, int pspectrum_len);
    void release() { d_z.release(); d_zd.release(); }
};

// The two host steps of that table, shared with WidebandTables below (music.hip).  ula_theta_grid: theta[P], the float
// accumulator of the reference.  ula_phase_row: z_i = (cos psi_i, sin psi_i), psi_i = -2 pi cos(theta_i) d in double, for P
// directions and an element spacing of d wavelengths; zd (doubles) and z (the same values rounded to float), either may be NULL.
void ula_theta_grid(int P, float *theta);
void ula_phase_row(const float *theta, int P, double d, double2 *zd, float2 *z);

// coefficient record per item: [u0, Re u1, Im u1, ..., Re u_{N-1}, Im u_{N-1}, pad] = 2N floats
inline int coef_stride(int N) { return 2 * N; }

// ---- K2+K3: batched Hermitian EVD + noise projector + diagonal sums (music_evd.hip) ---------------------------------------
// The outputs of the eigen stage, every one optional: an entry or a kernel body writes those that are set and that it
// names below, and ignores the others.  Device pointers; set the fields by name.
struct EvdOut {
    float *__restrict__ coef = nullptr;          // float coefficient records, for the float scan
    double *__restrict__ coef_d = nullptr;       // double coefficient records, same layout: the root finder, the double scan
    float2 *__restrict__ pn_out = nullptr;       // diagnostics: P_N itself, N x N float2 per item, column-major
    const float2 *__restrict__ pilot = nullptr;  // calibrate mode: the pilot steering vector, N float2 (read)
    float2 *__restrict__ cal_out = nullptr;      // calibrate mode: the de-rotated top eigenvector, N float2 per item
    // (N <= 4, double) a second record per item, 8 doubles, holding the null spectrum's polynomial in the form the lean scan
    // kernel evaluates, Q = A(c) + s B(c): [a0, a1, a2, a3, b0, b1, b2, 0] (music_scan_impl.hpp, ChebQ) -- the change of
    // basis is per item, so it belongs to the kernel that runs once per item
    double *__restrict__ cheb_d = nullptr;
    double *__restrict__ pn_d = nullptr;         // P_N as a full record (below: launch_music_evd_full), before any rounding
    double *__restrict__ es_rec = nullptr;       // the signal-subspace record (below: launch_music_evd_record)
};
// Cnt of the EVD bodies: EvdFixedM = the launch-uniform num_targets of every existing entry (no code added); EvdCounts = a
// count per item, estimated from the item's eigenvalues (counts_in == nullptr: written to count_out) or supplied by the
// caller (counts_in), plus the optional eigenvalue output.  Double only.
struct EvdFixedM {};
struct EvdCounts {
    const int *counts_in;   // forced mode: M_i per item; nullptr = estimate
    int *count_out;         // estimate mode: int32 per item
    float *eig_out;         // optional: N floats per item, ascending, true scale
    int K, method, kmax;    // num_snapshots, DOA_SOURCE_COUNT_MDL / _AIC, largest count considered
};
inline EvdCounts evd_counts_forced(const int *counts_in) { return {counts_in, nullptr, nullptr, 0, 0, 0}; }
inline EvdCounts evd_counts_estimate(int *count_out, float *eig_out, int K, int method, int kmax)
{
    return {nullptr, count_out, eig_out, K, method, kmax};
}
// Uses out.coef, coef_d, pn_out and cheb_d (N <= 4, evd_bits == 64).
int launch_music_evd(int N, int M, int n_items, const void *d_R, const EvdOut &out, int evd_bits, hipStream_t st);
// The same stage with a count PER ITEM (double, always the Jacobi forms: one lane per item for N <= 4, 8 lanes for N <= 8,
// one wave for N <= 16).  Estimate mode (evd_counts_estimate): the count comes from the item's eigenvalues (jacobi.hpp:
// source_count_from_eigenvalues; K snapshots, method DOA_SOURCE_COUNT_*, counts 0..kmax) and is written to count_out.
// Forced mode (evd_counts_forced): the count is read from counts_in.  eig_out (optional): at the item's scale.
// Uses out.coef_d, cheb_d (N <= 4) and es_rec; with none of them: count / eigenvalues only.  Count 0: the record of
// P_N = I; a count outside 0..N-1: a NaN record.  With es_rec the launch is the group form at every N (4 lanes per item
// for N <= 4: the form that holds the eigenvectors by rows).
int launch_music_evd_counts(int N, int n_items, const void *d_R, const EvdCounts &cnt, const EvdOut &out, hipStream_t st);
// ---- ESPRIT (esprit.hip; definition in include/doa_hip.h) -----------------------------------------------------------------
// SIGNAL-SUBSPACE RECORD of an item: all N eigenvectors of H as columns ordered by DESCENDING eigenvalue (the eig_sym
// ranking reversed), 2 N^2 doubles: [2 (k N + row)] = Re V[row][k], [2 (k N + row) + 1] = Im V[row][k].  A consumer takes
// the first M columns, whatever M is for that item.  A non-finite item's record is UNSPECIFIED (its eigenvalues do not rank, so
// columns may stay unwritten): a consumer decides from the item itself, as esprit_kernel does for status 1.
__host__ __device__ inline size_t subspace_record_len(int N) { return (size_t)2 * N * N; }
// The eigen stage writing the record only (always the double Jacobi forms: 4 lanes per item for N <= 4, 8 lanes for N <= 8,
// one wave for N <= 16).  The record does not depend on a source count.
int launch_music_evd_record(int N, int n_items, const void *d_R, void *d_rec, hipStream_t st);
// esprit_kernel: W floats per item from the first m columns of its record; d_R (the items the record came from) supplies
// the trace test.  d_counts == NULL: m = W for every item.  Otherwise m_i = d_counts[i] (int32): 1 <= m_i <= min(W, N-1):
// the first m_i slots as the fixed launch writes them for W = m_i, the others NaN; 0: all NaN, status 0; else all NaN,
// status 2.  d_status (optional): int32 per item, 0 ok / 1 not solvable / 2 no usable count / 3 iteration cap.
int launch_esprit(int N, int W, float norm_spacing, int n_items, const void *d_R, const void *d_rec, const void *d_counts,
                  void *d_out, void *d_status, hipStream_t st);
// after the scan of a per-item-count call: rows (P floats) of items whose count is outside 0..N-1 become NaN (the scan kernels
// themselves write 0.0 dB for a NaN record)
int launch_music_invalid_rows(int N, int P, int n_items, const void *d_counts, void *d_spec, hipStream_t st);
// spatial smoothing (spatial_smooth.hip; definition in include/doa_hip.h): n_items column-major N x N items (upper triangle
// read) -> S x S items, full Hermitian.  fb: 0 forward, 1 forward-backward.  d_Rs must not overlap d_R (not checked).
// 16-byte loads and stores when both pointers are 16-byte aligned, 8-byte ones otherwise: the same bits either way.
int launch_spatial_smooth(int N, int S, int fb, int n_items, const void *d_R, void *d_Rs, hipStream_t st);
constexpr int kChebRecord = 8;      // doubles per item
// Q(psi) = u0 + 2 sum_l (x_l cos(l psi) - y_l sin(l psi)), u_l = x_l + j y_l, in powers of c = cos psi and s = sin psi
// (cos 2x = 2c^2 - 1, cos 3x = 4c^3 - 3c, sin 2x = 2sc, sin 3x = s(4c^2 - 1)):  Q = A(c) + s B(c),
// A = (u0 - 2x2) + (2x1 - 6x3) c + 4x2 c^2 + 8x3 c^3,  B = (2y3 - 2y1) - 4y2 c - 8y3 c^2   (music_scan_impl.hpp: ChebQ)
// ux[l], uy[l]: u_l for l = 0..3 (zero beyond the array size)
__device__ __forceinline__ void write_cheb_record(double *__restrict__ o, const double (&ux)[4], const double (&uy)[4])
{
    o[0] = ux[0] - 2 * ux[2]; o[1] = 2 * ux[1] - 6 * ux[3]; o[2] = 4 * ux[2]; o[3] = 8 * ux[3];
    o[4] = 2 * uy[3] - 2 * uy[1]; o[5] = -4 * uy[2]; o[6] = -8 * uy[3]; o[7] = 0.0;
}
// entry l of an item's coefficient records (above: coef_stride), u_l = tr + j ti; l = 0 also writes the pad.  co (float
// record) and cd (double record): the item's own, either may be NULL
template <typename T> __device__ __forceinline__ void store_coef_entry(float *co, double *cd, int N, int l, T tr, T ti)
{
    if (l == 0) {
        if (co) { co[0] = (float)tr; co[2 * N - 1] = 0.f; }
        if (cd) { cd[0] = (double)tr; cd[2 * N - 1] = 0.0; }
    } else {
        if (co) { co[2 * l - 1] = (float)tr; co[2 * l] = (float)ti; }
        if (cd) { cd[2 * l - 1] = (double)tr; cd[2 * l] = (double)ti; }
    }
}
// Capon (capon.hip; definition in include/doa_hip.h): the records of W = (H / mu + loading I)^-1 per item, in place of the
// eigen stage's.  Its outputs, in the style of EvdOut (device pointers; set the fields by name).  An item that is not positive
// definite enough, or not finite, has status 1 and NaN in every record.
struct CaponOut {
    double *coef_d = nullptr;   // u_l = sum_r W[r+l, r] as a double coefficient record: required unless `full` is set
    double *cheb_d = nullptr;   // N <= 4: the Chebyshev record, required wherever coef_d is
    float2 *w_out = nullptr;    // diagnostics: W as N x N float2, column-major
    double *full = nullptr;     // W as a full record for launch_array_scan (below), from the same double values as w_out
    int *status = nullptr;      // int32 per item: 0 ok / 1
};
int launch_capon_inverse(int N, int n_items, const void *d_R, double loading, const CaponOut &out, hipStream_t st);
// after scan and peak pick of a Capon call: for items with status != 0 the spectrum row (P floats; d_spec may be NULL) and the
// M peak values / locations (d_max / d_argmax may be NULL) become NaN (the scan kernels write 0.0 dB for a NaN record)
int launch_capon_invalid_rows(int P, int M, int n_items, const void *d_status, void *d_spec, void *d_max, void *d_argmax,
                              hipStream_t st);
// IAA (iaa.hip; definition in include/doa_hip.h): the whole estimator of n_items covariance items in one launch, one wave per
// item.  d_zd: the P double2 phases of a MusicTables.  Its outputs (device pointers; only spec is required):
struct IaaOut {
    float *spec = nullptr;      // P floats per item: dB against the row maximum
    float *power = nullptr;     // P floats per item: mu p_k, in the units of the covariance item
    int *status = nullptr;      // int32 per item: 0 ok / 1 (both rows NaN)
    double *p_dbg = nullptr;    // diagnostics: the final p_k in double, P per item
    double *lag_dbg = nullptr;  // diagnostics: the lags r_l of the last iteration's R, N (re, im) pairs per item
};
int launch_iaa(int N, int P, int iterations, double loading, int n_items, const void *d_R, const void *d_zd, const IaaOut &out,
               hipStream_t st);
// ---- arbitrary array geometry (array_scan.hip; definition in include/doa_hip.h) -------------------------------------------
// FULL RECORD of a Hermitian N x N matrix X: N^2 doubles per item, X packed into a real square (column-major index
// r + c N):   [r + r N] = X[r][r];   for r < c:  [r + c N] = Re X[r][c],  [c + r N] = Im X[r][c].
// With the table T built from the steering rows in the same order (ArrayTable), a^H X a = sum_k record[k] T[k]: a real dot
// product of length N^2.
inline int full_record_len(int N) { return N * N; }
// The eigen stage writing the full record of P_N (always the double Jacobi forms: 4 lanes per item for N <= 4, 8 lanes for
// N <= 8, one wave for N <= 16; the subspace iterations never form P_N outside their diagnostics).  d_pn (optional): P_N as
// float2, as launch_music_evd writes it.
int launch_music_evd_full(int N, int M, int n_items, const void *d_R, void *d_full, void *d_pn, hipStream_t st);
// The steering table of a handle in the scan's form: T[k][i], k over the full record's N^2 components, i over the P
// directions (doubles, row k contiguous in i):  |a_r|^2 on the diagonal components, 2 Re(conj(a_r) a_c) against Re X[r][c]
// and -2 Im(conj(a_r) a_c) against Im X[r][c].
struct ArrayTable {
    int N = 0, P = 0;
    DevBuf d_t;   // N^2 x P doubles
    // steering: HOST pointer, P rows of N complex doubles (a_i[n] at [2 (i N + n)], re then im)
    int build(int num_ant_ele, int pspectrum_len, const double *steering);
    void release() { d_t.release(); }
};
// validation shared by the create entries and doa_music_pipeline_set_steering_table: every entry finite
bool steering_table_finite(const double *steering, int N, int P);
// the table checks of every create that takes one (who: for the message): DOA_OK, or DOA_ERR_INVALID_ARG with the error set
int steering_table_args(const char *who, int num_ant_ele, int pspectrum_len, const double *steering);
// Q_i = sum_k record[k] T[k][i] in double, q = (float) Q, out = 1 / q, dB against the row maximum with the scan kernels' own
// normalisation (music_scan_impl.hpp: LeanNorm / db_from_ratio).  d_q (optional): q, P floats per item.
int launch_array_scan(const ArrayTable &t, int n_items, const void *d_full, void *d_spec, void *d_q, hipStream_t st);
// ---- incoherent wideband MUSIC (wideband_music.hip; definition in include/doa_hip.h) --------------------------------------
// The phase table of a handle: Z[j][p] = (cos psi, sin psi), psi = -2 pi cos(theta_p) d_f at the spacing d_f
// (bin_plan.hpp: wideband_bin_spacing) of bin sel.bin(j): sel.nb rows of P double2, each row by ula_phase_row on
// ula_theta_grid (a row at rate_over_carrier = 0 is MusicTables::d_zd).
struct WidebandTables {
    int N = 0, M = 0, P = 0, combine = 0;
    BinSelection sel;
    DevBuf d_z;   // sel.nb x P double2
    int build(float norm_spacing, int num_targets, int num_ant_ele, int pspectrum_len, const BinSelection &sel,
              double rate_over_carrier, int combine);
    void release() { d_z.release(); }
};
// One workgroup per snapshot: the double coefficient records of its num_bins items (d_coef, item i num_bins + j, coef_stride(N)
// doubles each) -> Q_ij by the double scan's Horner chain at row j of the table, combined over the used bins in item order
// by t.combine (DOA_WIDEBAND_*), q = (float) Q_i, dB against the row maximum with the scan kernels' own normalisation.
// d_weights (optional): n x num_bins floats, NULL = all ones.  d_counts (optional): n x num_bins int32, the counts the records
// were made with; NULL = every record is for t.M sources.  A bin is used if bin_weight_used(w) and (with counts) 1 <= c <=
// N - 1; a usable weight with c == 0 skips the bin, with any other c the snapshot has status 2.  d_q (optional): q, P floats
// per snapshot.  d_status (optional): int32 per snapshot, 0 ok / 1 no bin used / 2 bad count / 3 a used record not finite; a
// status other than 0 gives NaN rows (d_spec and d_q).  The records of unused bins are not read.
int launch_wideband_scan(const WidebandTables &t, int n_snapshots, const void *d_coef, const void *d_weights, const void *d_counts,
                         void *d_spec, void *d_q, void *d_status, hipStream_t st);
// ---- coherent focusing (focus_covariance.hip; definition in include/doa_hip.h) --------------------------------------------
// The focusing table of a handle: num_bins matrices of N x N double2, row-major per matrix (T_j[a][b] at (j N + a) N + b).
struct FocusTables {
    int N = 0, num_bins = 0;
    DevBuf d_t;
    // matrices: HOST pointer, num_bins N N complex doubles in that layout
    int build(int num_ant_ele, int num_bins, const double *matrices);
    void release() { d_t.release(); }
};
// One wave per snapshot: out_i = sum_j w_ij T_j H(R_ij) T_j^H / sum_j w_ij over the used bins (bin_weight_used), in double,
// rounded once.  d_items: n x num_bins column-major N x N float2 items (8-byte aligned); d_weights (optional): n x num_bins
// floats, NULL = all ones; d_out: n items, exactly Hermitian, must not overlap d_items (not checked); d_status (optional):
// int32 per snapshot, 0 ok / 1 no bin used / 3 a used item not finite; a status other than 0 gives an all-NaN item.
int launch_focus_covariance(const FocusTables &t, int n_snapshots, const void *d_items, const void *d_weights, void *d_out,
                            void *d_status, hipStream_t st);
// ---- difference co-array (coarray_covariance.hip; definition in include/doa_hip.h) ----------------------------------------
// The pair list of a layout, built once on the host: for every lag l < Lv the entries of the item's upper triangle that
// make up s[l], in the definition's order.  pair[k] = (row + col N) of the entry read, | kCoarrayConj if H[a,b] is its
// conjugate (a > b); the pairs of lag l are pair[start[l] .. start[l+1]).  At most N (N - 1) / 2 + N = 136 entries.
constexpr int kCoarrayMaxPairs = DOA_MAX_ANT_ELE * (DOA_MAX_ANT_ELE + 1) / 2;
constexpr unsigned short kCoarrayConj = 0x8000;
struct CoarrayTables {
    int N = 0, Lv = 0, mode = 0;
    // device: [0 .. kCoarrayMaxPairs) the pairs, then start[0 .. DOA_MAX_ANT_ELE], all unsigned short
    DevBuf d_pairs;
    // positions: N distinct integers (validated by the caller); Lv <= the contiguous size
    int build(const int *positions, int num_ant_ele, int virtual_size, int mode);
    void release() { d_pairs.release(); }
};
// n_items column-major N x N items (upper triangle read) -> Lv x Lv items, exactly Hermitian.  d_out must not overlap d_R (not
// checked).  16-byte loads and stores when both pointers are 16-byte aligned, 8-byte ones otherwise: the same bits either way.
int launch_coarray_covariance(const CoarrayTables &t, int n_items, const void *d_R, void *d_out, hipStream_t st);
// diagnostics: items that left the signal-subspace fast path of K2+K3 for the Jacobi fall-back since the last reset
long long evd_fallback_count(bool reset);
// the calling thread's current device's counter (allocated on first use; nullptr if that fails) and, for the tests, the device
// an allocation lives on
unsigned long long *evd_fallback_counter();
int evd_fallback_counter_device(const void *p);
// calibrate_lin_array (calibrate.hip): d_pilot = N float2 (pilot steering vector), d_out = n_items*N float2
int launch_calibrate(int N, int n_items, const void *d_R, const void *d_pilot, void *d_out, int bits, hipStream_t st);
// K4: spectrum scan in float (bits == 32, float coefficient records) or double (bits == 64, double
// records).  d_q (un-normalised null spectrum, P floats per item) may be NULL.
// With `peaks` (+ d_max/d_argmax) the find_local_max step is fused into the scan when the fast path
// applies; *peaks_done tells the caller whether it still has to launch K5 itself.
struct PeakTables;
int launch_music_scan(const MusicTables &t, int bits, int n_items, const void *d_coef, void *d_spec, void *d_q,
                      hipStream_t st, const PeakTables *peaks = nullptr, void *d_max = nullptr,
                      void *d_argmax = nullptr, bool *peaks_done = nullptr, bool store_spectrum = true,
                      const void *d_cheb = nullptr);
// the lean scan + peak pick over a group (scan_route's group mode says which shapes; peaks->L == t.P, every grp.spec 16-byte aligned);
// d_cheb: the group's records, dense by g.  store_spectrum = false: grp.spec are scratch rows (angles only)
int launch_music_scan_group(const MusicTables &t, const PeakTables &peaks, const BatchGroup &grp, const void *d_cheb,
                            bool store_spectrum, hipStream_t st);

// K5 (find_local_max.hip)
struct PeakTables {
    int M = 0, L = 0;
    float x_min = 0.f, x_max = 0.f;
    DevBuf d_x;  // L floats, float-accumulated x axis
    int build(int num_max_vals, int vector_len, float x_min, float x_max);
    void release() { d_x.release(); }
};
int launch_find_local_max(const PeakTables &t, int n_items, const void *d_in, void *d_max, void *d_argmax,
                          hipStream_t st);
// with a count per item (d_counts: int32 m_i): the first m_i slots as find_local_max(m_i, ...) writes them, items stay t.M
// floats wide, the other slots NaN; m_i outside 0..t.M: all NaN.  Every route of launch_find_local_max; L > 4096: the
// serial kernel (d_scratch: L bytes per item).
int launch_find_local_max_counts(const PeakTables &t, int n_items, const void *d_in, const void *d_counts, void *d_max,
                                 void *d_argmax, hipStream_t st);
// K5 on whichever route takes the vector length (d_counts: optional, as above): the parallel kernels for L <= 4096, else the
// serial kernel, for which `scratch` is grown to L bytes for each of `reserve_items` items and used from item `item_off` on
int launch_peak_pick(const PeakTables &t, int n_items, const void *d_in, const void *d_counts, void *d_max, void *d_argmax,
                     DevBuf &scratch, size_t reserve_items, size_t item_off, hipStream_t st);

// find_local_max_2d (find_local_max_2d.hip; the rule: include/doa_hip.h)
constexpr int kPeaks2dMaxCells = 1 << 24;
struct Peaks2dTables {
    int M = 0, n_az = 0, n_el = 0, wrap = 0;
    DevBuf d_az, d_el;   // n_az / n_el floats, each formed in double
    int build(int num_max_vals, int n_az, int n_el, float az_min, float az_max, float el_min, float el_max, int wrap_az);
    int cells() const { return n_az * n_el; }
};
// the argument checks of every entry that takes a grid (who: for the message); false with the error set
bool peaks2d_args_ok(const char *who, int num_max_vals, int n_az, int n_el, double az_min, double az_max, double el_min,
                     double el_max);
// d_val, d_az, d_el: t.M floats per item each.  stride_az_el > t.M, grids above 16384 cells (the global form) only: item i's
// azimuths and elevations start stride_az_el floats after item i - 1's (the pipeline's grid mode keeps both in one [n][2 M]
// buffer, and needs this launch only for such grids)
int launch_find_local_max_2d(const Peaks2dTables &t, int n_items, const void *d_in, void *d_val, void *d_az, void *d_el,
                             hipStream_t st, int stride_az_el = 0);
// The steering-table scan with find_local_max_2d's pick on its LDS row (array_scan.hip): per item the spectrum row (stored
// only if d_spec is given) and the 3 t.M outputs are bit for bit those of launch_array_scan followed by
// launch_find_local_max_2d on the same full records.  pk.cells() == t.P.  Grids of up to kArrayGridFusedMax cells are one
// launch and write no row without d_spec; larger ones are the two launches named, and need d_spec (the caller's scratch).
constexpr int kArrayGridFusedMax = 16384;
int launch_array_scan_peaks2d(const ArrayTable &t, const Peaks2dTables &pk, int n_items, const void *d_full, void *d_spec,
                              void *d_val, void *d_az, void *d_el, int stride_az_el, hipStream_t st);

// K6 (root_music.hip): polynomial roots from the DOUBLE coefficient records -> angles.
// d_roots (optional, diagnostics): the 2N-2 roots found per item as double2, in the kernel's lane order.
int launch_root_music(int N, int M, float norm_spacing, int n_items, const void *d_coef, void *d_out,
                      void *d_status, hipStream_t st, void *d_roots = nullptr);
// with a count per item (d_counts: int32 m_i; root_music.hip, RootCounts): items stay W floats wide.  1 <= m_i <= min(W, N-1):
// the first m_i slots as launch_root_music writes them for M = m_i, the others NaN, status 0 / 1; m_i == 0: all NaN, status 0,
// the record is not read; any other value: all NaN, status 2.
int launch_root_music_counts(int N, int W, float norm_spacing, int n_items, const void *d_coef, const void *d_counts, void *d_out,
                             void *d_status, hipStream_t st, void *d_roots = nullptr);
// the selection stage of K6 alone, on caller-supplied roots (n_items x (2N-2) double2): diagnostics
int launch_root_select(int N, int M, float norm_spacing, int n_items, const void *d_roots, void *d_out, void *d_status,
                       hipStream_t st);
int launch_root_select_counts(int N, int W, float norm_spacing, int n_items, const void *d_roots, const void *d_counts,
                              void *d_out, void *d_status, hipStream_t st);

}  // namespace doa
