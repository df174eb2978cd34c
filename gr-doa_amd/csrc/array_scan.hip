// array_scan.hip — spectra for an ARBITRARY array geometry on gfx950: the steering-table scan kernel, the host-built table,
// doa_planar_steering_table.  The C ABI of doa_MUSIC_array / doa_capon_array is in spectrum_blocks.hip.  Not blocks of the
// reference; the definition is stated once in include/doa_hip.h.
//
// The ULA scans (music_scan_impl.hpp) never see a matrix, only its 2N-1 diagonal sums, which summarise a^H X a only for
// a_n = z^n.  Here the stage in front (the Jacobi forms of the eigen stage, the Capon inverse) writes the FULL RECORD of its
// Hermitian matrix X (kernels.hpp: N^2 doubles, X packed into a real square) and the handle carries a table T[k][i] built
// once from the steering rows, so that
//     Q_i = Re(a_i^H X a_i) = sum_k record[k] T[k][i]                       (k over N^2 real components, i over P directions):
// a batch is an [items x N^2] . [N^2 x P] real product, then a reciprocal, a maximum and a logarithm per row.
//
// Structure: "wave over angles".  A workgroup of 256 threads owns IT items and every direction: thread t takes the
// directions t + 256 m.  The table row k is loaded coalesced, once per thread, and used for all IT items; the records are
// workgroup-uniform, so record[k] travels through scalar loads and reaches the FMA as a scalar operand.  q = (float) Q is
// parked in LDS (IT rows of P floats) until the row minimum is known; the second pass turns the row into dB with the
// normalisation of the ULA scans (LeanNorm / db_from_ratio) and writes it to memory ONCE.  The sum over k runs in index
// order for every direction of every item, whatever IT, the batch size or the item's neighbours are.
//   P <= 1024   8 items per workgroup, 2 directions per thread and step     (32 KiB of LDS)
//   P <= 4096   4 items, 4 directions                                        (64 KiB)
//   P <= 16384  1 item, 4 directions                                         (64 KiB)
//   longer      4 items, 4 directions, no row in LDS: the second pass forms Q again (the same sum, the same bits)
// array_scan_peaks2d_kernel (music_pipeline's grid mode) is the same body with find_local_max_2d's pick on the LDS row behind
// it: the second pass leaves the dB row in LDS, stores it only for a caller that wants it, and the top M local maxima of the
// azimuth x elevation grid go straight to the outputs (array_scan_body below).  Its forms: 8 items for P <= 1024, 4 items
// with 2 directions per thread for P <= 2048 (32 KiB: four workgroups per CU where the 64 KiB form has two), 4 items for
// P <= 4096, 1 item for P <= 16384; longer rows are the two launches (launch_array_scan_peaks2d).
// The matrix instruction v_mfma_f64_16x16x4_f64 (items as M, directions as N) was the alternative: it needs the records
// transposed into its operand layout and pays for 16 items per tile whatever the batch; at N = 4 the kernel is bound by
// the store of the spectrum either way, so the plain form came first.
#include "kernels.hpp"
#include "music_scan_impl.hpp"
#include "peak_device.hpp"

#include <cmath>
#include <vector>

namespace doa {
namespace {

constexpr int kScanThreads = 256;
static_assert(kScanThreads == kPeaks2dThreads, "block_argbest joins four waves");

// what the form that ends in the two-dimensional pick takes besides the scan's arguments
struct PickArgs {
    Grid2d g;
    Peaks2dOut out;
};

// PICK = false: array_scan_kernel.  PICK = true (rows in LDS only): array_scan_peaks2d_kernel -- pass 2 turns the LDS row into
// dB IN PLACE (and stores it only if `spec` is given), then find_local_max_2d's rule runs on that row.  The test runs on the dB
// values, not on Q: distinct Q can round to one dB value, and the plateau rule is defined on what the second block of the
// chain reads.  IT > 1 (P <= 4096, at most 64 flag words): one WAVE per item, flag word k in lane k, the rounds are wave
// arg-maxima: no barrier after the one that ends pass 2.  IT == 1: the workgroup form of find_local_max_2d_kernel.
template <int IT, int A, int PMAX, bool PICK>
__device__ __forceinline__ void array_scan_body(const double *__restrict__ full, const double *__restrict__ tab, float *__restrict__ spec,
                                                float *__restrict__ qout, int P, int NN, int n_items, const PickArgs *pk)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "array_scan_kernel keeps up to 64 KiB of rows plus its reduction slots in LDS: gfx950 (MI355X) only"
#endif
    constexpr bool ROWS = PMAX > 0;
    static_assert(!PICK || (ROWS && (IT == 1 ? PMAX <= 64 * kScanThreads : PMAX <= 64 * kWave)), "one flag word per thread / lane");
    __shared__ float rows[ROWS ? IT * PMAX : 1];           // item it, direction p at [it * P + p]
    __shared__ float red[2][kScanThreads / kWave][IT];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wib = tid / kWave;
    const int item0 = blockIdx.x * IT;
    const double *x[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) x[it] = full + (size_t)min(item0 + it, n_items - 1) * NN;   // idle slots shadow the last item
    // Q at one direction: the sum in index order (the second pass of the row-less form)
    auto q_at = [&](int it, int p) -> float {
        double acc = 0.0;
        for (int k = 0; k < NN; k++) acc = fma(x[it][k], tab[(size_t)k * P + p], acc);
        return (float)acc;
    };
    float mn[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) mn[it] = INFINITY;
    // pass 1: Q, its float image into the LDS row, the row minimum
    for (int p0 = 0; p0 < P; p0 += kScanThreads * A) {
        int pa[A];
#pragma unroll
        for (int a = 0; a < A; a++) pa[a] = min(p0 + a * kScanThreads + tid, P - 1);      // clamped: every load is in the table
        double acc[IT][A];
#pragma unroll
        for (int it = 0; it < IT; it++)
#pragma unroll
            for (int a = 0; a < A; a++) acc[it][a] = 0.0;
        const double *trow = tab;
#pragma unroll 2
        for (int k = 0; k < NN; k++, trow += P) {
            double t[A];
#pragma unroll
            for (int a = 0; a < A; a++) t[a] = trow[pa[a]];
#pragma unroll
            for (int it = 0; it < IT; it++) {
                const double xv = x[it][k];
#pragma unroll
                for (int a = 0; a < A; a++) acc[it][a] = fma(xv, t[a], acc[it][a]);
            }
        }
#pragma unroll
        for (int a = 0; a < A; a++) {
            const int p = p0 + a * kScanThreads + tid;
            if (p < P) {
#pragma unroll
                for (int it = 0; it < IT; it++) {
                    const float q = (float)acc[it][a];
                    mn[it] = fminf(mn[it], q);
                    if constexpr (ROWS) rows[it * P + p] = q;
                    if (qout && item0 + it < n_items) qout[(size_t)(item0 + it) * P + p] = q;
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const float m = wave_allreduce_min(mn[it]);
        if (lane == 0) red[0][wib][it] = m;
    }
    __syncthreads();                                        // the rows and the wave minima are in LDS
    // pass 2: dB, one write of the row.  Every branch below is workgroup-uniform (mn, the item index).
#pragma unroll
    for (int it = 0; it < IT; it++) {
        if (item0 + it >= n_items) break;
        const float m = fminf(fminf(red[0][0][it], red[0][1][it]), fminf(red[0][2][it], red[0][3][it]));
        float *grow = spec + (size_t)(item0 + it) * P;
        auto q_of = [&](int p) -> float {
            if constexpr (ROWS) return rows[it * P + p];
            else return q_at(it, p);
        };
        // PICK: the thread that read q at p is the one that overwrites it, so the row changes in place without a barrier
        auto put = [&](int p, float db) {
            if constexpr (PICK) {
                rows[it * P + p] = db;
                if (spec) __builtin_nontemporal_store(db, grow + p);
            } else {
                __builtin_nontemporal_store(db, grow + p);
            }
        };
        if (lean_norm_ok(m)) {
            const LeanNorm nrm(m);
            for (int p = tid; p < P; p += kScanThreads) {
                bool tie;
                put(p, nrm.db(q_of(p), tie));
            }
        } else {
            // rows whose minimum of Q is not a positive normal number: the general semantics (db_from_ratio)
            float mx = -INFINITY;
            for (int p = tid; p < P; p += kScanThreads) mx = fmaxf(mx, 1.0f / q_of(p));
            mx = wave_allreduce_max(mx);
            if (lane == 0) red[1][wib][it] = mx;
            __syncthreads();
            mx = fmaxf(fmaxf(red[1][0][it], red[1][1][it]), fmaxf(red[1][2][it], red[1][3][it]));
            const float inv_mx = __builtin_amdgcn_rcpf(mx);
            for (int p = tid; p < P; p += kScanThreads) put(p, db_from_ratio(1.0f / q_of(p), mx, inv_mx));
        }
    }
    if constexpr (PICK) {
        __syncthreads();                                    // every row is dB
        const Grid2d &g = pk->g;
        if constexpr (IT > 1) {
            for (int it = wib; it < IT; it += kScanThreads / kWave) {
                if (item0 + it >= n_items) break;           // wave-uniform: idle slots store nothing
                const float *row = rows + it * P;
                const auto lds = [&](int j) { return row[j]; };
                unsigned long long mine = 0ull;             // lane k: the flags of cells 64 k .. 64 k + 63
                for (int base = 0; base < P; base += kWave) {
                    const int i = base + lane;
                    const bool peak = (i < P) && is_peak<false>(lds, g, i, row[i < P ? i : 0]);
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(peak);
                    if (lane == (base >> 6)) mine = m;
                }
                peaks2d_rounds(g, pk->out, (size_t)(item0 + it), lane,
                               [&](bool first, float pv, int pi, float &bv, int &bi) { flagged_best(row, mine, lane, first, pv, pi, bv, bi); },
                               [](float &v, int &i, int) { wave_argbest(v, i); });
            }
        } else {
            __shared__ unsigned long long flags[PMAX / 64];
            __shared__ float sv[2][4];
            __shared__ int si[2][4];
            const auto lds = [&](int j) { return rows[j]; };
            for (int base = tid - lane; base < P; base += kScanThreads) {      // wave-uniform: 64 consecutive cells per step
                const int i = base + lane;
                const bool peak = (i < P) && is_peak<false>(lds, g, i, rows[i < P ? i : 0]);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(peak);
                if (lane == 0) flags[base >> 6] = m;
            }
            __syncthreads();
            const unsigned long long mine = (64 * tid < P) ? flags[tid] : 0ull;
            peaks2d_rounds(g, pk->out, (size_t)item0, tid,
                           [&](bool first, float pv, int pi, float &bv, int &bi) { flagged_best(rows, mine, tid, first, pv, pi, bv, bi); },
                           [&](float &v, int &i, int r) { block_argbest(v, i, sv, si, r); });
        }
    }
}

template <int IT, int A, int PMAX>
__global__ __launch_bounds__(kScanThreads) void array_scan_kernel(const double *__restrict__ full, const double *__restrict__ tab,
                                                                  float *__restrict__ spec, float *__restrict__ qout, int P, int NN,
                                                                  int n_items)
{
    array_scan_body<IT, A, PMAX, false>(full, tab, spec, qout, P, NN, n_items, nullptr);
}

template <int IT, int A, int PMAX>
__global__ __launch_bounds__(kScanThreads) void array_scan_peaks2d_kernel(const double *__restrict__ full, const double *__restrict__ tab,
                                                                          float *__restrict__ spec, int P, int NN, int n_items, PickArgs pk)
{
    array_scan_body<IT, A, PMAX, true>(full, tab, spec, nullptr, P, NN, n_items, &pk);
}

template <int IT, int A, int PMAX>
void launch_array_scan_form(const ArrayTable &t, int n_items, const void *d_full, void *d_spec, void *d_q, hipStream_t st)
{
    hipLaunchKernelGGL((array_scan_kernel<IT, A, PMAX>), dim3((n_items + IT - 1) / IT), dim3(kScanThreads), 0, st,
                       (const double *)d_full, t.d_t.as<double>(), (float *)d_spec, (float *)d_q, t.P, t.N * t.N, n_items);
}

template <int IT, int A, int PMAX>
void launch_array_grid_form(const ArrayTable &t, int n_items, const void *d_full, void *d_spec, const PickArgs &pk, hipStream_t st)
{
    hipLaunchKernelGGL((array_scan_peaks2d_kernel<IT, A, PMAX>), dim3((n_items + IT - 1) / IT), dim3(kScanThreads), 0, st,
                       (const double *)d_full, t.d_t.as<double>(), (float *)d_spec, t.P, t.N * t.N, n_items, pk);
}

}  // namespace

bool steering_table_finite(const double *steering, int N, int P)
{
    if (!steering) return false;
    const size_t n = 2 * (size_t)N * (size_t)P;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(steering[i])) return false;
    return true;
}

int ArrayTable::build(int num_ant_ele, int pspectrum_len, const double *steering)
{
    N = num_ant_ele; P = pspectrum_len;
    const size_t NN = (size_t)N * N;
    std::vector<double> T(NN * (size_t)P);
    for (int i = 0; i < P; i++) {
        const double *a = steering + 2 * (size_t)i * N;
        for (int c = 0; c < N; c++) {
            const double cr = a[2 * c], ci = a[2 * c + 1];
            T[((size_t)c + (size_t)c * N) * P + i] = cr * cr + ci * ci;
            for (int r = 0; r < c; r++) {
                const double rr = a[2 * r], ri = a[2 * r + 1];
                // w = conj(a_r) a_c:  conj(a_r) X[r][c] a_c + its conjugate = 2 (Re X Re w - Im X Im w)
                const double wr = rr * cr + ri * ci, wi = rr * ci - ri * cr;
                T[((size_t)r + (size_t)c * N) * P + i] = 2.0 * wr;
                T[((size_t)c + (size_t)r * N) * P + i] = -2.0 * wi;
            }
        }
    }
    const size_t bytes = T.size() * sizeof(double);
    if (int rc = d_t.reserve(bytes); rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_t.p, T.data(), bytes, hipMemcpyHostToDevice));
    return DOA_OK;
}

int launch_array_scan(const ArrayTable &t, int n_items, const void *d_full, void *d_spec, void *d_q, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    if (t.N < 2 || t.N > DOA_MAX_ANT_ELE || t.P < 1 || !t.d_t.p || !d_full || !d_spec) {
        set_error("array scan: bad arguments (N=%d, P=%d)", t.N, t.P);
        return DOA_ERR_INVALID_ARG;
    }
    if (t.P <= 1024) launch_array_scan_form<8, 2, 1024>(t, n_items, d_full, d_spec, d_q, st);
    else if (t.P <= 4096) launch_array_scan_form<4, 4, 4096>(t, n_items, d_full, d_spec, d_q, st);
    else if (t.P <= 16384) launch_array_scan_form<1, 4, 16384>(t, n_items, d_full, d_spec, d_q, st);
    else launch_array_scan_form<4, 4, 0>(t, n_items, d_full, d_spec, d_q, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

int launch_array_scan_peaks2d(const ArrayTable &t, const Peaks2dTables &pk, int n_items, const void *d_full, void *d_spec,
                              void *d_val, void *d_az, void *d_el, int stride_az_el, hipStream_t st)
{
    if (n_items <= 0) return DOA_OK;
    if (t.N < 2 || t.N > DOA_MAX_ANT_ELE || t.P < 1 || !t.d_t.p || pk.M < 1 || pk.M > DOA_MAX_PEAKS || pk.n_az < 1 || pk.n_el < 1 ||
        (long long)pk.n_az * pk.n_el != t.P || t.P > kPeaks2dMaxCells || stride_az_el < pk.M || !pk.d_az.p || !pk.d_el.p || !d_full ||
        !d_val || !d_az || !d_el || (t.P > kArrayGridFusedMax && !d_spec)) {
        set_error("array scan with the two-dimensional pick: bad arguments (N=%d, P=%d, grid %d x %d, M=%d, stride %d)", t.N, t.P,
                  pk.n_az, pk.n_el, pk.M, stride_az_el);
        return DOA_ERR_INVALID_ARG;
    }
    if (t.P > kArrayGridFusedMax) {
        // no row of this length fits in LDS: the scan's row-less form, then the pick's global form
        if (int rc = launch_array_scan(t, n_items, d_full, d_spec, nullptr, st); rc != DOA_OK) return rc;
        return launch_find_local_max_2d(pk, n_items, d_spec, d_val, d_az, d_el, st, stride_az_el);
    }
    const PickArgs a{make_grid2d(pk.n_az, pk.n_el, pk.wrap),
                     {pk.d_az.as<float>(), pk.d_el.as<float>(), (float *)d_val, (float *)d_az, (float *)d_el, pk.M, stride_az_el}};
    if (t.P <= 1024) launch_array_grid_form<8, 2, 1024>(t, n_items, d_full, d_spec, a, st);
    else if (t.P <= 2048) launch_array_grid_form<4, 2, 2048>(t, n_items, d_full, d_spec, a, st);
    else if (t.P <= 4096) launch_array_grid_form<4, 4, 4096>(t, n_items, d_full, d_spec, a, st);
    else launch_array_grid_form<1, 4, 16384>(t, n_items, d_full, d_spec, a, st);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

}  // namespace doa

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#include "block_host.hpp"

int doa::steering_table_args(const char *who, int num_ant_ele, int pspectrum_len, const double *steering)
{
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE) {
        doa::set_error("%s: need 2 <= num_ant_ele <= %d (got %d)", who, DOA_MAX_ANT_ELE, num_ant_ele);
        return DOA_ERR_INVALID_ARG;
    }
    if (pspectrum_len < 1) {
        doa::set_error("%s: pspectrum_len must be > 0 (got %d)", who, pspectrum_len);
        return DOA_ERR_INVALID_ARG;
    }
    if (!steering) {
        doa::set_error("%s: the steering table is NULL", who);
        return DOA_ERR_INVALID_ARG;
    }
    if (!doa::steering_table_finite(steering, num_ant_ele, pspectrum_len)) {
        doa::set_error("%s: the steering table holds a value that is not finite", who);
        return DOA_ERR_INVALID_ARG;
    }
    return DOA_OK;
}

namespace {

// the rows of doa_planar_steering_table (include/doa_hip.h): n_az directions at one elevation; arguments already validated
void planar_steering_rows(int num_ant_ele, const double *xy, int n_az, double az_min_deg, double az_max_deg, double elevation_deg,
                          double *table_out)
{
    const double se = std::sin(elevation_deg * M_PI / 180.0);
    for (int i = 0; i < n_az; i++) {
        const double az = (az_min_deg + (double)i * (az_max_deg - az_min_deg) / (double)n_az) * M_PI / 180.0;
        const double ca = std::cos(az), sa = std::sin(az);
        for (int n = 0; n < num_ant_ele; n++) {
            const double ph = 2.0 * M_PI * se * (xy[2 * n] * ca + xy[2 * n + 1] * sa);
            table_out[2 * ((size_t)i * num_ant_ele + n)] = std::cos(ph);
            table_out[2 * ((size_t)i * num_ant_ele + n) + 1] = std::sin(ph);
        }
    }
}

}  // namespace

extern "C" {

int doa_planar_steering_table(int num_ant_ele, const double *xy, int pspectrum_len, double az_min_deg, double az_max_deg,
                              double elevation_deg, double *table_out)
{
    doa::clear_error();
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE || pspectrum_len < 1 || !xy || !table_out) {
        doa::set_error("planar_steering_table: need 2 <= num_ant_ele <= %d, pspectrum_len > 0 and non-NULL pointers (got %d, %d)",
                       DOA_MAX_ANT_ELE, num_ant_ele, pspectrum_len);
        return DOA_ERR_INVALID_ARG;
    }
    bool finite = std::isfinite(az_min_deg) && std::isfinite(az_max_deg) && std::isfinite(elevation_deg);
    for (int k = 0; k < 2 * num_ant_ele; k++) finite = finite && std::isfinite(xy[k]);
    if (!finite) {
        doa::set_error("planar_steering_table: positions, azimuth limits and elevation must be finite");
        return DOA_ERR_INVALID_ARG;
    }
    if (!(az_max_deg > az_min_deg)) {
        doa::set_error("planar_steering_table: need az_max > az_min (got %g, %g)", az_min_deg, az_max_deg);
        return DOA_ERR_INVALID_ARG;
    }
    planar_steering_rows(num_ant_ele, xy, pspectrum_len, az_min_deg, az_max_deg, elevation_deg, table_out);
    return DOA_OK;
}

int doa_planar_steering_grid(int num_ant_ele, const double *xy, int n_az, double az_min_deg, double az_max_deg, int n_el,
                             double el_min_deg, double el_max_deg, double *table_out)
{
    doa::clear_error();
    if (num_ant_ele < 2 || num_ant_ele > DOA_MAX_ANT_ELE || !xy || !table_out) {
        doa::set_error("planar_steering_grid: need 2 <= num_ant_ele <= %d and non-NULL pointers (got %d)", DOA_MAX_ANT_ELE, num_ant_ele);
        return DOA_ERR_INVALID_ARG;
    }
    if (!doa::peaks2d_args_ok("planar_steering_grid", 1, n_az, n_el, az_min_deg, az_max_deg, el_min_deg, el_max_deg))
        return DOA_ERR_INVALID_ARG;
    for (int k = 0; k < 2 * num_ant_ele; k++)
        if (!std::isfinite(xy[k])) {
            doa::set_error("planar_steering_grid: the positions must be finite");
            return DOA_ERR_INVALID_ARG;
        }
    // one azimuth row block per elevation, by the routine doa_planar_steering_table runs
    for (int e = 0; e < n_el; e++) {
        const double el = el_min_deg + (double)e * (el_max_deg - el_min_deg) / (double)n_el;
        planar_steering_rows(num_ant_ele, xy, n_az, az_min_deg, az_max_deg, el, table_out + 2 * (size_t)e * n_az * num_ant_ele);
    }
    return DOA_OK;
}

// ---- the scan with the two-dimensional pick, on supplied full records (include/doa_hip_test.h) ----------------------------
int doa_hip_array_grid_debug(int num_ant_ele, const double *steering, int n_az, int n_el, float az_min, float az_max, float el_min,
                             float el_max, int wrap_az, int num_max_vals, int n_items, const double *records, int fused,
                             float *spectrum_out, float *val_out, float *az_out, float *el_out)
{
    doa::clear_error();
    const char *who = "hip_array_grid_debug";
    if (!doa::peaks2d_args_ok(who, num_max_vals, n_az, n_el, az_min, az_max, el_min, el_max)) return DOA_ERR_INVALID_ARG;
    const int P = n_az * n_el, N = num_ant_ele, M = num_max_vals, n = n_items;
    if (int rc = doa::steering_table_args(who, N, P, steering); rc != DOA_OK) return rc;
    if (n < 1 || !records || !val_out || !az_out || !el_out || (fused != 0 && fused != 1)) {
        doa::set_error("%s: need n_items >= 1, the records, the three outputs and fused = 0 or 1 (got %d items, fused %d)", who, n, fused);
        return DOA_ERR_INVALID_ARG;
    }
    doa::BlockBase b;
    if (int rc = doa::ensure_device(&b.device); rc != DOA_OK) return rc;
    if (hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking) != hipSuccess) {
        doa::set_error("%s: no stream", who);
        return DOA_ERR_HIP;
    }
    doa::ArrayTable tab;
    doa::Peaks2dTables axes;
    doa::DevBuf d_full, d_spec, d_val, d_az, d_el;
    int rc = tab.build(N, P, steering);
    if (rc == DOA_OK) rc = axes.build(M, n_az, n_el, az_min, az_max, el_min, el_max, wrap_az);
    if (rc == DOA_OK) {
        // the fused launch gets a row pointer only if the caller wants the rows (or the grid takes the two-launch route)
        const bool rows = spectrum_out || !fused || P > doa::kArrayGridFusedMax;
        const size_t out_bytes = (size_t)n * M * sizeof(float);
        doa::HostCall io(b);
        io.in(d_full, records, (size_t)n * doa::full_record_len(N) * sizeof(double));
        if (rows) io.out(d_spec, spectrum_out, (size_t)n * P * sizeof(float));
        io.out(d_val, val_out, out_bytes);
        io.out(d_az, az_out, out_bytes);
        io.out(d_el, el_out, out_bytes);
        rc = io.status();
        if (rc == DOA_OK && fused)
            rc = doa::launch_array_scan_peaks2d(tab, axes, n, d_full.p, rows ? d_spec.p : nullptr, d_val.p, d_az.p, d_el.p, M, b.stream);
        if (rc == DOA_OK && !fused) rc = doa::launch_array_scan(tab, n, d_full.p, d_spec.p, nullptr, b.stream);
        if (rc == DOA_OK && !fused) rc = doa::launch_find_local_max_2d(axes, n, d_spec.p, d_val.p, d_az.p, d_el.p, b.stream);
        rc = io.finish(rc == DOA_OK ? n : rc);
    }
    (void)hipStreamDestroy(b.stream);
    return rc;
}

}  // extern "C"
