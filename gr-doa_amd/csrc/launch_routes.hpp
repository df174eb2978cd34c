// launch_routes.hpp — which kernel instantiation a shape launches, and with which grid: the covariance stage (K1,
// autocorrelate.hip), the eigen stage (K2+K3, music_evd.hip) and the scan of a uniform linear array (K4, music_scan_impl.hpp).
// One function and one plain record per stage.  The launchers compute the route, refuse if it refuses, and switch on its
// kernel; nothing else restates these rules.  Pure host logic on integers: no HIP call, no device; the compute-unit count is a
// parameter (the launchers pass cu_count()), and the lab knobs go in as structs whose defaults are the shipped values.
// tests/test_cpu_launch_routes.py drives all three through doa_hip_launch_route_debug.
#pragma once
#include <cstddef>
#include <cstdio>

#include "../../include/doa_hip.h"

namespace doa {

struct LaunchDim { unsigned grid = 0, block = 0; };     // workgroups, threads per workgroup; grid 0 = no such launch
// status != DOA_OK: the launcher sets `why` as the error and returns the status without a launch
struct RouteRefusal { int status = DOA_OK; char why[120] = {0}; };

constexpr int kRouteWave = 64, kRouteWavesPerBlock = 4;
inline unsigned route_blocks(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }
inline unsigned route_capped(unsigned blocks, int cap) { return (cap >= 0 && blocks > (unsigned)cap) ? (unsigned)cap : blocks; }

// ---- K1 -------------------------------------------------------------------------------------------------------------------
struct CovKnobs { int waves_per_cu = -1, mfma_waves_per_cu = 16, group_waves_per_cu = 0; };      // DOA_COV_*_WAVES_PER_CU
struct CovShape {
    int N = 0, K = 0, ovl = 0, avg = 0, n_out = 0, format = DOA_SAMPLE_FC32;
    bool pair_aligned = false;      // every stream aligned to two samples
    bool workspace = false;         // a piece-sum workspace was supplied
    bool group = false;             // a group of batches (CovGroupArgs; n_out = the group's total, ovl = 0)
};
enum class CovKernel { Wave, Pieces, Mfma };
struct CovRoute : RouteRefusal {
    CovKernel kernel = CovKernel::Wave;
    int TN = 0, UN = 1;             // TN: the compiled array size of the wave and piece kernels
    bool vec2 = false, NT = false;  // pair loads; non-temporal loads
    LaunchDim main;                 // cov_wave_kernel / cov_piece_kernel / cov_mfma_kernel
    LaunchDim second;               // Pieces: cov_combine_kernel; Mfma with avg == 1: cov_fb_kernel
    size_t workspace_bytes = 0;     // the piece-sum workspace this shape wants (0: it never takes the read-once path)
    int q = 0, r = 0, n_steps = 0;  // Pieces: K = q S + r, n_out + q steps
};
// the pair-load route: every stream aligned to two samples and an even step
inline bool cov_pair_loads(int K, int ovl, bool pair_aligned) { return pair_aligned && (K - ovl) % 2 == 0; }
// 16-byte loads in flight per stream and wave (measurements: autocorrelate.hip)
constexpr int cov_unroll(int TN) { return TN <= 6 ? 4 : 2; }
// bytes of piece-sum workspace the read-once path of overlapping windows wants (0: the shape does not take it)
inline size_t cov_workspace_bytes(int N, int K, int ovl, int n_out)
{
    const int S = K - ovl;
    if (ovl <= 0 || N > 8 || n_out <= 0 || (S & 1) || ((K % S) & 1)) return 0;
    return (size_t)(n_out + K / S) * 2 * N * N * 2 * sizeof(float);
}
inline CovRoute cov_route(const CovShape &s, int cu, const CovKnobs &knobs = CovKnobs())
{
    CovRoute rt;
    const int wpb = kRouteWavesPerBlock;
    rt.vec2 = cov_pair_loads(s.K, s.ovl, s.pair_aligned);
    rt.main.block = wpb * kRouteWave;
    if (s.group) {
        // ONE WAVE PER SNAPSHOT, no cap (autocorrelate.hip: launch_autocorrelate_group)
        if (s.N < 2 || s.N > 4) {
            rt.status = DOA_ERR_INVALID_ARG;
            snprintf(rt.why, sizeof rt.why, "autocorrelate: not a group shape (N=%d)", s.N);
            return rt;
        }
        rt.TN = s.N;
        rt.main.grid = route_capped(route_blocks(s.n_out, wpb), knobs.group_waves_per_cu > 0 ? cu * knobs.group_waves_per_cu / wpb : -1);
    } else if (s.N <= 8) {
        rt.TN = s.N;
        rt.workspace_bytes = cov_workspace_bytes(s.N, s.K, s.ovl, s.n_out);
        // waves per CU one launch may occupy (0 = one wave per snapshot, no cap); larger launches grid-stride
        const int wpc = knobs.waves_per_cu >= 0 ? knobs.waves_per_cu : (s.N <= 4 ? 16 : 8);
        const int cap = wpc > 0 ? cu * wpc / wpb : -1;
        if (s.workspace && rt.vec2 && rt.workspace_bytes > 0) {
            rt.kernel = CovKernel::Pieces;
            const int S = s.K - s.ovl;
            rt.q = s.K / S; rt.r = s.K % S; rt.n_steps = s.n_out + rt.q;
            rt.UN = cov_unroll(rt.TN); rt.NT = true;
            rt.main.grid = route_capped(route_blocks(rt.n_steps, wpb), cap);
            rt.second.grid = route_blocks((long long)s.n_out * s.N * s.N, 256); rt.second.block = 256;
            return rt;
        }
        rt.main.grid = route_capped(route_blocks(s.n_out, wpb), cap);
    } else {
        rt.kernel = CovKernel::Mfma;
        rt.UN = 4;                              // 4 wave-iterations (64 samples) of loads in flight
        rt.main.grid = route_capped(route_blocks(s.n_out, wpb), cu * knobs.mfma_waves_per_cu / wpb);
        if (s.avg == 1) { rt.second.grid = route_blocks((long long)s.n_out * ((s.N * s.N + 1) / 2), 256); rt.second.block = 256; }
        return rt;
    }
    // the wave kernel: pair loads are a read-once stream (non-temporal), single loads are not unrolled
    if (rt.vec2) { rt.UN = cov_unroll(rt.TN); rt.NT = true; }
    return rt;
}

// ---- K2+K3 ----------------------------------------------------------------------------------------------------------------
enum class EvdMode { Fixed, Counts, Record, Full, Calibrate, Group };
struct EvdShape {
    int N = 0, M = 0, bits = 64, n_items = 0;
    EvdMode mode = EvdMode::Fixed;
    bool pn_out = false;            // Fixed: the projector diagnostics are wanted
    bool cheb = false, es_rec = false;      // Counts: the Chebyshev record / the signal-subspace record is wanted
    bool quad = true;               // lab knob DOA_EVD_QUAD
};
// OneLane: music_evd_kernel<N, T, Src>; Quad: music_evd_quad_kernel<2, PN>; Subspace: music_evd_subspace_kernel<G, MC, PN>;
// Jacobi: music_evd_group[_counts|_full|_record]_kernel<G[, T]>, G = 4 / 8; Block16: music_evd_block16[_...]_kernel[<T, LEAN>]
enum class EvdKernel { OneLane, Quad, Subspace, Jacobi, Block16 };
struct EvdRoute : RouteRefusal {
    EvdKernel kernel = EvdKernel::OneLane;
    int G = 1;                      // lanes per item
    bool PN = false, LEAN = false;  // Quad, Subspace: PN; Block16 in the Fixed and Calibrate modes: LEAN (false elsewhere)
    bool counts_fallbacks = false;  // the launch gets the device's fall-back counter
    LaunchDim dim;
};
inline EvdRoute evd_route(const EvdShape &s)
{
    EvdRoute rt;
    rt.dim.block = kRouteWave;
    if (s.mode == EvdMode::Group) {
        // the one-lane kernel over a group of batches: double, and not the quad kernel's N = 4, M = 2
        if (s.N < 2 || s.N > 4 || (s.N == 4 && s.M == 2) || s.bits != 64) {
            rt.status = DOA_ERR_INVALID_ARG;
            snprintf(rt.why, sizeof rt.why, "MUSIC: not a group shape (N=%d, M=%d, %d bits)", s.N, s.M, s.bits);
            return rt;
        }
    } else if (s.mode != EvdMode::Calibrate && (s.N < 2 || s.N > DOA_MAX_ANT_ELE)) {
        rt.status = DOA_ERR_UNSUPPORTED;
        snprintf(rt.why, sizeof rt.why, "MUSIC: num_ant_ele=%d outside the built range 2..%d", s.N, DOA_MAX_ANT_ELE);
        return rt;
    }
    const bool f64 = (s.bits != 32);
    auto one_lane = [&](bool counter) -> EvdRoute & {
        rt.kernel = EvdKernel::OneLane; rt.G = 1; rt.counts_fallbacks = counter;
        rt.dim.grid = route_blocks(s.n_items, 64);
        return rt;
    };
    // the Jacobi form of an array size: one wave per item above 8 elements, else 8 lanes per item above 4, else 4
    auto jacobi = [&](bool lean16) -> EvdRoute & {
        rt.G = s.N > 8 ? 16 : (s.N > 4 ? 8 : 4);
        rt.kernel = rt.G == 16 ? EvdKernel::Block16 : EvdKernel::Jacobi;
        rt.LEAN = rt.G == 16 && lean16;
        rt.dim.grid = rt.G == 16 ? (unsigned)s.n_items : route_blocks(s.n_items, kRouteWave / rt.G);
        return rt;
    };
    switch (s.mode) {
    case EvdMode::Group: return one_lane(true);
    case EvdMode::Calibrate: return jacobi(false);
    case EvdMode::Record: return jacobi(false);
    case EvdMode::Full: return jacobi(false);
    case EvdMode::Counts:
        // always the Jacobi forms (the subspace iterations never form the noise eigenvalues)
        if (s.N <= 4 && !s.es_rec) return one_lane(false);
        // N <= 4: the record needs the eigenvectors by rows: four lanes per item (no Chebyshev record from this form's count mode)
        if (s.N <= 4 && s.cheb) {
            rt.status = DOA_ERR_INVALID_ARG;
            snprintf(rt.why, sizeof rt.why, "MUSIC: the signal-subspace record and the Chebyshev record do not come from one launch");
            return rt;
        }
        return jacobi(false);
    case EvdMode::Fixed: break;
    }
    // wide arrays, few sources, double: the signal-subspace iteration with the block Jacobi as its per-item fall-back
    // (4 < N <= 16, 1 <= M <= 4, 2 M <= N: the iteration pays when the signal subspace is the small one)
    if (f64 && s.N > 4 && s.M >= 1 && s.M <= 4 && 2 * s.M <= s.N) {
        rt.kernel = EvdKernel::Subspace; rt.G = s.N <= 8 ? 8 : 16; rt.PN = s.pn_out; rt.counts_fallbacks = true;
        rt.dim.grid = (unsigned)s.n_items;
        return rt;
    }
    if (s.N > 4) return jacobi(!s.pn_out);
    // N = 4, two sources, double: four lanes per item (measurements: music_evd.hip, above launch_evd)
    if (f64 && s.quad && s.N == 4 && s.M == 2) {
        rt.kernel = EvdKernel::Quad; rt.G = 4; rt.PN = s.pn_out; rt.counts_fallbacks = true;
        rt.dim.grid = route_blocks(s.n_items, 16);
        return rt;
    }
    return one_lane(f64);           // float: no subspace iteration to count
}

// ---- K4 -------------------------------------------------------------------------------------------------------------------
// N <= 4 in double: the lean scan kernel reads the Chebyshev record the stage in front wrote (kernels.hpp: EvdOut::cheb_d), and
// that record exists (spectrum_chain.hpp: spectrum_plan).  LeanRecord<N, T>::kPre is this predicate on the device side.
constexpr bool scan_reads_cheb(int N, int bits) { return N <= 4 && bits == 64; }
// compiled polynomial sizes: an array of n elements uses the next size up with zero high-order coefficients
constexpr int scan_poly_size(int n_ant) { return n_ant <= 4 ? n_ant : (n_ant <= 6 ? 6 : (n_ant <= 8 ? 8 : (n_ant <= 12 ? 12 : 16))); }
// the spectrum lengths the lean kernel is compiled for (P == 256 CH exactly)
constexpr bool scan_lean_length(int P) { return P == 256 || P == 512 || P == 1024; }

struct ScanKnobs { int lean_wpb = kRouteWavesPerBlock, lean_waves_per_cu = 0, notrim = 0, waves_per_cu = 8; };   // DOA_SCAN_*
struct ScanShape {
    int n_ant = 0, bits = 64, P = 0, n_items = 0;
    bool spec_aligned = false;      // the spectrum pointer (a group: every one) is 16-byte aligned
    bool q = false;                 // the un-normalised null spectrum is wanted (diagnostics)
    bool pick = false;              // a fused peak pick is wanted and possible (outputs given, vector length == P)
    int M = 0;                      // the pick's num_max_vals
    bool store = true;              // false: angles only, the rows are scratch
    bool cheb = false;              // a Chebyshev record was supplied
    bool group = false;             // a group of batches (ScanGroup; n_items = the group's total; always picks)
};
// Lean: music_scan_peak1_kernel<N, CH, T, MULTI, PEAKS, STORE, 0, Out>; Long: music_scan_peak_long_kernel<N, T>;
// Stream: music_scan_stream_kernel<N, T>; Fast: music_scan_kernel<N, CH, T, HAS_Q, PEAK, NT, ZREG>; Generic: music_scan_generic_kernel<N, T>
enum class ScanKernel { Lean, Long, Stream, Fast, Generic };
struct ScanRoute : RouteRefusal {
    ScanKernel kernel = ScanKernel::Generic;
    int N = 0, CH = 0;              // the compiled polynomial size; 256-angle chunks per row (Lean, Fast)
    bool MULTI = false, PEAKS = false, STORE = true;    // Lean; PEAKS is also Fast's PEAK
    bool HAS_Q = false, NT = false, ZREG = true;        // Fast
    int M_pick = 0;                 // Long: the kernel's M (0 = spectrum only)
    bool reads_cheb = false;        // the records are the Chebyshev form's
    bool picked = false;            // the fused peak pick runs: the caller has no K5 to launch
    LaunchDim dim;
};
inline ScanRoute scan_route(const ScanShape &s, int cu, const ScanKnobs &knobs = ScanKnobs())
{
    ScanRoute rt;
    const int wpb = kRouteWavesPerBlock;
    if (s.n_ant < 2 || s.n_ant > DOA_MAX_ANT_ELE) {
        rt.status = DOA_ERR_UNSUPPORTED;
        snprintf(rt.why, sizeof rt.why, "MUSIC: num_ant_ele=%d outside the built range 2..%d", s.n_ant, DOA_MAX_ANT_ELE);
        return rt;
    }
    rt.N = scan_poly_size(s.n_ant);
    const bool f64 = (s.bits != 32), pick = s.pick || s.group;
    const bool aligned = (s.P % 4 == 0) && s.spec_aligned;
    const bool pre = scan_reads_cheb(rt.N, f64 ? 64 : 32);
    // the lean benchmark-shape kernel; also without a peak pick, so that block and pipeline produce the same spectrum bit for
    // bit.  For N <= 4 in double it reads the pre-transformed records, which the caller must supply.
    const bool lean = aligned && !s.q && s.n_ant == rt.N && scan_lean_length(s.P) && (!pre || s.cheb);
    if (s.group && !(lean && pre)) {
        rt.status = DOA_ERR_INVALID_ARG;
        snprintf(rt.why, sizeof rt.why, "MUSIC: not a group the lean scan kernel takes (N=%d, P=%d, %d bits)", s.n_ant, s.P, s.bits);
        return rt;
    }
    rt.dim.block = wpb * kRouteWave;
    if (lean) {
        rt.kernel = ScanKernel::Lean; rt.CH = s.P / 256; rt.reads_cheb = pre; rt.picked = pick;
        rt.PEAKS = pick; rt.MULTI = pick && s.M != 1; rt.STORE = !pick || s.store;
        // workgroup size in waves, 1..4 (the kernels are bounded to 256 threads and their per-wave LDS rows to four)
        const int lwpb = knobs.lean_wpb < 1 ? 1 : (knobs.lean_wpb > 4 ? 4 : knobs.lean_wpb);
        rt.dim.block = lwpb * kRouteWave;
        unsigned lb = route_blocks(s.n_items, lwpb);
        // Waves per CU: 12 up to a few items per wave, 16 -- all the 104-VGPR kernel can hold -- beyond (measurements:
        // music_scan_impl.hpp, launch_scan_lean)
        const int per_wave16 = s.n_items / (cu * 16);
        const int lwpc = knobs.lean_waves_per_cu > 0 ? knobs.lean_waves_per_cu : (per_wave16 >= 4 ? 16 : 12);
        const unsigned cap = (unsigned)(cu * lwpc / lwpb);
        if (lb > cap && !knobs.notrim) {
            // every wave takes the same number of items (4096 items on a cap of 3072 waves would be one round of 3072 and a
            // second of 1024 with two thirds of the chip idle: 2048 waves with two items each instead)
            const int cap_waves = (int)cap * lwpb;
            const int per_wave = (s.n_items + cap_waves - 1) / cap_waves;
            const int waves = (s.n_items + per_wave - 1) / per_wave;
            lb = route_blocks(waves, lwpb);
        } else if (lb > cap) lb = cap;
        rt.dim.grid = lb;
        return rt;
    }
    const unsigned blocks = route_blocks(s.n_items, wpb);
    // long spectra without diagnostics, double: the row does not fit the registers next to peak_pick<16>
    if (aligned && s.P > 2048 && f64 && !s.q) {
        // a multiple of 64 up to 4096: scan + K5 in one launch, the row staged in LDS (64 KiB per workgroup: two per CU)
        if ((!pick || s.M >= 1) && s.P % 64 == 0 && s.P <= 4096) {
            rt.kernel = ScanKernel::Long; rt.M_pick = pick ? s.M : 0; rt.picked = pick;
            rt.dim.grid = route_capped(blocks, cu * 2);
            return rt;
        }
        // other lengths: the rolled two-pass kernel; the peak pick, if any, is left to the caller
        rt.kernel = ScanKernel::Stream;
        rt.dim.grid = route_capped(blocks, cu * 16 / wpb);
        return rt;
    }
    rt.dim.grid = route_capped(blocks, cu * knobs.waves_per_cu / wpb);
    if (aligned && s.P <= 4096) {
        rt.kernel = ScanKernel::Fast;
        rt.CH = s.P <= 256 ? 1 : (s.P <= 512 ? 2 : (s.P <= 1024 ? 4 : (s.P <= 2048 ? 8 : 16)));
        rt.ZREG = rt.CH <= 4 || !f64;               // float tables fit the register file up to P = 4096
        // three variants: diagnostics (Q out), fused with the peak pick, plain; spectra are write-once -> non-temporal
        // stores in the two production variants
        rt.HAS_Q = s.q; rt.PEAKS = !s.q && pick; rt.NT = !s.q;
        rt.picked = rt.PEAKS;
        return rt;
    }
    return rt;                                      // Generic: any P, any alignment
}

// Batches may share a group's launches exactly when both group modes accept the shape (with the records and the alignment a
// group has by construction): today N = 2..4 in double, not N = 4 with M = 2, P = 256 / 512 / 1024
inline bool group_routes_accept(int N, int M, int P, int bits)
{
    EvdShape e;
    e.mode = EvdMode::Group; e.N = N; e.M = M; e.bits = bits; e.n_items = 1;
    ScanShape s;
    s.group = true; s.n_ant = N; s.bits = bits; s.P = P; s.M = M; s.n_items = 1; s.cheb = s.spec_aligned = true;
    return evd_route(e).status == DOA_OK && scan_route(s, 1).status == DOA_OK;
}

}  // namespace doa
