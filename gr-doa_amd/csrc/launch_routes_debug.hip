// launch_routes_debug.hip — doa_hip_launch_route_debug (include/doa_hip_test.h): the routes of launch_routes.hpp as text, for
// tests/test_cpu_launch_routes.py.  No handle, no device, no kernel.
#include "kernels.hpp"

#include <string>

namespace {
const char *tf(bool b) { return b ? "true" : "false"; }
// one launch: name<template arguments> grid block lanes-per-work-item work-items grid-strides
void route_line(std::string &t, const std::string &kernel, doa::LaunchDim d, int lanes, long long work, bool strides)
{
    char tail[96];
    snprintf(tail, sizeof tail, " %u %u %d %lld %d\n", d.grid, d.block, lanes, work, strides ? 1 : 0);
    t += kernel + tail;
}
std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...)
{
    char b[200];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}

int cov_route_text(const int *v, int cu, std::string &t)
{
    doa::CovShape s;
    s.N = v[0]; s.K = v[1]; s.ovl = v[2]; s.avg = v[3]; s.n_out = v[4]; s.format = v[5];
    s.pair_aligned = v[6] != 0; s.workspace = v[7] != 0; s.group = v[8] != 0;
    const doa::CovRoute r = doa::cov_route(s, cu);
    if (r.status != DOA_OK) { doa::set_error("%s", r.why); return r.status; }
    const char *L = s.format == DOA_SAMPLE_SC16 ? "Sc16Samples" : "Fc32Samples", *A = s.group ? "CovGroupArgs" : "CovArgs";
    int n = 1;
    switch (r.kernel) {
    case doa::CovKernel::Wave:
        route_line(t, fmt("cov_wave_kernel<%s,%d,%s,%d,%s,%s>", L, r.TN, tf(r.vec2), r.UN, tf(r.NT), A), r.main, 64, s.n_out, true);
        break;
    case doa::CovKernel::Pieces:
        route_line(t, fmt("cov_piece_kernel<%s,%d,%d,%s>", L, r.TN, r.UN, tf(r.NT)), r.main, 64, r.n_steps, true);
        route_line(t, "cov_combine_kernel", r.second, 1, (long long)s.n_out * s.N * s.N, false);
        n = 2;
        break;
    case doa::CovKernel::Mfma:
        route_line(t, fmt("cov_mfma_kernel<%s,%s,%d>", L, tf(r.vec2), r.UN), r.main, 64, s.n_out, true);
        if (r.second.grid) { route_line(t, "cov_fb_kernel", r.second, 1, (long long)s.n_out * ((s.N * s.N + 1) / 2), false); n = 2; }
        break;
    }
    t += fmt("workspace_bytes %zu\n", r.workspace_bytes);
    return n;
}

int evd_route_text(const int *v, std::string &t)
{
    if (v[4] < 0 || v[4] > 5) { doa::set_error("hip_launch_route_debug: eigen mode %d outside 0..5", v[4]); return DOA_ERR_INVALID_ARG; }
    doa::EvdShape s;
    s.N = v[0]; s.M = v[1]; s.bits = v[2]; s.n_items = v[3]; s.mode = (doa::EvdMode)v[4];
    s.pn_out = v[5] != 0; s.cheb = v[6] != 0; s.es_rec = v[7] != 0;
    const doa::EvdRoute r = doa::evd_route(s);
    if (r.status != DOA_OK) { doa::set_error("%s", r.why); return r.status; }
    const char *T = s.bits == 32 ? "float" : "double";
    static const char *const variant[6] = {"", "_counts", "_record", "_full", "", ""};
    const bool plain = !variant[v[4]][0];
    std::string k;
    switch (r.kernel) {
    case doa::EvdKernel::OneLane:
        // (the count-per-item and group forms are compiled in double only: music_evd.hip, launch_evd_one_lane)
        k = fmt("music_evd_kernel<%d,%s,%s>", s.N, s.mode == doa::EvdMode::Fixed ? T : "double", s.mode == doa::EvdMode::Group ? "EvdGroup" : (s.mode == doa::EvdMode::Counts ? "EvdOneCounts" : "EvdOne"));
        break;
    case doa::EvdKernel::Quad: k = fmt("music_evd_quad_kernel<2,%s>", tf(r.PN)); break;
    case doa::EvdKernel::Subspace: k = fmt("music_evd_subspace_kernel<%d,%d,%s>", r.G, s.M, tf(r.PN)); break;
    case doa::EvdKernel::Jacobi:
        k = plain ? fmt("music_evd_group_kernel<%d,%s>", r.G, T) : fmt("music_evd_group%s_kernel<%d>", variant[v[4]], r.G);
        break;
    case doa::EvdKernel::Block16:
        k = plain ? fmt("music_evd_block16_kernel<%s,%s>", T, tf(r.LEAN)) : fmt("music_evd_block16%s_kernel", variant[v[4]]);
        break;
    }
    route_line(t, k, r.dim, r.kernel == doa::EvdKernel::Subspace ? 64 : (r.G == 16 ? 64 : r.G), s.n_items, false);
    t += fmt("counts_fallbacks %d\n", r.counts_fallbacks ? 1 : 0);
    return 1;
}

int scan_route_text(const int *v, int cu, std::string &t)
{
    doa::ScanShape s;
    s.n_ant = v[0]; s.bits = v[1]; s.P = v[2]; s.n_items = v[3]; s.spec_aligned = v[4] != 0; s.q = v[5] != 0; s.pick = v[6] != 0;
    s.M = v[7]; s.store = v[8] != 0; s.cheb = v[9] != 0; s.group = v[10] != 0;
    const doa::ScanRoute r = doa::scan_route(s, cu);
    if (r.status != DOA_OK) { doa::set_error("%s", r.why); return r.status; }
    const char *T = s.bits == 32 ? "float" : "double";
    std::string k;
    switch (r.kernel) {
    case doa::ScanKernel::Lean:
        k = fmt("music_scan_peak1_kernel<%d,%d,%s,%s,%s,%s,0,%s>", r.N, r.CH, T, tf(r.MULTI), tf(r.PEAKS), tf(r.STORE), s.group ? "ScanGroup" : "ScanOne");
        break;
    case doa::ScanKernel::Long: k = fmt("music_scan_peak_long_kernel<%d,%s,0>", r.N, T); break;
    case doa::ScanKernel::Stream: k = fmt("music_scan_stream_kernel<%d,%s>", r.N, T); break;
    case doa::ScanKernel::Fast:
        k = fmt("music_scan_kernel<%d,%d,%s,%s,%s,%s,%s>", r.N, r.CH, T, tf(r.HAS_Q), tf(r.PEAKS), tf(r.NT), tf(r.ZREG));
        break;
    case doa::ScanKernel::Generic: k = fmt("music_scan_generic_kernel<%d,%s>", r.N, T); break;
    }
    route_line(t, k, r.dim, 64, s.n_items, true);
    t += fmt("reads_cheb %d\npicked %d\n", r.reads_cheb ? 1 : 0, r.picked ? 1 : 0);
    return 1;
}
}  // namespace

extern "C" {

int doa_hip_launch_route_debug(int stage, const int *shape, int n_shape, int cu_count, char *text_out, int text_cap)
{
    doa::clear_error();
    static const int want[3] = {9, 8, 11};
    if (stage < 0 || stage > 2 || !shape || n_shape != want[stage] || cu_count < 1 || !text_out || text_cap < 1) {
        doa::set_error("hip_launch_route_debug: bad arguments (stage 0..2 with 9 / 8 / 11 shape values, cu_count >= 1, text_out)");
        return DOA_ERR_INVALID_ARG;
    }
    std::string t;
    const int n = stage == 0 ? cov_route_text(shape, cu_count, t) : (stage == 1 ? evd_route_text(shape, t) : scan_route_text(shape, cu_count, t));
    if (n < 0) return n;
    if ((int)t.size() >= text_cap) { doa::set_error("hip_launch_route_debug: text_cap=%d is too small", text_cap); return DOA_ERR_INVALID_ARG; }
    memcpy(text_out, t.c_str(), t.size() + 1);
    return n;
}

}  // extern "C"
