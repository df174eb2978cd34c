// bin_plan.hpp — the rules of a "snapshot of bins" (include/doa_hip.h, "Snapshots of bins"), each stated once for the blocks
// that write one (channel_covariance) or read one (wideband_music, focus_covariance, doa_rss_focusing_matrices).  Plain
// functions for host and device code.  A check returns DOA_OK, or DOA_ERR_INVALID_ARG with the error set (who: the entry's
// name); an entry runs them in the order its refusals have always had (tests/test_cpu_bin_plan_refusals.py pins it).
#pragma once
#include "common.hpp"

#include <climits>
#include <cmath>

namespace doa {

// nu_f of bin f of an fft_len-point FFT (numpy.fft.fftfreq) and the element spacing in wavelengths at that bin; pure
inline double wideband_bin_nu(int fft_len, int bin) { return (bin < fft_len / 2 ? (double)bin : (double)bin - fft_len) / fft_len; }
inline double wideband_bin_spacing(float norm_spacing, double rate_over_carrier, int fft_len, int bin)
{
    const double s = wideband_bin_nu(fft_len, bin) * rate_over_carrier;
    return (double)norm_spacing * (1.0 + s);
}

// lg(F) = 4..8 for the transform sizes 16, 32, 64, 128 and 256; -1 for every other F (the message is the caller's)
inline int fft_len_log2(int F) { return F == 16 ? 4 : F == 32 ? 5 : F == 64 ? 6 : F == 128 ? 7 : F == 256 ? 8 : -1; }

// The bins of a snapshot, in item order: nb of the F bins of the transform, from bin `first` on, wrapping.
struct BinSelection {
    int F = 0, first = 0, nb = 0;
    int bin(int j) const { return (first + j) % F; }
};
inline int check_bin_selection(const char *who, int F, int first, int nb)
{
    if (first >= 0 && first < F && nb >= 1 && nb <= F) return DOA_OK;
    set_error("%s: need 0 <= first_bin < fft_len and 1 <= num_bins <= fft_len (got %d, %d, fft_len %d)", who, first, nb, F);
    return DOA_ERR_INVALID_ARG;
}

// The band of a uniform linear array: the spacing at the carrier, the band's width, the spacing at every selected bin (the
// first bin outside (0, 0.5] is named).  Two checks, not one, because the entries refuse other arguments between them.
inline int check_norm_spacing(const char *who, float norm_spacing)
{
    if (norm_spacing > 0.0f && norm_spacing <= 0.5f) return DOA_OK;
    set_error("%s: need 0 < norm_spacing <= 0.5 (got %g)", who, (double)norm_spacing);
    return DOA_ERR_INVALID_ARG;
}
inline int check_rate_over_carrier(const char *who, double rate_over_carrier)
{
    if (std::isfinite(rate_over_carrier) && rate_over_carrier >= 0.0) return DOA_OK;
    set_error("%s: rate_over_carrier must be finite and >= 0 (got %g)", who, rate_over_carrier);
    return DOA_ERR_INVALID_ARG;
}
inline int check_bin_spacings(const char *who, float norm_spacing, double rate_over_carrier, const BinSelection &sel)
{
    for (int j = 0; j < sel.nb; j++) {
        const double df = wideband_bin_spacing(norm_spacing, rate_over_carrier, sel.F, sel.bin(j));
        if (df > 0.0 && df <= 0.5) continue;
        set_error("%s: the element spacing at bin %d is %g wavelengths, outside (0, 0.5] (norm_spacing %g, rate_over_carrier %g)",
                  who, sel.bin(j), df, (double)norm_spacing, rate_over_carrier);
        return DOA_ERR_INVALID_ARG;
    }
    return DOA_OK;
}

// n snapshots of nb bins are n * nb items, and the items of one call are counted in an int
inline int snapshot_items(const char *who, int n, int nb)
{
    if ((long long)n * nb <= INT_MAX) return DOA_OK;
    set_error("%s: %d snapshots of %d bins are more items than one call takes", who, n, nb);
    return DOA_ERR_INVALID_ARG;
}

// The used-bin rule: a bin counts when its weight is positive and finite.  The item (or record) of any other bin is not read.
__host__ __device__ inline bool bin_weight_used(float w) { return w > 0.0f && w < INFINITY; }

}  // namespace doa
