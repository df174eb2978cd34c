// calibration_files.hip — the producing side of the two calibration files the library reads.
//
// calib_mean: the reduction of the reference's save_antenna_calib sink (python/save_antenna_calib.py:61-69: per antenna
// element i, numpy.mean(G[i::num_inputs]) of the flattened magnitude items and the same of the phase items, over ALL items
// of the work call), on the device, so that autocorrelate -> calibrate_lin_array -> here needs no host round trip.  The
// complex form takes calibrate_lin_array's output items as they are and forms |c| and atan2f(im, re) per element itself:
// blocks.complex_to_magphase of apps/run_calib_lin_array_simulation.grc.
//   gain[m] = mean_i mag[i * N + m],   phase[m] = mean_i phase[i * N + m],   i = 0 .. n_items-1
// numpy.mean of a float32 array accumulates pairwise in float32; here, as in compass_mean.hip, the sum is carried in double
// in a fixed order and rounded once: the correctly rounded mean.  n_items == 0 gives NaN, as numpy.mean of nothing does.
//
// Writers: the text formats of the phase file (python/findmax_and_save.py:66-78, python/average_and_save.py:68-80: one
// value per line; read by python/phase_correct_hier.py:33-45) and of the antenna file (python/save_antenna_calib.py:61-72:
// "gain phase" per line; read by lib/antenna_correction_impl.cc:56-73).  No device involved.
#include "kernels.hpp"

#include <cmath>

namespace doa {

template <bool CPLX>
__global__ __launch_bounds__(256) void calib_mean_kernel(const void *__restrict__ a_in, const float *__restrict__ ph_in,
                                                         float *__restrict__ gain_out, float *__restrict__ phase_out, int n, int N)
{
    __shared__ double s_g[256], s_p[256];
    const int m = blockIdx.x, t = threadIdx.x;
    double g = 0.0, p = 0.0;
    for (int i = t; i < n; i += 256) {
        const size_t e = (size_t)i * N + m;
        if constexpr (CPLX) {
            const float2 c = static_cast<const float2 *>(a_in)[e];
            g += (double)hypotf(c.x, c.y);
            p += (double)atan2f(c.y, c.x);
        } else {
            g += (double)static_cast<const float *>(a_in)[e];
            p += (double)ph_in[e];
        }
    }
    s_g[t] = g; s_p[t] = p;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {          // fixed tree: the result does not depend on scheduling
        if (t < s) { s_g[t] += s_g[t + s]; s_p[t] += s_p[t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        gain_out[m] = (n > 0) ? (float)(s_g[0] / (double)n) : nanf("");
        phase_out[m] = (n > 0) ? (float)(s_p[0] / (double)n) : nanf("");
    }
}

static int calib_mean_args(const char *what, int n_items, int num_inputs, const void *a, const void *b, bool need_b,
                           const float *gain_out, const float *phase_out)
{
    if (num_inputs <= 0 || num_inputs > DOA_MAX_ANT_ELE) {
        set_error("%s: num_inputs=%d outside 1..%d", what, num_inputs, DOA_MAX_ANT_ELE);
        return DOA_ERR_INVALID_ARG;
    }
    if (n_items < 0 || !gain_out || !phase_out || (n_items > 0 && (!a || (need_b && !b)))) {
        set_error("%s: bad arguments", what);
        return DOA_ERR_INVALID_ARG;
    }
    return DOA_OK;
}

static int launch_calib_mean(bool cplx, int n_items, int N, const void *d_a, const void *d_ph, float *d_gain, float *d_phase,
                             hipStream_t st)
{
    if (cplx) hipLaunchKernelGGL(calib_mean_kernel<true>, dim3(N), dim3(256), 0, st, d_a, nullptr, d_gain, d_phase, n_items, N);
    else      hipLaunchKernelGGL(calib_mean_kernel<false>, dim3(N), dim3(256), 0, st, d_a, static_cast<const float *>(d_ph),
                                 d_gain, d_phase, n_items, N);
    DOA_HIP_TRY(hipGetLastError());
    return DOA_OK;
}

// host entry of both forms: a one-shot calibration step, so it allocates and frees what it stages
static int calib_mean_host(bool cplx, int n_items, int N, const void *a, const void *ph, float *gain_out, float *phase_out)
{
    int dev = 0;
    if (int rc = ensure_device(&dev); rc != DOA_OK) return rc;
    const size_t elem = cplx ? sizeof(float2) : sizeof(float);
    const size_t a_bytes = (size_t)n_items * N * elem, p_bytes = cplx ? 0 : a_bytes;
    DevBuf d_a, d_p, d_o;
    int rc = d_a.reserve(a_bytes ? a_bytes : 4);
    if (rc == DOA_OK) rc = d_p.reserve(p_bytes ? p_bytes : 4);
    if (rc == DOA_OK) rc = d_o.reserve(2 * N * sizeof(float));
    auto done = [&](int r) { d_a.release(); d_p.release(); d_o.release(); return r; };
    if (rc != DOA_OK) return done(rc);
    hipError_t e = hipSuccess;
    if (a_bytes) e = hipMemcpy(d_a.p, a, a_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && p_bytes) e = hipMemcpy(d_p.p, ph, p_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error("calib_mean: copy to the device failed: %s", hipGetErrorString(e)); return done(DOA_ERR_HIP); }
    float *o = d_o.as<float>();
    rc = launch_calib_mean(cplx, n_items, N, d_a.p, d_p.p, o, o + N, nullptr);
    if (rc != DOA_OK) return done(rc);
    float host[2 * DOA_MAX_ANT_ELE];
    e = hipMemcpy(host, o, 2 * N * sizeof(float), hipMemcpyDeviceToHost);       // waits for the kernel (null stream)
    if (e != hipSuccess) { set_error("calib_mean: copy from the device failed: %s", hipGetErrorString(e)); return done(DOA_ERR_HIP); }
    memcpy(gain_out, host, N * sizeof(float));
    memcpy(phase_out, host + N, N * sizeof(float));
    return done(n_items);
}

}  // namespace doa

extern "C" {

int doa_calib_mean_work_dev(int n_items, int num_inputs, const float *d_mag_in, const float *d_phase_in, float *d_gain_out,
                            float *d_phase_out, void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::calib_mean_args("calib_mean_work_dev", n_items, num_inputs, d_mag_in, d_phase_in, true, d_gain_out, d_phase_out); rc != DOA_OK) return rc;
    if (int rc = doa::ensure_device(nullptr); rc != DOA_OK) return rc;
    const int rc = doa::launch_calib_mean(false, n_items, num_inputs, d_mag_in, d_phase_in, d_gain_out, d_phase_out,
                                          static_cast<hipStream_t>(hip_stream));
    return rc == DOA_OK ? n_items : rc;
}

int doa_calib_mean_work(int n_items, int num_inputs, const float *mag_in, const float *phase_in, float *gain_out, float *phase_out)
{
    doa::clear_error();
    if (int rc = doa::calib_mean_args("calib_mean_work", n_items, num_inputs, mag_in, phase_in, true, gain_out, phase_out); rc != DOA_OK) return rc;
    return doa::calib_mean_host(false, n_items, num_inputs, mag_in, phase_in, gain_out, phase_out);
}

int doa_calib_mean_complex_work_dev(int n_items, int num_inputs, const void *d_c_in, float *d_gain_out, float *d_phase_out,
                                    void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::calib_mean_args("calib_mean_complex_work_dev", n_items, num_inputs, d_c_in, nullptr, false, d_gain_out, d_phase_out); rc != DOA_OK) return rc;
    if (int rc = doa::ensure_device(nullptr); rc != DOA_OK) return rc;
    const int rc = doa::launch_calib_mean(true, n_items, num_inputs, d_c_in, nullptr, d_gain_out, d_phase_out,
                                          static_cast<hipStream_t>(hip_stream));
    return rc == DOA_OK ? n_items : rc;
}

int doa_calib_mean_complex_work(int n_items, int num_inputs, const void *c_in, float *gain_out, float *phase_out)
{
    doa::clear_error();
    if (int rc = doa::calib_mean_args("calib_mean_complex_work", n_items, num_inputs, c_in, nullptr, false, gain_out, phase_out); rc != DOA_OK) return rc;
    return doa::calib_mean_host(true, n_items, num_inputs, c_in, nullptr, gain_out, phase_out);
}

// %.9g: nine significant digits identify a float32, so every value parses back to the float it was
int doa_write_phase_config(const char *filename, const float *values, int n)
{
    doa::clear_error();
    if (!filename || n < 0 || (n > 0 && !values)) { doa::set_error("write_phase_config: bad arguments"); return DOA_ERR_INVALID_ARG; }
    FILE *f = fopen(filename, "w");
    if (!f) { doa::set_error("Configuration %s, not writable", filename); return DOA_ERR_INVALID_ARG; }
    bool ok = true;
    for (int i = 0; i < n; i++) ok = ok && fprintf(f, "%.9g\n", (double)values[i]) > 0;
    ok = (fclose(f) == 0) && ok;
    if (!ok) { doa::set_error("Configuration %s, not writable", filename); return DOA_ERR_INVALID_ARG; }
    return DOA_OK;
}

int doa_write_antenna_calib(const char *filename, const float *gains, const float *phases, int n)
{
    doa::clear_error();
    if (!filename || n < 0 || (n > 0 && (!gains || !phases))) { doa::set_error("write_antenna_calib: bad arguments"); return DOA_ERR_INVALID_ARG; }
    FILE *f = fopen(filename, "w");
    if (!f) { doa::set_error("Configuration %s, not valid", filename); return DOA_ERR_INVALID_ARG; }
    bool ok = true;
    for (int i = 0; i < n; i++) ok = ok && fprintf(f, "%.9g %.9g\n", (double)gains[i], (double)phases[i]) > 0;
    ok = (fclose(f) == 0) && ok;
    if (!ok) { doa::set_error("Configuration %s, not valid", filename); return DOA_ERR_INVALID_ARG; }
    return DOA_OK;
}

}  // extern "C"
