// wave_ops_debug.hip — doa_hip_wave_ops_debug (include/doa_hip_test.h): each primitive of wave_ops.hpp applied to a supplied
// input by one workgroup of four waves, for tests/test_gpu_wave_ops.py.  The only kernels of this unit are the test's.
#include "kernels.hpp"
#include "wave_ops.hpp"

namespace {
using namespace doa;

constexpr int kThreads = 256;                            // one workgroup: four waves, so that wave_index() has something to tell apart
struct ValIdx { float v; int i; };                       // wave_argbest's element

// out[t] = what thread t holds after f(in, t); F reads its inputs itself (one element per thread, or two for the DPP move)
template <class T, class F> __global__ __launch_bounds__(kThreads) void wave_ops_kernel(const T *__restrict__ in, T *__restrict__ out, F f)
{
    out[threadIdx.x] = f(in, (int)threadIdx.x);
}

template <class T, class F> int run(const void *in, void *out, int n_in, F f)
{
    DevBuf d_in, d_out;
    if (int rc = d_in.reserve((size_t)n_in * sizeof(T)); rc != DOA_OK) return rc;
    if (int rc = d_out.reserve((size_t)kThreads * sizeof(T)); rc != DOA_OK) return rc;
    DOA_HIP_TRY(hipMemcpy(d_in.p, in, (size_t)n_in * sizeof(T), hipMemcpyHostToDevice));
    wave_ops_kernel<T><<<1, kThreads>>>(d_in.as<T>(), d_out.as<T>(), f);
    DOA_HIP_TRY(hipGetLastError());
    DOA_HIP_TRY(hipMemcpy(out, d_out.p, (size_t)kThreads * sizeof(T), hipMemcpyDeviceToHost));
    return kThreads;
}
// f(v, lane) on in[t]
template <class T, class F> int each(const void *in, void *out, F f)
{
    return run<T>(in, out, kThreads, [f] __device__(const T *x, int t) { return f(x[t], t & (kWave - 1)); });
}

// the DPP move: v = in[t], old = in[256 + t]
template <class T, int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF> int move(const void *in, void *out)
{
    return run<T>(in, out, 2 * kThreads, [] __device__(const T *x, int t) { return dpp<CTRL, ROW_MASK, BANK_MASK>(x[kThreads + t], x[t]); });
}
template <class T> int move_op(int c, const void *in, void *out)
{
    switch (c) {
    case 0: return move<T, kQuadXor1>(in, out);
    case 1: return move<T, kQuadXor2>(in, out);
    case 2: return move<T, row_shl<2>>(in, out);
    case 3: return move<T, row_shr<2>>(in, out);
    case 4: return move<T, row_shr<2>, 0xF, 0x1>(in, out);       // the block-16 caterpillar's second shift
    case 5: return move<T, kRowBcast15, 0xA>(in, out);           // steps five and six of the wave schedule
    case 6: return move<T, kRowBcast31, 0xC>(in, out);
    case 7: return move<T, kQuadXor1, 0x5, 0x6>(in, out);        // a row mask and a bank mask together
    case 11: return move<T, row_ror<1>>(in, out);
    case 12: return move<T, row_ror<2>>(in, out);
    case 13: return move<T, row_ror<3>>(in, out);
    case 14: return move<T, row_ror<4>>(in, out);
    case 15: return move<T, row_ror<5>>(in, out);
    case 16: return move<T, row_ror<6>>(in, out);
    case 17: return move<T, row_ror<7>>(in, out);
    case 18: return move<T, row_ror<8>>(in, out);
    case 19: return move<T, row_ror<9>>(in, out);
    case 20: return move<T, row_ror<10>>(in, out);
    case 21: return move<T, row_ror<11>>(in, out);
    case 22: return move<T, row_ror<12>>(in, out);
    case 23: return move<T, row_ror<13>>(in, out);
    case 24: return move<T, row_ror<14>>(in, out);
    case 25: return move<T, row_ror<15>>(in, out);
    default: return DOA_ERR_INVALID_ARG;
    }
}

template <int G> int group_op(int kind, const void *in, void *out)
{
    switch (kind) {
    case 0: return each<double>(in, out, [] __device__(double v, int lane) { return group_sum<G, double>(v, lane); });
    case 1: return each<float>(in, out, [] __device__(float v, int lane) { return group_sum<G, float>(v, lane); });
    case 2: return each<double>(in, out, [] __device__(double v, int lane) { return group_max<G, double>(v, lane); });
    case 3: return each<int>(in, out, [] __device__(int v, int lane) { return group_or<G>(v, lane); });
    default: return DOA_ERR_INVALID_ARG;
    }
}

int dispatch(int op, const void *in, void *out)
{
    if (op >= 1000 && op < 1300) {
        const int c = op % 100;
        return op < 1100 ? move_op<int>(c, in, out) : (op < 1200 ? move_op<float>(c, in, out) : move_op<double>(c, in, out));
    }
    if (op >= 10 && op < 50) {
        const int kind = op / 10 - 1;
        return op % 10 == 0 ? group_op<4>(kind, in, out) : (op % 10 == 1 ? group_op<8>(kind, in, out) : (op % 10 == 2 ? group_op<16>(kind, in, out) : DOA_ERR_INVALID_ARG));
    }
    switch (op) {
    case 0: return each<int>(in, out, [] __device__(int, int) { return wave_index(); });
    case 51: return each<double>(in, out, [] __device__(double v, int) { return quad_rot<1>(v); });
    case 52: return each<double>(in, out, [] __device__(double v, int) { return quad_rot<2>(v); });
    case 53: return each<double>(in, out, [] __device__(double v, int) { return quad_rot<3>(v); });
    case 54: return each<double>(in, out, [] __device__(double v, int) { return quad_sum(v); });
    case 55: return each<double>(in, out, [] __device__(double v, int) { return row_sum16(v); });
    case 60: return each<float>(in, out, [] __device__(float v, int) { return wave_allreduce_sum(v); });
    case 61: return each<int>(in, out, [] __device__(int v, int) { return wave_allreduce_sum(v); });
    case 62: return each<float>(in, out, [] __device__(float v, int) { return wave_allreduce_max(v); });
    case 63: return each<float>(in, out, [] __device__(float v, int) { return wave_allreduce_min(v); });
    case 64: return each<int>(in, out, [] __device__(int v, int) { return wave_allreduce_min_int(v); });
    case 65: return each<ValIdx>(in, out, [] __device__(ValIdx x, int) { wave_argbest(x.v, x.i); return x; });
    case 70: return each<float>(in, out, [] __device__(float v, int) { return wave_butterfly_sum_fetch<float>(v); });
    case 71: return each<double>(in, out, [] __device__(double v, int) { return wave_butterfly_sum_fetch<double>(v); });
    case 72: return each<double>(in, out, [] __device__(double v, int) { return wave_butterfly_sum_xor<double>(v); });
    case 73: return each<float>(in, out, [] __device__(float v, int) { return wave_butterfly_nan_max(v); });
    default: return DOA_ERR_INVALID_ARG;
    }
}
}  // namespace

extern "C" {

int doa_hip_wave_ops_debug(int op, int n, const void *in, void *out)
{
    doa::clear_error();
    const int want = (op >= 1000) ? 2 * kThreads : kThreads;
    if (n != want || !in || !out) {
        doa::set_error("hip_wave_ops_debug: op %d takes n = %d input elements, in and out (got n = %d)", op, want, n);
        return DOA_ERR_INVALID_ARG;
    }
    int device;
    if (int rc = doa::ensure_device(&device); rc != DOA_OK) return rc;
    const int rc = dispatch(op, in, out);
    if (rc == DOA_ERR_INVALID_ARG) doa::set_error("hip_wave_ops_debug: no op %d", op);
    return rc;
}

}  // extern "C"
