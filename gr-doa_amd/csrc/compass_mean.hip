// compass_mean.hip — the consumer side of the hot path: the per-call average the
// reference's `compass` sink displays, taken on the device so that the per-snapshot angles need not
// cross PCIe at all.
//
// Replaces, as a unit, blocks.vector_to_streams(gr.sizeof_float, num_targets)
// (apps/run_MUSIC_lin_array_simulation.py:199, connections :236-239: port 1 of find_local_max, item =
// num_targets floats, de-interleaved into num_targets float streams) followed by one doa.compass per
// stream, whose work() is `self.next_angle = numpy.mean(input_items[0])` over the items of the call
// (python/compass.py:134-136).  The Qt dial/LCD of the compass is GUI and out of scope.
//
//   next_angle[m] = mean_i in[i * num_streams + m],  i = 0 .. ninput_items-1
//
// numpy.mean of a float32 array accumulates pairwise in float32; here the sum is carried in double
// and rounded once, so the result is the correctly rounded mean (numpy's differs from it by <= a few
// ulp).  ninput_items == 0 gives NaN, as numpy.mean of an empty array does.
#include "block_host.hpp"
#include "kernels.hpp"

#include <cmath>

namespace doa {

__global__ __launch_bounds__(256) void compass_mean_kernel(const float *__restrict__ in, float *__restrict__ out, int n, int M)
{
    __shared__ double part[256];
    const int m = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)in[(size_t)i * M + m];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {          // fixed tree: the result does not depend on scheduling
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[m] = (n > 0) ? (float)(part[0] / (double)n) : nanf("");
}

}  // namespace doa

struct doa_compass_mean : doa::BlockBase {
    int M = 0;
    doa::DevBuf d_in, d_out;
};

extern "C" {

doa_compass_mean_t *doa_compass_mean_create(int num_streams)
{
    doa::clear_error();
    if (num_streams <= 0 || num_streams > DOA_MAX_PEAKS) {
        doa::set_error("compass_mean: num_streams=%d outside 1..%d", num_streams, DOA_MAX_PEAKS);
        return nullptr;
    }
    return doa::create_block<doa_compass_mean>("compass_mean", [&](doa_compass_mean &h) { h.M = num_streams; return (int)DOA_OK; });
}

void doa_compass_mean_destroy(doa_compass_mean_t *h) { doa::destroy_block(h); }

// Zero items is a call like any other: the kernel runs and writes NaN.  next_angle is therefore required then too, which
// work_args does not ask of its pointer list: without it the call is refused as one without a handle is.
int doa_compass_mean_work_dev(doa_compass_mean_t *h, int ninput_items, const void *d_input_items0, float *d_next_angle,
                              void *hip_stream)
{
    doa::clear_error();
    if (int rc = doa::work_args("compass_mean_work_dev", d_next_angle ? h : nullptr, ninput_items, {d_input_items0}); rc != DOA_OK) return rc;
    if (int brc = doa::bind_device(h->device); brc != DOA_OK) return brc;
    hipLaunchKernelGGL(doa::compass_mean_kernel, dim3(h->M), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                       static_cast<const float *>(d_input_items0), d_next_angle, ninput_items, h->M);
    DOA_HIP_TRY(hipGetLastError());
    return ninput_items;          // "consume all inputs" (python/compass.py:143-144)
}

int doa_compass_mean_work(doa_compass_mean_t *h, int ninput_items, const void *input_items0, float *next_angle)
{
    doa::clear_error();
    if (int rc = doa::work_args("compass_mean_work", next_angle ? h : nullptr, ninput_items, {input_items0}); rc != DOA_OK) return rc;
    doa::HostCall io(*h);
    if (ninput_items > 0) io.in(h->d_in, input_items0, (size_t)ninput_items * h->M * sizeof(float));
    int rc = io.out(h->d_out, next_angle, h->M * sizeof(float));
    if (rc == DOA_OK) rc = doa_compass_mean_work_dev(h, ninput_items, h->d_in.p, h->d_out.as<float>(), h->stream);
    return io.finish(rc);
}

}  // extern "C"
