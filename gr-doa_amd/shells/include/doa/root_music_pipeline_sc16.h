// gr::doa::root_music_pipeline_sc16 — gr::doa::root_music_pipeline on complex int16 streams (sc16 items, 4 bytes), widened
// on the device as float(q) * scale (doa_root_pipeline_set_input_format, include/doa_hip.h).  Ports, history and
// scheduling as gr::doa::root_music_pipeline except the input item size; the angles are bit for bit those of
// gr::doa::root_music_pipeline on the widened samples.
#pragma once
#include <doa/api.h>

namespace gr {
namespace doa {

class DOA_API root_music_pipeline_sc16 : virtual public gr::block
{
public:
    typedef DOA_SPTR<root_music_pipeline_sc16> sptr;
    static sptr make(int inputs, int snapshot_size, int overlap_size, int avg_method, float norm_spacing, int num_targets,
                     float scale);

    // as gr::doa::root_music_pipeline::work_device_batches; d_input_items point at sc16 data on the device (4-byte aligned)
    virtual int work_device_batches(int n_batches, int noutput_items, const void *const *d_input_items, void *const *d_angles_out,
                                    int *const *d_status_out, void *hip_stream) = 0;
    virtual int synchronize_device() = 0;
    virtual int max_batch() const = 0;
};

}  // namespace doa
}  // namespace gr
