// gr::doa::music_pipeline_sc16 — gr::doa::music_pipeline on complex int16 streams (sc16 items, 4 bytes: int16 real, int16
// imaginary), widened on the device as float(q) * scale (doa_music_pipeline_set_input_format, include/doa_hip.h).  Ports,
// history and scheduling as gr::doa::music_pipeline except the input item size; every output is bit for bit what
// gr::doa::music_pipeline gives on the widened samples.  Half the bytes of the fc32 block cross PCIe per snapshot.
// With calibrated arrays the gains are folded into the block (doa_music_pipeline_fuse_antenna_correction): a standalone
// antenna_correction block in front would emit gr_complex again.
#pragma once
#include <doa/api.h>

namespace gr {
namespace doa {

class DOA_API music_pipeline_sc16 : virtual public gr::block
{
public:
    typedef DOA_SPTR<music_pipeline_sc16> sptr;
    static sptr make(int inputs, int snapshot_size, int overlap_size, int avg_method, float norm_spacing, int num_targets,
                     int pspectrum_len, float scale);

    // as gr::doa::music_pipeline::work_device_batches; d_input_items point at sc16 data on the device (4-byte aligned)
    virtual int work_device_batches(int n_batches, int noutput_items, const void *const *d_input_items,
                                    void *const *d_spectrum_out, void *const *d_max_out, void *const *d_argmax_out,
                                    void *hip_stream) = 0;
    virtual int synchronize_device() = 0;
    virtual int max_batch() const = 0;
};

}  // namespace doa
}  // namespace gr
