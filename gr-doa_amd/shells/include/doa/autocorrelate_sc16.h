// gr::doa::autocorrelate_sc16 — gr::doa::autocorrelate on complex int16 streams (GNU Radio's sc16 items: int16 real,
// int16 imaginary, 4 bytes; what a UHD source hands over unconverted).  Not a block of the reference: GNU Radio's own
// convention for a second item type is a second block (add_cc / add_ss).  The samples are widened on the device as
// float(q) * scale (doa_autocorrelate_set_input_format, include/doa_hip.h); the output items are bit for bit those of
// gr::doa::autocorrelate fed the widened samples.
#pragma once
#include <doa/api.h>

namespace gr {
namespace doa {

// N sc16 streams in, one stream of column-major N x N gr_complex sample-covariance matrices out; history, forecast and
// consume_each as gr::doa::autocorrelate.
class DOA_API autocorrelate_sc16 : virtual public gr::block
{
public:
    typedef DOA_SPTR<autocorrelate_sc16> sptr;
    static sptr make(int inputs, int snapshot_size, int overlap_size, int avg_method, float scale);
};

}  // namespace doa
}  // namespace gr
