// run_flowgraph_sc16 — the sc16 block shells wired as the fc32 ones are in run_flowgraph, fed complex int16 stream files:
//     N stream files -> autocorrelate_sc16                                     (mode "autocorrelate")
//     N stream files -> music_pipeline_sc16                                    (mode "pipeline")
//     N stream files -> root_music_pipeline_sc16                               (mode "root_pipeline")
// Inputs/outputs are raw little-endian binary files so that the pytest driver (tests/test_gpu_sc16_shells.py) can compare
// every port with the Python binding and with run_flowgraph fed the widened samples.
//
// usage: run_flowgraph_sc16 autocorrelate|pipeline|root_pipeline <in_prefix> <out_prefix> inputs snapshot overlap avg
//                           norm_spacing num_targets pspectrum_len max_noutput scale
//   reads  <in_prefix>.ch<k>.sc16   (int16 real, int16 imaginary per sample of stream k, no history)
//   writes <out_prefix>.cov.c64                                   (autocorrelate)
//          <out_prefix>.spec.f32, .max.f32, .argmax.f32           (pipeline)
//          <out_prefix>.aoa.f32                                   (root_pipeline)
// and prints the wall time spent inside the blocks' work() calls (host buffers in, host buffers out).
#include <doa/autocorrelate_sc16.h>
#include <doa/music_pipeline_sc16.h>
#include <doa/root_music_pipeline_sc16.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

using gr::lite::port_data;

static port_data read_file(const std::string &path, size_t item_size)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    port_data d;
    d.item_size = item_size;
    d.bytes.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return d;
}
static void write_file(const std::string &path, const port_data &d)
{
    std::ofstream f(path, std::ios::binary);
    f.write(d.bytes.data(), (std::streamsize)d.bytes.size());
}

int main(int argc, char **argv)
{
    if (argc != 13) {
        std::cerr << "usage: run_flowgraph_sc16 autocorrelate|pipeline|root_pipeline in_prefix out_prefix inputs snapshot overlap "
                     "avg norm_spacing num_targets pspectrum_len max_noutput scale\n";
        return 2;
    }
    const std::string mode = argv[1], in_prefix = argv[2], out_prefix = argv[3];
    const int inputs = atoi(argv[4]), snapshot = atoi(argv[5]), overlap = atoi(argv[6]), avg = atoi(argv[7]);
    const float d = (float)atof(argv[8]);
    const int M = atoi(argv[9]), P = atoi(argv[10]), max_noutput = atoi(argv[11]);
    const float scale = strtof(argv[12], nullptr);
    try {
        std::vector<port_data> streams;
        for (int k = 0; k < inputs; k++)
            streams.push_back(read_file(in_prefix + ".ch" + std::to_string(k) + ".sc16", 2 * sizeof(int16_t)));

        double work_s = 0.0;
        if (mode == "autocorrelate") {
            auto ac = gr::doa::autocorrelate_sc16::make(inputs, snapshot, overlap, avg, scale);
            auto cov = gr::lite::run_block(*ac, streams, 1, max_noutput, &work_s);
            write_file(out_prefix + ".cov.c64", cov[0]);
            std::cout << "items: cov " << cov[0].items() << "\nwork_seconds " << work_s << std::endl;
            return 0;
        }
        if (mode == "pipeline") {
            auto pipe = gr::doa::music_pipeline_sc16::make(inputs, snapshot, overlap, avg, d, M, P, scale);
            auto out = gr::lite::run_block(*pipe, streams, 3, max_noutput);      // first pass: code load, buffer allocation
            write_file(out_prefix + ".argmax.f32", out[0]);
            write_file(out_prefix + ".max.f32", out[1]);
            write_file(out_prefix + ".spec.f32", out[2]);
            auto again = gr::lite::run_block(*pipe, streams, 3, max_noutput, &work_s);   // timed: the same stream once more
            if (again[0].bytes != out[0].bytes || again[2].bytes != out[2].bytes) throw std::runtime_error("music_pipeline_sc16: second pass differs");
            std::cout << "items: peaks " << out[0].items() << " spec " << out[2].items() << "\nwork_seconds " << work_s
                      << " snapshots_per_s " << (work_s > 0 ? out[0].items() / work_s : 0.0) << std::endl;
            // the same block with only port 0 connected (angles out)
            auto pipe1 = gr::doa::music_pipeline_sc16::make(inputs, snapshot, overlap, avg, d, M, P, scale);
            double w1 = 0.0;
            auto out1 = gr::lite::run_block(*pipe1, streams, 1, max_noutput);
            out1 = gr::lite::run_block(*pipe1, streams, 1, max_noutput, &w1);
            if (out1[0].bytes != out[0].bytes) throw std::runtime_error("music_pipeline_sc16: port 0 differs with ports 1, 2 unconnected");
            std::cout << "angles_only work_seconds " << w1 << " snapshots_per_s " << (w1 > 0 ? out1[0].items() / w1 : 0.0) << std::endl;
            return 0;
        }
        if (mode == "root_pipeline") {
            auto pipe = gr::doa::root_music_pipeline_sc16::make(inputs, snapshot, overlap, avg, d, M, scale);
            auto out = gr::lite::run_block(*pipe, streams, 1, max_noutput);
            write_file(out_prefix + ".aoa.f32", out[0]);
            auto again = gr::lite::run_block(*pipe, streams, 1, max_noutput, &work_s);
            if (again[0].bytes != out[0].bytes) throw std::runtime_error("root_music_pipeline_sc16: second pass differs");
            std::cout << "items: aoa " << out[0].items() << "\nwork_seconds " << work_s << " snapshots_per_s "
                      << (work_s > 0 ? out[0].items() / work_s : 0.0) << std::endl;
            return 0;
        }
        std::cerr << "run_flowgraph_sc16: unknown mode " << mode << std::endl;
        return 2;
    } catch (const std::exception &e) {
        std::cerr << "run_flowgraph_sc16: " << e.what() << std::endl;
        return 1;
    }
}
