"""The fused phase-offset estimator and K1 on the same device-resident streams, back to back, for a
`rocprofv3 --kernel-trace --stats` run of its own (kernel times come from the trace, not from this script):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_phase_offset_est.py

N streams of 2^log2n samples, fc32 and sc16 (the fc32 streams quantised at scale 2^-12).  Per repetition: one
twinrx_phase_offset_est.estimate_dev (poe_partial_kernel + poe_combine_kernel) and one autocorrelate.work_dev over the same
bytes (K = 4096, no overlap: cov_wave_kernel), each format.  K1 is the yardstick: same bytes, same loads.
Prints the bytes each kernel reads per launch and, with --events, HIP-event times of its own as a cross-check."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4)
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--events", action="store_true")
    a = ap.parse_args()
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    N, n, K = a.N, 1 << a.log2n, 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    tone = torch.exp(2j * torch.pi * ((0.0137 * t) % 1.0))
    fc, sc = [], []
    for k in range(N):
        noise = 0.1 * torch.complex(torch.randn(n, generator=g, device="cuda", dtype=torch.float64),
                                    torch.randn(n, generator=g, device="cuda", dtype=torch.float64))
        x = (tone * complex(torch.exp(torch.tensor(-0.7j * k))) + noise).to(torch.complex64)
        fc.append(x)
        sc.append(doa.sim.to_sc16(x, 2.0 ** -12))
    del tone, t
    fc, sc = doa.sim.stream_slab_torch(fc), doa.sim.stream_slab_torch(sc)
    res = torch.empty((3, N - 1), dtype=torch.float32, device="cuda")
    cov = torch.empty((n // K, N * N), dtype=torch.complex64, device="cuda")
    st = torch.cuda.current_stream()
    runs = {}
    for fmt, streams in (("fc32", fc), ("sc16", sc)):
        est = doa.twinrx_phase_offset_est(N, 0)
        ac = doa.autocorrelate(N, K, 0, 0)
        if fmt == "sc16":
            est.set_input_format("sc16", 2.0 ** -12)
            ac.set_input_format("sc16", 2.0 ** -12)
        ptrs = [s.data_ptr() for s in streams]
        runs[fmt] = (lambda est=est, ptrs=ptrs: est.estimate_dev(n, ptrs, n, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), st),
                     lambda ac=ac, ptrs=ptrs: ac.work_dev(n // K, ptrs, cov.data_ptr(), st))
    out = {"N": N, "samples_per_stream": n, "bytes_fc32": N * n * 8, "bytes_sc16": N * n * 4, "reps": a.reps}
    for fmt, (f_est, f_cov) in runs.items():
        for name, fn in (("estimate", f_est), ("k1", f_cov)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if a.events:
                out[f"{fmt}_{name}_us_per_call_events"] = round(e0.elapsed_time(e1) * 1000.0 / a.reps, 2)
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
