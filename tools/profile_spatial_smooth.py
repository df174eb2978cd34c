"""Measurements of spatial smoothing (profiles/spatial_smooth.txt):

  kernel   the smoothing kernel alone on device-resident items, shapes N -> S (forward-backward) 4 -> 3, 8 -> 6, 16 -> 12
           at 4096 and 262144 items, for a `rocprofv3 --kernel-trace --stats` run of its own -- kernel times come from the
           trace, not from this script:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_spatial_smooth.py kernel
               python3 tools/profile_spatial_smooth.py summarize OUT

           `summarize` splits the trace's spatial_smooth_kernel dispatches, in order, into the configurations `kernel` ran
           (warm-up dispatches dropped) and prints time and algorithmic bytes n (N^2 + S^2) 8 over time for each.
  step     one music_pipeline.work_dev step at N = 8, K = 1024, P = 1024, M = 2, batch 4096 on the SAME handle with smoothing
           off and on (6, forward-backward), alternating in one process; device events around synchronised blocks of steps.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "python"))

SHAPES = ((4, 3), (8, 6), (16, 12))
BATCHES = (4096, 262144)
KERNEL = "spatial_smooth_kernel"


def configs():
    return [(N, S, n) for N, S in SHAPES for n in BATCHES]


def algorithmic_bytes(N, S, n):
    return n * (N * N + S * S) * 8


def run_kernel(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()
    out = {"reps": a.reps, "warmup": a.warmup, "configs": []}
    for N, S, n in configs():
        g = torch.Generator(device="cuda")
        g.manual_seed(N)
        R = torch.view_as_complex(torch.randn((n, N * N, 2), generator=g, device="cuda", dtype=torch.float32))
        Rs = torch.empty((n, S * S), dtype=torch.complex64, device="cuda")
        blk = doa.spatial_smooth(N, S, True)
        for _ in range(a.warmup):
            blk.work_dev(n, R.data_ptr(), Rs.data_ptr(), st)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            blk.work_dev(n, R.data_ptr(), Rs.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        out["configs"].append({"N": N, "S": S, "items": n, "bytes": algorithmic_bytes(N, S, n),
                               "us_per_call_events_back_to_back": round(e0.elapsed_time(e1) * 1000.0 / a.reps, 2)})
    print(json.dumps(out))


def summarize(a):
    rows = []
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if KERNEL in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    per = a.warmup + a.reps
    assert len(rows) == per * len(configs()), (len(rows), per, len(configs()))
    for k, (N, S, n) in enumerate(configs()):
        ns = [e - s for s, e in rows[k * per + a.warmup:(k + 1) * per]]
        med = statistics.median(ns) / 1000.0
        b = algorithmic_bytes(N, S, n)
        print("N %2d -> S %2d fb 1, %6d items: kernel %8.2f us median (min %.2f, max %.2f; %d dispatches), %6.1f MB algorithmic, "
              "%7.1f GB/s" % (N, S, n, med, min(ns) / 1000.0, max(ns) / 1000.0, len(ns), b / 1e6, b / med / 1e3))


def run_step(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    N, K, P, M, B = 8, 1024, 1024, 2, 4096
    streams, _ = doa.sim.make_batch_streams_torch(N, K, B, 0.5, M, 20.0, seed=7)
    streams = doa.sim.stream_slab_torch(streams)
    ptrs = [s.data_ptr() for s in streams]
    spec = torch.empty((B, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((B, M), dtype=torch.float32, device="cuda")
    am = torch.empty((B, M), dtype=torch.float32, device="cuda")
    pipe = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=B)
    st = torch.cuda.current_stream()
    times = {"off": [], "on": []}
    for rnd in range(a.rounds + 1):                     # round 0 warms both settings up
        for mode in ("off", "on"):
            pipe.set_spatial_smoothing(6 if mode == "on" else 0, 1)
            for _ in range(a.warmup):
                pipe.work_dev(B, ptrs, 0, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                pipe.work_dev(B, ptrs, 0, spec.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[mode].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    out = {"shape": {"N": N, "K": K, "P": P, "M": M, "batch": B, "S": 6, "fb": 1}, "steps_per_block": a.steps, "rounds": a.rounds}
    for mode, t in times.items():
        out[mode] = {"us_per_step_median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    out["on_minus_off_us_median"] = round(statistics.median(times["on"]) - statistics.median(times["off"]), 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "summarize", "step"))
    ap.add_argument("dir", nargs="?", help="summarize: the rocprofv3 output directory")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="step: work_dev calls per timed block")
    ap.add_argument("--rounds", type=int, default=7, help="step: timed blocks per setting, alternating")
    a = ap.parse_args()
    {"kernel": run_kernel, "summarize": summarize, "step": run_step}[a.mode](a)


if __name__ == "__main__":
    main()
