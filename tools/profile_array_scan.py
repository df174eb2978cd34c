"""Measurements of the steering-table scan (profiles/array_scan.txt):

  kernel   doa.MUSIC_array.work_dev and, on the same items, doa.MUSIC_lin_array.work_dev with a ULA table, shapes
           (N, P, items) = (4, 1024, 4096), (8, 1024, 4096), (16, 4096, 4096), (4, 1024, 262144), for a
           `rocprofv3 --kernel-trace --stats` run of its own -- kernel times come from the trace, not from this script:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_array_scan.py kernel
               python3 tools/profile_array_scan.py summarize OUT

           `summarize` splits the trace's array_scan_kernel dispatches and the ULA scan kernels' dispatches, in order, into
           the shapes `kernel` ran (warm-up dispatches dropped) and prints each median beside the floor of the shape -- the
           larger of 4 P items bytes at the project's measured copy rate (6.29 TB/s) and N^2 P items double
           FMAs at the fp64 rate of profiles/r03_lab_valu_rates.txt (v_fma_f64 at four waves per SIMD: 2.83 SIMD cycles per
           instruction at 1.84 GHz, 1024 SIMDs) -- and beside the ULA scan at the same shape.
  step     one music_pipeline.work_dev step at N = 4, K = 1024, P = 1024, M = 1, batch 4096 on the SAME handle with and
           without a (ULA) steering table, alternating in one process; device events around synchronised blocks of steps.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "python"))

SHAPES = ((4, 1024, 4096), (8, 1024, 4096), (16, 4096, 4096), (4, 1024, 262144))
KERNEL = "array_scan_kernel"
ULA_KERNEL = "music_scan"
COPY_RATE = 6.29e12                                     # bytes per second
FMA_RATE = 1024 * 64 / 2.83 * 1.84e9                    # double FMAs per second


def floors_us(N, P, n):
    return 4.0 * P * n / COPY_RATE * 1e6, float(N) * N * P * n / FMA_RATE * 1e6


def ula_table(N, P, d=0.5):
    """[P, N] complex128: a ULA over 0..180 degrees (the geometry of MUSIC_lin_array; its float-accumulated grid is not replayed)."""
    import doa
    xy = np.stack([d * (np.arange(N) - (N - 1) / 2.0), np.zeros(N)], axis=1)
    return doa.planar_steering_table(xy, P, 0.0, 180.0)


def run_kernel(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()
    out = {"reps": a.reps, "warmup": a.warmup, "shapes": []}
    for N, P, n in SHAPES:
        M = 1 if N <= 4 else 2
        streams, _ = doa.sim.make_batch_streams_torch(N, 64, n, 0.5, M, 20.0, seed=7)
        ptrs = [s.data_ptr() for s in doa.sim.stream_slab_torch(streams)]
        cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
        doa.autocorrelate(N, 64, 0, 0).work_dev(n, ptrs, cov.data_ptr(), st)
        spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
        for blk in (doa.MUSIC_array(M, ula_table(N, P)), doa.MUSIC_lin_array(0.5, M, N, P)):
            for _ in range(a.warmup + a.reps):
                blk.work_dev(n, cov.data_ptr(), spec.data_ptr(), st)
            torch.cuda.synchronize()
        out["shapes"].append({"N": N, "P": P, "items": n, "M": M})
    print(json.dumps(out))


def summarize(a):
    mine, ula = [], []
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                row = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
                if KERNEL in r["Kernel_Name"]:
                    mine.append(row)
                elif ULA_KERNEL in r["Kernel_Name"]:
                    ula.append(row)
    mine.sort(); ula.sort()
    per = a.warmup + a.reps
    assert len(mine) == per * len(SHAPES), (len(mine), per)
    for k, (N, P, n) in enumerate(SHAPES):
        t = [e - s for s, e in mine[k * per + a.warmup:(k + 1) * per]]
        # the ULA scan's dispatches of this shape lie between this shape's last array_scan_kernel and the next shape's first
        lo = mine[(k + 1) * per - 1][1]
        hi = mine[(k + 1) * per][0] if k + 1 < len(SHAPES) else float("inf")
        u = [e - s for s, e in ula if lo <= s < hi]
        assert u and len(u) % per == 0, (len(u), per)
        per_call = len(u) // per                         # launches per work_dev call (1 on every shape measured so far)
        calls = [sum(u[c * per_call:(c + 1) * per_call]) for c in range(a.warmup, per)]
        med, umed = statistics.median(t) / 1000.0, statistics.median(calls) / 1000.0
        store, fma = floors_us(N, P, n)
        floor = max(store, fma)
        print("N %2d P %4d, %6d items: array_scan_kernel %9.2f us median (min %.2f, max %.2f; %d dispatches); floor %8.2f us "
              "(store %.2f, fp64 %.2f: %s-bound) -> %.2f x floor; ULA scan %8.2f us (%d launch per call) -> %.2f x the ULA scan"
              % (N, P, n, med, min(t) / 1000.0, max(t) / 1000.0, len(t), floor, store, fma, "store" if store >= fma else "fp64",
                 med / floor, umed, per_call, med / umed))


def run_step(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    N, K, P, M, B = 4, 1024, 1024, 1, 4096
    streams, _ = doa.sim.make_batch_streams_torch(N, K, B, 0.5, M, 20.0, seed=7)
    streams = doa.sim.stream_slab_torch(streams)
    ptrs = [s.data_ptr() for s in streams]
    spec = torch.empty((B, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((B, M), dtype=torch.float32, device="cuda")
    am = torch.empty((B, M), dtype=torch.float32, device="cuda")
    pipe = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=B)
    table = ula_table(N, P)
    st = torch.cuda.current_stream()
    times = {"ula": [], "table": []}
    for rnd in range(a.rounds + 1):                     # round 0 warms both settings up
        for mode in ("ula", "table"):
            pipe.set_steering_table(table if mode == "table" else None, 0.0, 180.0)
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
    out = {"shape": {"N": N, "K": K, "P": P, "M": M, "batch": B}, "steps_per_block": a.steps, "rounds": a.rounds}
    for mode, t in times.items():
        out[mode] = {"us_per_step_median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    out["table_minus_ula_us_median"] = round(statistics.median(times["table"]) - statistics.median(times["ula"]), 2)
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
