"""Measurements of ESPRIT beside Root-MUSIC (profiles/esprit.txt), per 4096 items, everything in one run:

  kernel   doa.esprit_linear_array and doa.rootMUSIC_linear_array on the same device-resident covariance items, shapes
           (N, M) = (4,1), (4,2), (8,2), (8,3), (16,3), (16,15) at 20 and 5 dB, for a `rocprofv3 --kernel-trace` run of its
           own -- kernel times come from the trace, not from this script:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_esprit.py kernel
               python3 tools/profile_esprit.py summarize OUT

           `summarize` splits the trace's eigen / esprit_kernel / root_music_group_kernel dispatches, in order, into the
           configurations `kernel` ran (warm-up dispatches dropped) and prints the median of each.
  step     one root_pipeline.work_dev step, and one work_dev_auto step, at N = 4, K = 1024, batch 4096, M = 2 on the SAME
           handle in Root-MUSIC and in ESPRIT mode, alternating in one process; device events around synchronised blocks
           of steps.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "python"))

D, K_COV, ITEMS = 0.4, 256, 4096
# (N, M) -> source directions (the layouts of tests/esprit_ref.py)
SHAPES = {
    (4, 1): (70.0,), (4, 2): (30.0, 123.0), (8, 2): (50.0, 100.0), (8, 3): (60.0, 75.0, 120.0),
    (16, 3): (40.0, 42.5, 120.0), (16, 15): tuple(25.0 + 9.25 * i for i in range(15)),
}
SNRS = (20.0, 5.0)
ESTIMATORS = ("esprit", "root_music")


def configs():
    return [(N, M, snr) for (N, M) in SHAPES for snr in SNRS]


def run_kernel(a):
    import numpy as np
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()
    out = {"reps": a.reps, "warmup": a.warmup, "items": ITEMS, "configs": []}
    for N, M, snr in configs():
        x = doa.sim.make_streams(N, ITEMS * K_COV, list(SHAPES[(N, M)]), D, snr_db=snr, seed=7)
        streams = [torch.from_numpy(np.ascontiguousarray(x[k])).cuda() for k in range(N)]
        streams = doa.sim.stream_slab_torch(streams)
        R = torch.empty((ITEMS, N * N), dtype=torch.complex64, device="cuda")
        doa.autocorrelate(N, K_COV, 0, 0).work_dev(ITEMS, [s.data_ptr() for s in streams], R.data_ptr(), st)
        ang = torch.empty((ITEMS, M), dtype=torch.float32, device="cuda")
        status = torch.empty((ITEMS,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        row = {"N": N, "M": M, "snr_db": snr}
        for est in ESTIMATORS:
            if est == "esprit":
                blk = doa.esprit_linear_array(D, M, N)
                call = lambda: blk.work_dev(ITEMS, R.data_ptr(), ang.data_ptr(), status.data_ptr(), st)
            else:
                blk = doa.rootMUSIC_linear_array(D, M, N)
                call = lambda: blk.work_dev(ITEMS, R.data_ptr(), ang.data_ptr(), st)
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            row[est + "_us_per_call_events_back_to_back"] = round(e0.elapsed_time(e1) * 1000.0 / a.reps, 2)
            if est == "esprit":
                row["esprit_status_nonzero"] = int((status != 0).sum().item())
                row["esprit_nan_angles"] = int(torch.isnan(ang).sum().item())
        out["configs"].append(row)
    print(json.dumps(out))


def summarize(a):
    rows = []
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                kind = ("esprit" if "esprit_kernel" in name else "root" if "root_music_group_kernel" in name else
                        "evd" if "music_evd" in name else None)
                if kind:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    rows.sort()
    per = 2 * (a.warmup + a.reps)                        # dispatches of one estimator in one configuration: eigen + estimate
    assert len(rows) == 2 * per * len(configs()), (len(rows), per, len(configs()))
    med = lambda v: statistics.median(v) / 1000.0
    print("per %d items, medians of %d dispatches (us): eigen launch | estimate kernel | sum" % (ITEMS, a.reps))
    for k, (N, M, snr) in enumerate(configs()):
        line = "N %2d M %2d %4.0f dB:" % (N, M, snr)
        for e, est in enumerate(ESTIMATORS):
            part = rows[(2 * k + e) * per + 2 * a.warmup:(2 * k + e + 1) * per]
            want = "esprit" if est == "esprit" else "root"
            assert [p[2] for p in part] == ["evd", want] * a.reps, (N, M, snr, est)
            evd = med([t1 - t0 for t0, t1, kind in part if kind == "evd"])
            fin = med([t1 - t0 for t0, t1, kind in part if kind == want])
            line += "   %-10s %8.2f | %8.2f | %8.2f" % (est, evd, fin, evd + fin)
        print(line)


def run_step(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    N, K, M, B = 4, 1024, 2, 4096
    streams, _ = doa.sim.make_batch_streams_torch(N, K, B, 0.5, M, 20.0, seed=7)
    streams = doa.sim.stream_slab_torch(streams)
    ptrs = [s.data_ptr() for s in streams]
    ang = torch.empty((B, M), dtype=torch.float32, device="cuda")
    cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    pipe = doa.root_pipeline(N, K, 0, 0, 0.5, M, max_batch=B)
    st = torch.cuda.current_stream()
    entries = {"work_dev": lambda: pipe.work_dev(B, ptrs, 0, ang.data_ptr(), None, st),
               "work_dev_auto": lambda: pipe.work_dev_auto(B, ptrs, ang.data_ptr(), cnt.data_ptr(), "mdl", None, None, None, st)}
    times = {(e, m): [] for e in entries for m in ("root_music", "esprit")}
    for rnd in range(a.rounds + 1):                     # round 0 warms every setting up
        for entry, call in entries.items():
            for mode in ("root_music", "esprit"):
                pipe.set_estimator(mode)
                for _ in range(a.warmup):
                    call()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[(entry, mode)].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    out = {"shape": {"N": N, "K": K, "M": M, "batch": B}, "steps_per_block": a.steps, "rounds": a.rounds}
    for (entry, mode), t in times.items():
        out[entry + "/" + mode] = {"us_per_step_median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    for entry in entries:
        out[entry + "/esprit_minus_root_music_us_median"] = round(
            statistics.median(times[(entry, "esprit")]) - statistics.median(times[(entry, "root_music")]), 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "summarize", "step"))
    ap.add_argument("dir", nargs="?", help="summarize: the rocprofv3 output directory")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="step: calls per timed block")
    ap.add_argument("--rounds", type=int, default=7, help="step: timed blocks per setting, alternating")
    a = ap.parse_args()
    {"kernel": run_kernel, "summarize": summarize, "step": run_step}[a.mode](a)


if __name__ == "__main__":
    main()
