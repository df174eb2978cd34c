"""Measurements of Root-MUSIC with a count per item (profiles/root_counts.txt):

  kernel   rootMUSIC_linear_array on device-resident covariance items, 4096 per launch, at N = 4, M = 2 and N = 16, M = 3:
           the fixed entry (work_dev), the counted entry with uniform counts = M, the counted entry with counts cycling
           0 .. M, and the fixed entry again (the spread of two runs of the same kernel), for a
           `rocprofv3 --kernel-trace --stats` run of its own -- kernel times come from the trace, not from this script:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_root_counts.py kernel
               python3 tools/profile_root_counts.py summarize OUT

           `summarize` splits the trace's root_music_group_kernel dispatches, in order, into the configurations `kernel` ran
           (warm-up dispatches dropped) and checks that the fixed / counted instantiation ran where it should.
  step     one root_pipeline step at N = 4, K = 1024, batch 4096, two sources: work_dev of a num_targets = 2 handle against
           work_dev_auto (MDL) of a num_targets = 3 handle, alternating in one process; device events around synchronised
           blocks of steps.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "python"))

SHAPES = ((4, 2), (16, 3))
MODES = ("fixed", "uniform", "cycling", "fixed_again")
ITEMS, K, D = 4096, 256, 0.5
KERNEL = "root_music_group_kernel"


def configs():
    return [(N, M, mode) for N, M in SHAPES for mode in MODES]


def _covariances(N, M):
    import torch
    import doa
    streams, _ = doa.sim.make_batch_streams_torch(N, K, ITEMS, D, M, 15.0, seed=5)
    streams = doa.sim.stream_slab_torch(streams)
    R = torch.empty((ITEMS, N * N), dtype=torch.complex64, device="cuda")
    doa.autocorrelate(N, K, 0, 0).work_dev(ITEMS, [s.data_ptr() for s in streams], R.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return R


def run_kernel(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()
    for N, M in SHAPES:
        R = _covariances(N, M)
        blk = doa.rootMUSIC_linear_array(D, M, N)
        out = torch.empty((ITEMS, M), dtype=torch.float32, device="cuda")
        status = torch.empty((ITEMS,), dtype=torch.int32, device="cuda")
        counts = {"uniform": torch.full((ITEMS,), M, dtype=torch.int32, device="cuda"),
                  "cycling": (torch.arange(ITEMS, device="cuda") % (M + 1)).to(torch.int32)}
        for mode in MODES:
            for _ in range(a.warmup + a.reps):
                if mode in counts:
                    blk.work_dev_counts(ITEMS, R.data_ptr(), counts[mode].data_ptr(), out.data_ptr(), status.data_ptr(), st)
                else:
                    blk.work_dev(ITEMS, R.data_ptr(), out.data_ptr(), st)
            torch.cuda.synchronize()
    print(json.dumps({"reps": a.reps, "warmup": a.warmup, "items": ITEMS, "configs": [list(c) for c in configs()]}))


def summarize(a):
    rows = []
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if KERNEL in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "RootCounts" in r["Kernel_Name"]))
    rows.sort()
    per = a.warmup + a.reps
    assert len(rows) == per * len(configs()), (len(rows), per, len(configs()))
    base = {}
    for k, (N, M, mode) in enumerate(configs()):
        mine = rows[k * per + a.warmup:(k + 1) * per]
        assert all(counted == (mode in ("uniform", "cycling")) for _, _, counted in mine), (N, M, mode)
        ns = [e - s for s, e, _ in mine]
        med = statistics.median(ns) / 1000.0
        base.setdefault((N, M), med)
        print("N %2d M %d %-11s: root kernel %7.2f us median (min %.2f, max %.2f; %d dispatches of %d items), %.3f x the first "
              "fixed run" % (N, M, mode, med, min(ns) / 1000.0, max(ns) / 1000.0, len(ns), ITEMS, med / base[(N, M)]))


def run_step(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    N, Ks, B, M = 4, 1024, 4096, 2
    streams, _ = doa.sim.make_batch_streams_torch(N, Ks, B, D, M, 20.0, seed=7)
    streams = doa.sim.stream_slab_torch(streams)
    ptrs = [s.data_ptr() for s in streams]
    W = 3
    ang = torch.empty((B, W), dtype=torch.float32, device="cuda")
    cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    fixed = doa.root_pipeline(N, Ks, 0, 0, D, M, max_batch=B)
    auto = doa.root_pipeline(N, Ks, 0, 0, D, W, max_batch=B)
    st = torch.cuda.current_stream()
    calls = {"work_dev": lambda: fixed.work_dev(B, ptrs, 0, ang.data_ptr(), None, st),
             "work_dev_auto": lambda: auto.work_dev_auto(B, ptrs, ang.data_ptr(), cnt.data_ptr(), "mdl", stream=st)}
    times = {k: [] for k in calls}
    for rnd in range(a.rounds + 1):                     # round 0 warms both up
        for mode, call in calls.items():
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
                times[mode].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    out = {"shape": {"N": N, "K": Ks, "batch": B, "sources": M, "auto_num_targets": W}, "steps_per_block": a.steps, "rounds": a.rounds,
           "counts_seen": sorted(set(cnt.cpu().tolist()))}
    for mode, t in times.items():
        out[mode] = {"us_per_step_median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    out["auto_minus_fixed_us_median"] = round(statistics.median(times["work_dev_auto"]) - statistics.median(times["work_dev"]), 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "summarize", "step"))
    ap.add_argument("dir", nargs="?", help="summarize: the rocprofv3 output directory")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="step: calls per timed block")
    ap.add_argument("--rounds", type=int, default=7, help="step: timed blocks per entry, alternating")
    a = ap.parse_args()
    {"kernel": run_kernel, "summarize": summarize, "step": run_step}[a.mode](a)


if __name__ == "__main__":
    main()
