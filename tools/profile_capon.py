"""Measurements of the Capon estimator (profiles/capon.txt):

  kernel   per 4096 covariance items (two sources, K = 256) at N = 4, 8, 16 and at 20 dB and 0 dB, the three launches that
           can stand between K1 and the scan, each on device-resident items through its block's work_dev:
             capon     capon_inverse_kernel                          (doa.capon_lin_array.work_dev)
             jacobi    the fixed-count Jacobi eigen launch           (doa.MUSIC_lin_array.work_dev_counts, forced counts:
                       data-independent up to the sweep count; one lane per item for N <= 4, 8 lanes for N <= 8, the
                       one-wave-per-item block Jacobi for N <= 16)
             default   the default eigen launch of launch_music_evd  (doa.MUSIC_lin_array.work_dev)
           for a `rocprofv3 --kernel-trace --stats` run of its own -- kernel times come from the trace, not from this script:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_capon.py kernel
               python3 tools/profile_capon.py summarize OUT

           `summarize` splits the trace's dispatches of each of the three kernel families, in order, into the configurations
           `kernel` ran (warm-up dispatches dropped) and prints median, minimum and maximum, the two conditions (inverse no
           slower than the Jacobi launch of the same N; its 0 dB median within the repeat-to-repeat spread of its 20 dB runs)
           and the ratio to the default route.
  step     one music_pipeline.work_dev step at N = 4, K = 1024, P = 1024, M = 2, batch 4096 on the SAME handle with the MUSIC
           and the Capon estimator, alternating in one process; device events around synchronised blocks of steps.
  all      both of the above, each in a child process of its own (the first under rocprofv3), written to profiles/capon.txt.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-doa_amd", "python"))

SIZES = (4, 8, 16)
SNRS = (20.0, 0.0)
ITEMS, K, M = 4096, 256, 2
FAMILIES = ("capon", "jacobi", "default")


def configs():
    return [(N, snr) for N in SIZES for snr in SNRS]


def family(kernel_name):
    """capon: the inverse kernels; jacobi: the per-item-count eigen kernels (music_evd_*_counts_kernel, and for N <= 4
    music_evd_kernel<N, double, EvdOneCounts>); default: every other music_evd kernel (subspace, quad, plain)."""
    if "capon_inverse" in kernel_name:
        return "capon"
    if "music_evd" not in kernel_name:
        return None
    return "jacobi" if ("_counts_kernel" in kernel_name or "EvdOneCounts" in kernel_name) else "default"


def run_kernel(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()
    P = 256
    for N, snr in configs():
        streams, _ = doa.sim.make_batch_streams_torch(N, K, ITEMS, 0.5, M, snr, seed=11)
        R = torch.empty((ITEMS, N * N), dtype=torch.complex64, device="cuda")
        doa.autocorrelate(N, K, 0, 0).work_dev(ITEMS, [s.data_ptr() for s in streams], R.data_ptr(), st)
        spec = torch.empty((ITEMS, P), dtype=torch.float32, device="cuda")
        counts = torch.full((ITEMS,), M, dtype=torch.int32, device="cuda")
        capon = doa.capon_lin_array(0.5, N, P, 0.0)
        music = doa.MUSIC_lin_array(0.5, M, N, P)
        torch.cuda.synchronize()
        for call in (lambda: capon.work_dev(ITEMS, R.data_ptr(), spec.data_ptr(), None, st),
                     lambda: music.work_dev_counts(ITEMS, R.data_ptr(), counts.data_ptr(), spec.data_ptr(), st),
                     lambda: music.work_dev(ITEMS, R.data_ptr(), spec.data_ptr(), st)):
            for _ in range(a.warmup + a.reps):
                call()
                torch.cuda.synchronize()
    print(json.dumps({"reps": a.reps, "warmup": a.warmup, "items": ITEMS, "K": K, "sources": M}))


def summarize(a, out=sys.stdout):
    rows = {f: [] for f in FAMILIES}
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                fam = family(r["Kernel_Name"])
                if fam:
                    rows[fam].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    per = a.warmup + a.reps
    t = {}
    for fam in FAMILIES:
        rows[fam].sort()
        assert len(rows[fam]) == per * len(configs()), (fam, len(rows[fam]), per, len(configs()))
        for k, cfg in enumerate(configs()):
            chunk = rows[fam][k * per + a.warmup:(k + 1) * per]
            us = [(e - s) / 1000.0 for s, e, _ in chunk]
            t[fam, cfg] = (statistics.median(us), min(us), max(us), chunk[0][2].replace("(anonymous namespace)::", "").split("(")[0])
    print("per %d items, two sources, K = %d; kernel times from the trace, %d dispatches each (us: median, min, max)" % (ITEMS, K, a.reps), file=out)
    for cfg in configs():
        N, snr = cfg
        for fam in FAMILIES:
            med, lo, hi, name = t[fam, cfg]
            print("N %2d  %4.0f dB  %-7s %8.2f  (%.2f .. %.2f)  %s" % (N, snr, fam, med, lo, hi, name), file=out)
    print("", file=out)
    for N in SIZES:
        c20, c0 = t["capon", (N, 20.0)], t["capon", (N, 0.0)]
        spread = max(c20[2] - c20[1], c0[2] - c0[1])
        for snr in SNRS:
            c, j, d = t["capon", (N, snr)][0], t["jacobi", (N, snr)][0], t["default", (N, snr)][0]
            print("N %2d  %4.0f dB: inverse %.2f us, Jacobi form %.2f us (inverse %s; ratio %.2f), default route %.2f us (ratio %.2f)"
                  % (N, snr, c, j, "no slower" if c <= j else "SLOWER", c / j, d, c / d), file=out)
        print("N %2d: inverse 0 dB - 20 dB = %+.2f us, repeat-to-repeat spread %.2f us: %s" %
              (N, c0[0] - c20[0], spread, "within the spread" if abs(c0[0] - c20[0]) <= spread else "OUTSIDE the spread"), file=out)


def run_step(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    N, Ks, P, Ms, B = 4, 1024, 1024, 2, 4096
    streams, _ = doa.sim.make_batch_streams_torch(N, Ks, B, 0.5, Ms, 20.0, seed=7)
    streams = doa.sim.stream_slab_torch(streams)
    ptrs = [s.data_ptr() for s in streams]
    spec = torch.empty((B, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((B, Ms), dtype=torch.float32, device="cuda")
    am = torch.empty((B, Ms), dtype=torch.float32, device="cuda")
    pipe = doa.music_pipeline(N, Ks, 0, 0, 0.5, Ms, P, max_batch=B)
    st = torch.cuda.current_stream()
    times = {"music": [], "capon": []}
    for rnd in range(a.rounds + 1):                     # round 0 warms both settings up
        for mode in ("music", "capon"):
            pipe.set_estimator(mode, 0.0)
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
    out = {"shape": {"N": N, "K": Ks, "P": P, "M": Ms, "batch": B}, "steps_per_block": a.steps, "rounds": a.rounds}
    for mode, t in times.items():
        out[mode] = {"us_per_step_median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    out["capon_minus_music_us_median"] = round(statistics.median(times["capon"]) - statistics.median(times["music"]), 2)
    print(json.dumps(out))


def run_all(a):
    me = os.path.abspath(__file__)
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup)]
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, me,
                        "kernel"] + common, check=True, timeout=300, stdout=subprocess.DEVNULL)
        a.dir = tmp
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "capon.txt"), "w") as f:
            print("tools/profile_capon.py all (one rocprofv3 --kernel-trace --stats run; then the step comparison, device events)\n", file=f)
            summarize(a, f)
            step = subprocess.run([sys.executable, me, "step", "--steps", str(a.steps), "--rounds", str(a.rounds)] + common,
                                  check=True, timeout=300, capture_output=True, text=True)
            print("\nmusic_pipeline.work_dev step, MUSIC against Capon on one handle (us per step):\n" + step.stdout.strip(), file=f)
    print(open(os.path.join(ROOT, "profiles", "capon.txt")).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "summarize", "step", "all"))
    ap.add_argument("dir", nargs="?", help="summarize: the rocprofv3 output directory")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="step: work_dev calls per timed block")
    ap.add_argument("--rounds", type=int, default=7, help="step: timed blocks per setting, alternating")
    a = ap.parse_args()
    {"kernel": run_kernel, "summarize": summarize, "step": run_step, "all": run_all}[a.mode](a)


if __name__ == "__main__":
    main()
