"""Measurements of the IAA estimator (profiles/iaa.txt):

  kernel   per 4096 covariance items (two sources, K = 256, 20 dB) at (N, P) = (4, 1024), (8, 1024) and (16, 4096), on
           device-resident items through the blocks' work_dev:
             iaa       iaa_wave_kernel at 10 iterations, and at 1 and 20 to show the slope   (doa.iaa_lin_array.work_dev)
             capon     capon_inverse_kernel                                                   (doa.capon_lin_array.work_dev)
             scan      the uniform-linear-array scan kernel of the same call
           for a `rocprofv3 --kernel-trace --stats` run of its own, with no counters in the same run -- kernel times come from
           the trace, not from this script:

               rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_iaa.py kernel
               python3 tools/profile_iaa.py summarize OUT

           `summarize` splits the trace's dispatches of each family, in order, into the configurations `kernel` ran (warm-up
           dispatches dropped), prints median, minimum and maximum, and sets beside the IAA time what it is to be judged
           against: L x (capon_inverse_kernel + scan) from the same run -- what IAA would cost chained out of existing
           launches, two sweeps' worth of scan short of it -- and the time of its double flops by count at the vector FP64
           peak.
  all      the above in a child process under rocprofv3, written to profiles/iaa.txt next to the compiler's resource report
           of the kernels (gr-doa_amd/build/iaa.resources.txt, when the build left one).
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-doa_amd", "python"))

SHAPES = ((4, 1024), (8, 1024), (16, 4096))
ITERATIONS = (10, 1, 20)            # the order `kernel` runs them in
ITEMS, K, M = 4096, 256, 2
FAMILIES = ("iaa", "capon", "scan")
# Vector FP64 flop/s of an MI355X as AMD's data sheet of the part gives it (78.6 Tflop/s): 256 CUs x 4 SIMDs x 16 double FMAs
# per clock x 2 flops at 2.4 GHz, half the 157.3 Tflop/s FP32 vector rate.  A spec figure, not measured here.
PEAK_FP64 = 78.6e12
FLOP_PER_CELL = 24                  # double flops per direction, element and iteration: two Horner chains of 4 FMAs a step,
                                    # one lag accumulator of 2 FMAs, 2 products and 2 additions


def flops_by_count(N, P, L):
    """The issue's count: L iterations of FLOP_PER_CELL flops per direction and element, for every item.  It counts the two
    polynomials and the lag accumulation only.  Left out: the start sweep (one polynomial), the last evaluation of the pair,
    the division per direction, the reduction of the lags and the whole dense step (Cholesky, inverse, two products)."""
    return float(FLOP_PER_CELL) * N * P * L * ITEMS


def family(kernel_name):
    if "iaa_wave_kernel" in kernel_name:
        return "iaa"
    if "capon_inverse" in kernel_name:
        return "capon"
    if "music_scan" in kernel_name:
        return "scan"
    return None


def run_kernel(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()
    for N, P in SHAPES:
        streams, _ = doa.sim.make_batch_streams_torch(N, K, ITEMS, 0.5, M, 20.0, seed=11)
        R = torch.empty((ITEMS, N * N), dtype=torch.complex64, device="cuda")
        doa.autocorrelate(N, K, 0, 0).work_dev(ITEMS, [s.data_ptr() for s in streams], R.data_ptr(), st)
        spec = torch.empty((ITEMS, P), dtype=torch.float32, device="cuda")
        power = torch.empty((ITEMS, P), dtype=torch.float32, device="cuda")
        status = torch.empty((ITEMS,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for L in ITERATIONS:
            blk = doa.iaa_lin_array(0.5, N, P, 0.0, L)
            for _ in range(a.warmup + a.reps):
                blk.work_dev(ITEMS, R.data_ptr(), spec.data_ptr(), power.data_ptr(), status.data_ptr(), st)
                torch.cuda.synchronize()
            assert int(status.sum().item()) == 0
        capon = doa.capon_lin_array(0.5, N, P, 0.0)
        for _ in range(a.warmup + a.reps):
            capon.work_dev(ITEMS, R.data_ptr(), spec.data_ptr(), None, st)
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
    want = {"iaa": per * len(SHAPES) * len(ITERATIONS), "capon": per * len(SHAPES), "scan": per * len(SHAPES)}
    t = {}

    def chunk(fam, k):
        c = rows[fam][k * per + a.warmup:(k + 1) * per]
        us = [sum((e - s) / 1000.0 for s, e, _ in call) for call in c]
        return statistics.median(us), min(us), max(us), " + ".join(n.replace("(anonymous namespace)::", "").split("(")[0] for _, _, n in c[0])

    for fam in FAMILIES:
        rows[fam].sort()
        each, rest = divmod(len(rows[fam]), want[fam])              # launches of the family per call (the scan may take two)
        assert each >= 1 and rest == 0, (fam, len(rows[fam]), want[fam])
        rows[fam] = [rows[fam][i * each:(i + 1) * each] for i in range(want[fam])]
    for s, shape in enumerate(SHAPES):
        for l, L in enumerate(ITERATIONS):
            t["iaa", shape, L] = chunk("iaa", s * len(ITERATIONS) + l)
        t["capon", shape] = chunk("capon", s)
        t["scan", shape] = chunk("scan", s)
    print("per %d items, two sources, K = %d, 20 dB; kernel times from the trace, %d dispatches each (us: median, min, max)"
          % (ITEMS, K, a.reps), file=out)
    for shape in SHAPES:
        N, P = shape
        for L in sorted(ITERATIONS):
            med, lo, hi, name = t["iaa", shape, L]
            print("N %2d P %4d  iaa L=%-2d %10.2f  (%.2f .. %.2f)  %s" % (N, P, L, med, lo, hi, name), file=out)
        for fam in ("capon", "scan"):
            med, lo, hi, name = t[fam, shape]
            print("N %2d P %4d  %-8s %10.2f  (%.2f .. %.2f)  %s" % (N, P, fam, med, lo, hi, name), file=out)
    print("", file=out)
    for shape in SHAPES:
        N, P = shape
        iaa10, iaa1, iaa20 = t["iaa", shape, 10][0], t["iaa", shape, 1][0], t["iaa", shape, 20][0]
        chained = 10 * (t["capon", shape][0] + t["scan", shape][0])
        count = flops_by_count(N, P, 10) / PEAK_FP64 * 1e6
        print("N %2d P %4d: IAA at 10 iterations %.1f us; slope %.1f us per iteration between 1 and 20 (one iteration alone: %.1f us)"
              % (N, P, iaa10, (iaa20 - iaa1) / 19.0, iaa1), file=out)
        print("            10 x (capon_inverse_kernel + scan) = %.1f us: ratio %.2f;  %.3g double flops by count (sweeps only, no "
              "dense step) = %.1f us at the %.1f Tflop/s of the data sheet: ratio %.1f"
              % (chained, iaa10 / chained, flops_by_count(N, P, 10), count, PEAK_FP64 / 1e12, iaa10 / count), file=out)


def resource_report(out):
    path = os.path.join(ROOT, "gr-doa_amd", "build", "iaa.resources.txt")
    if not os.path.exists(path):
        return
    print("\nthe compiler's resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):", file=out)
    keep = re.compile(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize|Occupancy|LDS Size)( \[[^\]]*\])?: (.*?) \[-R")
    for line in open(path):
        m = keep.search(line)
        if m:
            print(("  " if m.group(1) != "Function Name" else "") + m.group(1) + (m.group(2) or "") + ": " + m.group(3), file=out)


def run_all(a):
    me = os.path.abspath(__file__)
    common = ["--reps", str(a.reps), "--warmup", str(a.warmup)]
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, me,
                        "kernel"] + common, check=True, timeout=300, stdout=subprocess.DEVNULL)
        a.dir = tmp
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "iaa.txt"), "w") as f:
            print("tools/profile_iaa.py all (one rocprofv3 --kernel-trace --stats run, no counters)\n", file=f)
            summarize(a, f)
            resource_report(f)
    print(open(os.path.join(ROOT, "profiles", "iaa.txt")).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "summarize", "all"))
    ap.add_argument("dir", nargs="?", help="summarize: the rocprofv3 output directory")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    {"kernel": run_kernel, "summarize": summarize, "all": run_all}[a.mode](a)


if __name__ == "__main__":
    main()
