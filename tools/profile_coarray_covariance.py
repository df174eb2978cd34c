"""Measurements of doa.coarray_covariance (profiles/coarray_covariance.txt), 4096 items per call:

    python3 tools/profile_coarray_covariance.py measure --out measured.json        (on the GPU)
    python3 tools/profile_coarray_covariance.py write measured.json gr-doa_amd/build/coarray_covariance.resources.txt
                                                                                (where the library was built)

measure: HIP-event time per call, calls back to back on one stream, for mra4 (0 1 4 6 -> 7), nested6 (0 1 2 3 7 11 -> 12) and
the 16-element uniform array (16 -> 16), the variants alternating round by round, all in one run:
    smoothed, toeplitz   work_dev in that mode: the one launch
    same bytes           a device-to-device copy of (input + output) / 2 bytes: one launch that moves the launch's bytes
    smooth               (16 -> 16 only) spatial_smooth.work_dev at N = 16, S = 15, forward-backward: the kernel this one is modelled on
and once per run the copy rate of a 256 MiB device-to-device copy (bytes read plus bytes written over its time); `floor` is
the launch's input plus output bytes at that rate.
write: adds the compiler's resource report (VGPRs, scratch, LDS, occupancy per instantiation) and writes the text file."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-doa_amd", "python"))

ITEMS = 4096
LAYOUTS = [("mra4", (0, 1, 4, 6)), ("nested6", (0, 1, 2, 3, 7, 11)), ("ula16", tuple(range(16)))]
MODES = ("smoothed", "toeplitz")


def measure(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / reps                 # us per call

    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)
    big2.copy_(big)
    rate = statistics.median(2 * big.numel() / timed(lambda: big2.copy_(big), 5) / 1e3 for _ in range(a.rounds))       # GB/s
    del big, big2
    torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "items": ITEMS, "reps": a.reps, "rounds": a.rounds, "copy_GBps": round(rate, 0),
           "configs": []}
    n = ITEMS
    for name, positions in LAYOUTS:
        N = len(positions)
        g = torch.Generator(device="cuda")
        g.manual_seed(100 + N)
        cov = torch.view_as_complex(torch.randn((n, N * N, 2), generator=g, device="cuda", dtype=torch.float32))
        blocks = {mode: doa.coarray_covariance(positions, 0, mode) for mode in MODES}
        Lv = blocks["smoothed"].virtual_size
        res = torch.empty((n, Lv * Lv), dtype=torch.complex64, device="cuda")
        moved = n * (N * N + Lv * Lv) * 8
        half, half2 = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        variants = {mode: (lambda b=blocks[mode]: b.work_dev(n, cov.data_ptr(), res.data_ptr(), st)) for mode in MODES}
        variants["same_bytes"] = lambda: half2.copy_(half)
        if name == "ula16":
            smooth = doa.spatial_smooth(16, 15, True)
            sm = torch.empty((n, 15 * 15), dtype=torch.complex64, device="cuda")
            variants["smooth"] = lambda: smooth.work_dev(n, cov.data_ptr(), sm.data_ptr(), st)
        times = {v: [] for v in variants}
        for rnd in range(a.rounds + 1):                          # round 0 warms every variant up
            for v, call in variants.items():
                t = timed(call, a.reps)
                if rnd:
                    times[v].append(t)
        row = {"name": name, "positions": list(positions), "N": N, "Lv": Lv, "moved_MB": round(moved / 1e6, 2),
               "floor_us": round(moved / rate / 1e3, 2)}
        row.update({v: {"us_median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)} for v, t in times.items()})
        out["configs"].append(row)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def resources(path):
    """[{v16, mode, vgprs, agprs, sgprs, scratch, occupancy, lds}] from -Rpass-analysis=kernel-resource-usage."""
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: \S*coarray_covariance_kernelILb(\d)ELi(\d)E", line)
        if m:
            cur = {"v16": int(m.group(1)), "mode": MODES[int(m.group(2))]}
            rows.append(cur)
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def write(a):
    m = json.load(open(a.measured))
    lines = ["doa.coarray_covariance: %d items per call, on %s" % (m["items"], m["device"]),
             "HIP-event time per call (us), calls back to back, median of %d rounds of %d calls, the variants alternating, one run." % (m["rounds"], m["reps"]),
             "smoothed / toeplitz = the one launch in that mode; floor = the launch's input plus output bytes at the copy rate of a",
             "256 MiB device-to-device copy (%d GB/s, read plus written); same bytes = one copy launch that moves as many bytes;" % m["copy_GBps"],
             "smooth = spatial_smooth at N = 16, S = 15, forward-backward, on the same items.", ""]
    for c in m["configs"]:
        lines.append("%s  %s -> %d  (%.2f MB read plus written)" % (c["name"], " ".join(str(p) for p in c["positions"]), c["Lv"], c["moved_MB"]))
        for mode in MODES:
            lines.append("  %-9s %7.2f (min %7.2f max %7.2f)   floor %6.2f   launch / floor %6.2f   same bytes %6.2f   launch / same bytes %5.2f" % (
                mode, c[mode]["us_median"], c[mode]["min"], c[mode]["max"], c["floor_us"], c[mode]["us_median"] / c["floor_us"],
                c["same_bytes"]["us_median"], c[mode]["us_median"] / c["same_bytes"]["us_median"]))
        if "smooth" in c:
            lines.append("  %-9s %7.2f (min %7.2f max %7.2f)   smoothed / smooth %5.2f   toeplitz / smooth %5.2f" % (
                "smooth", c["smooth"]["us_median"], c["smooth"]["min"], c["smooth"]["max"],
                c["smoothed"]["us_median"] / c["smooth"]["us_median"], c["toeplitz"]["us_median"] / c["smooth"]["us_median"]))
        lines.append("")
    lines.append("coarray_covariance_kernel<16-byte form, mode>: compiler resource report (gfx950), scratch 0 in every instantiation")
    lines.append("  access   mode      VGPRs  AGPRs  SGPRs  scratch  LDS bytes/workgroup  waves/SIMD")
    for r in sorted(resources(a.resources), key=lambda r: (r["mode"], -r["v16"])):
        assert r["scratch"] == 0
        lines.append("  %-8s %-9s %5d %6d %6d %8d %20d %11d" % ("16-byte" if r["v16"] else "8-byte", r["mode"], r["vgprs"], r["agprs"], r["sgprs"],
                                                                r["scratch"], r["lds"], r["occupancy"]))
    path = os.path.join(ROOT, "profiles", "coarray_covariance.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("measure")
    p.add_argument("--out")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--rounds", type=int, default=7)
    p = sub.add_parser("write")
    p.add_argument("measured")
    p.add_argument("resources")
    a = ap.parse_args()
    {"measure": measure, "write": write}[a.mode](a)


if __name__ == "__main__":
    main()
