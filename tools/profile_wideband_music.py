"""Measurements of doa.wideband_music beside the chain by hand (profiles/wideband_music.txt), 4096 snapshots per call:

    python3 tools/profile_wideband_music.py measure --out measured.json        (on the GPU)
    python3 tools/profile_wideband_music.py write measured.json gr-doa_amd/build/wideband_music.resources.txt
                                                                                (where the library was built)

measure: HIP-event time per call, calls back to back on one stream, at P = 1024, F = 64 for (N, bins) = (4, 64), (4, 8) and
(8, 64), both combine rules, the variants alternating round by round:
    wideband      work_dev: the eigen launch over n * bins items and the scan launch
    front         the same call with every weight 0: the eigen launch, and a scan that only writes its n NaN rows
                  (scan = wideband - front is the scan launch's share, to the cost of those rows)
    by_hand       MUSIC_lin_array.work_dev over the n * bins items (n * bins * P floats written) and a torch mean of the
                  rows over the bins -- the cost of the chain without this block, not its result (one spacing in every bin)
write: adds the compiler's resource report (VGPRs, LDS, occupancy per instantiation) and writes the text file."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-doa_amd", "python"))

SNAPSHOTS, P, F = 4096, 1024, 64
SHAPES = [(4, 2, 64), (4, 2, 8), (8, 4, 64)]            # N, M, bins


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

    out = {"device": torch.cuda.get_device_name(0), "snapshots": SNAPSHOTS, "P": P, "F": F, "reps": a.reps, "rounds": a.rounds,
           "configs": []}
    n = SNAPSHOTS
    for N, M, nb in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(100 * N + nb)
        # items of 4 N samples, column-major: M white sources spread over 30 .. 150 degrees at 15 dB, noise of its own per item
        # (noise-only items would time the eigen stage on its slowest path, §3 "The eigen stage by SNR")
        S = 4 * N
        th = torch.deg2rad(torch.linspace(30.0, 150.0, M + 2, device="cuda", dtype=torch.float64)[1:-1])
        loc = (N - 1 - 2 * torch.arange(N, device="cuda", dtype=torch.float64)) / 2.0
        A = torch.exp(1j * (-2.0 * torch.pi * torch.cos(th))[None, :] * loc[:, None] * 0.4).to(torch.complex64)       # [N, M]
        sig = torch.view_as_complex(torch.randn((n * nb, M, S, 2), generator=g, device="cuda", dtype=torch.float32)) * (0.5 ** 0.5)
        noise = torch.view_as_complex(torch.randn((n * nb, N, S, 2), generator=g, device="cuda", dtype=torch.float32))
        X = A[None] @ sig + (10.0 ** (-15.0 / 20.0) * 0.5 ** 0.5) * noise
        cov = (X @ X.conj().transpose(1, 2) / S).transpose(1, 2).contiguous().reshape(n * nb, N * N)
        del X, sig, noise
        spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
        rows = torch.empty((n * nb, P), dtype=torch.float32, device="cuda")
        zero_w = torch.zeros((n, nb), dtype=torch.float32, device="cuda")
        music = doa.MUSIC_lin_array(0.4, M, N, P)

        def by_hand():
            music.work_dev(n * nb, cov.data_ptr(), rows.data_ptr(), st)
            torch.mean(rows.view(n, nb, P), dim=1, out=spec)

        row = {"N": N, "M": M, "bins": nb, "items": n * nb, "by_hand_row_MB": round(n * nb * P * 4 / 1e6, 1),
               "spectrum_MB": round(n * P * 4 / 1e6, 1)}
        for combine in ("null_mean", "power_sum"):
            wb = doa.wideband_music(0.4, M, N, P, F, 0, nb, 0.4, combine)
            variants = {
                "wideband": lambda: wb.work_dev(n, cov.data_ptr(), spec.data_ptr(), None, None, None, st),
                "front": lambda: wb.work_dev(n, cov.data_ptr(), spec.data_ptr(), zero_w.data_ptr(), None, None, st),
                "by_hand": by_hand,
            }
            times = {v: [] for v in variants}
            for rnd in range(a.rounds + 1):                          # round 0 warms every variant up
                for v, call in variants.items():
                    t = timed(call, a.reps)
                    if rnd:
                        times[v].append(t)
            res = {v: {"us_median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
                   for v, t in times.items()}
            res["scan_us"] = round(res["wideband"]["us_median"] - res["front"]["us_median"], 1)
            res["by_hand_over_wideband"] = round(res["by_hand"]["us_median"] / res["wideband"]["us_median"], 2)
            row[combine] = res
        out["configs"].append(row)
        del cov, rows, spec
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def resources(path):
    """[{np, pmax, combine, vgprs, sgprs, scratch, occupancy, lds}] from -Rpass-analysis=kernel-resource-usage."""
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: \S*wideband_scan_kernelILi(\d+)ELi(\d+)ELi([01])E", line)
        if m:
            cur = {"np": int(m.group(1)), "pmax": int(m.group(2)), "combine": ("null_mean", "power_sum")[int(m.group(3))]}
            rows.append(cur)
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def write(a):
    m = json.load(open(a.measured))
    lines = ["doa.wideband_music beside the chain by hand: %d snapshots per call, P = %d, F = %d, on %s" % (m["snapshots"], m["P"], m["F"], m["device"]),
             "HIP-event time per call (us), calls back to back, median of %d rounds of %d calls, the variants alternating." % (m["rounds"], m["reps"]),
             "wideband = eigen launch + scan launch; front = the same call with every weight 0 (the eigen launch and n NaN rows);",
             "scan = wideband - front; by_hand = MUSIC_lin_array.work_dev over n * bins items + torch.mean of the rows over the bins.", ""]
    for c in m["configs"]:
        lines.append("N %d  M %d  %d bins  (%d items; the chain by hand writes %.1f MB of rows, this block %.1f MB)" % (
            c["N"], c["M"], c["bins"], c["items"], c["by_hand_row_MB"], c["spectrum_MB"]))
        for combine in ("null_mean", "power_sum"):
            r = c[combine]
            lines.append("  %-10s wideband %8.1f (min %8.1f max %8.1f)   front %8.1f   scan %8.1f   by_hand %8.1f (min %8.1f max %8.1f)   by_hand / wideband %5.2f%s" % (
                combine, r["wideband"]["us_median"], r["wideband"]["min"], r["wideband"]["max"], r["front"]["us_median"], r["scan_us"],
                r["by_hand"]["us_median"], r["by_hand"]["min"], r["by_hand"]["max"], r["by_hand_over_wideband"],
                "" if r["by_hand_over_wideband"] >= 1.0 else "   SLOWER than the chain by hand"))
        lines.append("")
    lines.append("wideband_scan_kernel<polynomial size, LDS row, combine>: compiler resource report (gfx950), scratch 0 in every instantiation")
    lines.append("  size  row    combine     VGPRs  SGPRs  LDS bytes/workgroup  waves/SIMD")
    for r in sorted(resources(a.resources), key=lambda r: (r["np"], r["pmax"], r["combine"])):
        assert r["scratch"] == 0
        lines.append("  %4d  %5d  %-10s %6d %6d %20d %11d" % (r["np"], r["pmax"], r["combine"], r["vgprs"], r["sgprs"], r["lds"], r["occupancy"]))
    path = os.path.join(ROOT, "profiles", "wideband_music.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("measure")
    p.add_argument("--out")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p = sub.add_parser("write")
    p.add_argument("measured")
    p.add_argument("resources")
    a = ap.parse_args()
    {"measure": measure, "write": write}[a.mode](a)


if __name__ == "__main__":
    main()
