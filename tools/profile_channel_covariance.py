"""Measurements of doa.channel_covariance beside doa.autocorrelate (profiles/channel_covariance.txt), 4096 snapshots per launch:

    python3 tools/profile_channel_covariance.py measure --out measured.json        (on the GPU)
    python3 tools/profile_channel_covariance.py write measured.json gr-doa_amd/build/channel_covariance.resources.txt
                                                                                    (where the library was built)

measure: HIP-event time per launch, launches back to back on one stream, at (N, K, F) = (4, 1024, 64), (8, 2048, 256) and
(2, 1024, 16); fc32 and sc16 streams; all bins and 8 selected bins; doa.autocorrelate on the same streams in the same run,
the variants alternating round by round.  Every launch reads another of several stream sets that together exceed 512 MiB,
twice the 256 MiB Infinity Cache, so no launch finds its samples cached.  The copy rate is measured in the same run (a
device-to-device copy of 1 GiB, read + written bytes over time).  Algorithmic bytes = the samples read once plus the items
and the power rows written.
write: adds the compiler's resource report (VGPRs, LDS, occupancy per instantiation) and writes the text file."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-doa_amd", "python"))

SNAPSHOTS = 4096
SHAPES = [(4, 1024, 64), (8, 2048, 256), (2, 1024, 16)]
SELECTED_BINS = 8
MIN_SET_BYTES = 512 << 20


def measure(a):
    import torch
    import doa

    assert torch.cuda.is_available(), "needs a HIP device"
    st = torch.cuda.current_stream()

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(reps):
            call(r)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / reps                 # us per launch

    # the copy rate of this device, now
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_us = statistics.median(timed(lambda r: dst.copy_(src), 10) for _ in range(5))
    copy_rate = 2.0 * src.numel() / (copy_us * 1e-6)               # bytes per second, read + written
    del src, dst
    out = {"device": torch.cuda.get_device_name(0), "snapshots": SNAPSHOTS, "reps": a.reps, "rounds": a.rounds,
           "copy_rate_TBps": round(copy_rate / 1e12, 3), "configs": []}

    for N, K, F in SHAPES:
        T = SNAPSHOTS * K
        g = torch.Generator(device="cuda")
        g.manual_seed(N * K + F)
        row = {"N": N, "K": K, "F": F}
        for fmt in ("fc32", "sc16"):
            sample_bytes = 8 if fmt == "fc32" else 4
            n_sets = max(2, -(-MIN_SET_BYTES // (N * T * sample_bytes)))
            sets = []
            for _ in range(n_sets):
                if fmt == "fc32":
                    s = [torch.view_as_complex(torch.randn((T, 2), generator=g, device="cuda", dtype=torch.float32)) for _ in range(N)]
                else:
                    s = [torch.randint(-2000, 2000, (T, 2), generator=g, device="cuda", dtype=torch.int16) for _ in range(N)]
                views = doa.sim.stream_slab_torch(s)                 # one slab per set, streams at the recommended distance
                del s
                sets.append((views, [t.data_ptr() for t in views]))
            cov = torch.empty((SNAPSHOTS * F, N * N), dtype=torch.complex64, device="cuda")
            pw = torch.empty((SNAPSHOTS, F), dtype=torch.float32, device="cuda")
            chan_all = doa.channel_covariance(N, K, 0, F, "hann")
            chan_sel = doa.channel_covariance(N, K, 0, F, "hann")
            chan_sel.set_bins(F // 4, SELECTED_BINS)
            k1 = doa.autocorrelate(N, K, 0, 0)
            if fmt == "sc16":
                for b in (chan_all, chan_sel, k1):
                    b.set_input_format("sc16", 2.0 ** -15)
            variants = {
                "channel_covariance_all_bins": lambda r: chan_all.work_dev(SNAPSHOTS, sets[r % n_sets][1], cov.data_ptr(), pw.data_ptr(), st),
                "channel_covariance_8_bins": lambda r: chan_sel.work_dev(SNAPSHOTS, sets[r % n_sets][1], cov.data_ptr(), pw.data_ptr(), st),
                "autocorrelate": lambda r: k1.work_dev(SNAPSHOTS, sets[r % n_sets][1], cov.data_ptr(), st),
            }
            times = {v: [] for v in variants}
            for rnd in range(a.rounds + 1):                          # round 0 warms every variant up
                for v, call in variants.items():
                    t = timed(call, a.reps)
                    if rnd:
                        times[v].append(t)
            in_bytes = N * T * sample_bytes
            written = {"channel_covariance_all_bins": SNAPSHOTS * F * (N * N * 8 + 4),
                       "channel_covariance_8_bins": SNAPSHOTS * (SELECTED_BINS * N * N * 8 + F * 4),
                       "autocorrelate": SNAPSHOTS * N * N * 8}
            res = {"stream_sets": n_sets}
            for v, t in times.items():
                med = statistics.median(t)
                nbytes = in_bytes + written[v]
                res[v] = {"us_per_launch_median": round(med, 1), "min": round(min(t), 1), "max": round(max(t), 1),
                          "algorithmic_MB": round(nbytes / 1e6, 1), "TBps": round(nbytes / (med * 1e-6) / 1e12, 3),
                          "fraction_of_copy_rate": round(nbytes / (med * 1e-6) / copy_rate, 3)}
            for v in ("channel_covariance_all_bins", "channel_covariance_8_bins"):
                res[v]["time_over_autocorrelate"] = round(res[v]["us_per_launch_median"] / res["autocorrelate"]["us_per_launch_median"], 2)
            row[fmt] = res
            del sets, cov, pw
            torch.cuda.empty_cache()
        out["configs"].append(row)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def resources(path):
    """[(loader, N, pair route, VGPRs, LDS bytes, waves per SIMD)] from -Rpass-analysis=kernel-resource-usage."""
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: \S*channel_covariance_kernelINS_\d+(Fc32|Sc16)SamplesELi(\d)ELb([01])ELb([01])", line)
        if m:
            cur = {"loader": m.group(1).lower(), "N": int(m.group(2)), "pair": m.group(3) == "1", "small": m.group(4) == "1"}
            rows.append(cur)
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def write(a):
    m = json.load(open(a.measured))
    lines = ["doa.channel_covariance beside doa.autocorrelate: %d snapshots per launch, overlap 0, Hann window, on %s" % (m["snapshots"], m["device"]),
             "HIP-event time per launch (us), launches back to back, median of %d rounds of %d launches, the variants alternating;" % (m["rounds"], m["reps"]),
             "every launch reads another of several stream sets (> 512 MiB together).  Copy rate in the same run: %.3f TB/s (read + written)." % m["copy_rate_TBps"],
             "bytes = samples read once + items and power rows written; fraction = bytes / time / copy rate.", ""]
    for c in m["configs"]:
        for fmt in ("fc32", "sc16"):
            r = c[fmt]
            lines.append("N %d  K %d  F %d  %s  (%d stream sets)" % (c["N"], c["K"], c["F"], fmt, r["stream_sets"]))
            for v in ("channel_covariance_all_bins", "channel_covariance_8_bins", "autocorrelate"):
                x = r[v]
                lines.append("  %-28s %8.1f us (min %8.1f max %8.1f)  %7.1f MB  %6.3f TB/s  %5.3f of copy rate%s" % (
                    v, x["us_per_launch_median"], x["min"], x["max"], x["algorithmic_MB"], x["TBps"], x["fraction_of_copy_rate"],
                    "  %5.2f x autocorrelate" % x["time_over_autocorrelate"] if "time_over_autocorrelate" in x else ""))
        lines.append("")
    lines.append("channel_covariance_kernel<loader, N, pair loads, F <= 64>: compiler resource report (gfx950), scratch 0 in every instantiation")
    lines.append("  loader  N  pair  F<=64  VGPRs  LDS bytes/workgroup  waves/SIMD")
    for r in sorted(resources(a.resources), key=lambda r: (r["loader"], r["N"], not r["pair"], not r["small"])):
        assert r["scratch"] == 0
        lines.append("  %-6s %2d  %-5s %-5s %6d %20d %11d" % (r["loader"], r["N"], "yes" if r["pair"] else "no", "yes" if r["small"] else "no", r["vgprs"], r["lds"], r["occupancy"]))
    path = os.path.join(ROOT, "profiles", "channel_covariance.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("measure")
    p.add_argument("--out")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p = sub.add_parser("write")
    p.add_argument("measured")
    p.add_argument("resources")
    a = ap.parse_args()
    {"measure": measure, "write": write}[a.mode](a)


if __name__ == "__main__":
    main()
