"""Measurements of doa.focus_covariance (profiles/focus_covariance.txt), 4096 snapshots of 64 bins per call:

    python3 tools/profile_focus_covariance.py measure --out measured.json        (on the GPU)
    python3 tools/profile_focus_covariance.py write measured.json gr-doa_amd/build/focus_covariance.resources.txt
                                                                                (where the library was built)

measure: HIP-event time per call, calls back to back on one stream, at N = 4, 8 and 16, P = 1024, the variants alternating
round by round, all in one run:
    focus         work_dev: the one launch
    copy          a device-to-device copy of the input items; reading the input once at that rate takes half its time
                  (the copy reads and writes every byte)
    chain         focus_covariance.work_dev then MUSIC_lin_array.work_dev over the n focused items
    wideband      wideband_music.work_dev (null_mean) on the same n * 64 items: the eigen stage over all of them
write: adds the compiler's resource report (VGPRs, scratch, LDS, occupancy per instantiation) and writes the text file."""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-doa_amd", "python"))

SNAPSHOTS, P, F = 4096, 1024, 64
SHAPES = [(4, 2), (8, 4), (16, 4)]            # N, M


def measure(a):
    import numpy as np
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
    n, nb = SNAPSHOTS, F
    for N, M in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(100 * N + nb)
        # items of 4 N samples, column-major: M white sources spread over 30 .. 150 degrees at 15 dB, noise of its own per item
        S = 4 * N
        th = torch.deg2rad(torch.linspace(30.0, 150.0, M + 2, device="cuda", dtype=torch.float64)[1:-1])
        loc = (N - 1 - 2 * torch.arange(N, device="cuda", dtype=torch.float64)) / 2.0
        A = torch.exp(1j * (-2.0 * torch.pi * torch.cos(th))[None, :] * loc[:, None] * 0.4).to(torch.complex64)       # [N, M]
        sig = torch.view_as_complex(torch.randn((n * nb, M, S, 2), generator=g, device="cuda", dtype=torch.float32)) * (0.5 ** 0.5)
        noise = torch.view_as_complex(torch.randn((n * nb, N, S, 2), generator=g, device="cuda", dtype=torch.float32))
        X = A[None] @ sig + (10.0 ** (-15.0 / 20.0) * 0.5 ** 0.5) * noise
        cov = (X @ X.conj().transpose(1, 2) / S).transpose(1, 2).contiguous().reshape(n * nb, N * N)
        del X, sig, noise
        cov2 = torch.empty_like(cov)
        foc = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
        spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
        focus = doa.focus_covariance.for_ula(0.4, N, F, np.linspace(20.0, 160.0, N), rate_over_carrier=0.4)
        music = doa.MUSIC_lin_array(0.4, M, N, P)
        wb = doa.wideband_music(0.4, M, N, P, F, 0, nb, 0.4, "null_mean")

        def chain():
            focus.work_dev(n, cov.data_ptr(), foc.data_ptr(), None, None, st)
            music.work_dev(n, foc.data_ptr(), spec.data_ptr(), st)

        variants = {
            "focus": lambda: focus.work_dev(n, cov.data_ptr(), foc.data_ptr(), None, None, st),
            "copy": lambda: cov2.copy_(cov),
            "chain": chain,
            "wideband": lambda: wb.work_dev(n, cov.data_ptr(), spec.data_ptr(), None, None, None, st),
        }
        times = {v: [] for v in variants}
        for rnd in range(a.rounds + 1):                          # round 0 warms every variant up
            for v, call in variants.items():
                t = timed(call, a.reps)
                if rnd:
                    times[v].append(t)
        res = {v: {"us_median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)} for v, t in times.items()}
        in_bytes = n * nb * N * N * 8
        row = {"N": N, "M": M, "bins": nb, "items": n * nb, "input_MB": round(in_bytes / 1e6, 1), "output_MB": round(n * N * N * 8 / 1e6, 2)}
        row.update(res)
        row["copy_GBps"] = round(2 * in_bytes / res["copy"]["us_median"] / 1e3, 0)
        row["read_once_us"] = round(res["copy"]["us_median"] / 2, 1)
        row["focus_over_read_once"] = round(res["focus"]["us_median"] / row["read_once_us"], 2)
        row["wideband_over_chain"] = round(res["wideband"]["us_median"] / res["chain"]["us_median"], 2)
        out["configs"].append(row)
        del cov, cov2, foc, spec
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def resources(path):
    """[{n, vgprs, agprs, sgprs, scratch, occupancy, lds}] from -Rpass-analysis=kernel-resource-usage."""
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: \S*focus_covariance_kernelILi(\d+)E", line)
        if m:
            cur = {"n": int(m.group(1))}
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
    lines = ["doa.focus_covariance: %d snapshots of %d bins per call, P = %d, on %s" % (m["snapshots"], m["F"], m["P"], m["device"]),
             "HIP-event time per call (us), calls back to back, median of %d rounds of %d calls, the variants alternating, one run." % (m["rounds"], m["reps"]),
             "focus = the one launch; read once = half a device-to-device copy of the input; chain = focus_covariance + MUSIC_lin_array",
             "over the n focused items; wideband = wideband_music (null_mean) on the same n * bins items.", ""]
    for c in m["configs"]:
        lines.append("N %d  M %d  (%d items, %.1f MB read, %.2f MB written; copy rate %d GB/s)" % (
            c["N"], c["M"], c["items"], c["input_MB"], c["output_MB"], c["copy_GBps"]))
        lines.append("  focus %8.1f (min %8.1f max %8.1f)   read once %8.1f   focus / read once %6.2f" % (
            c["focus"]["us_median"], c["focus"]["min"], c["focus"]["max"], c["read_once_us"], c["focus_over_read_once"]))
        lines.append("  chain %8.1f (min %8.1f max %8.1f)   wideband %8.1f (min %8.1f max %8.1f)   wideband / chain %6.2f%s" % (
            c["chain"]["us_median"], c["chain"]["min"], c["chain"]["max"], c["wideband"]["us_median"], c["wideband"]["min"],
            c["wideband"]["max"], c["wideband_over_chain"], "" if c["wideband_over_chain"] >= 1.0 else "   the chain is SLOWER"))
        lines.append("")
    lines.append("focus_covariance_kernel<N>: compiler resource report (gfx950), scratch 0 in every instantiation")
    lines.append("     N  VGPRs  AGPRs  SGPRs  scratch  LDS bytes/workgroup  waves/SIMD")
    for r in sorted(resources(a.resources), key=lambda r: r["n"]):
        assert r["scratch"] == 0
        lines.append("  %4d %6d %6d %6d %8d %20d %11d" % (r["n"], r["vgprs"], r["agprs"], r["sgprs"], r["scratch"], r["lds"], r["occupancy"]))
    path = os.path.join(ROOT, "profiles", "focus_covariance.txt")
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
