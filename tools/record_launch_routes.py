#!/usr/bin/env python3
"""Records which kernels the public entries really launch, for tests/test_cpu_launch_routes.py.

Two steps, both on a machine with the device:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/record_launch_routes.py run OUT/calls.json
    python3 tools/record_launch_routes.py write OUT tests/golden/launch_routes.json

`run` walks a fixed table of shapes through autocorrelate, MUSIC_lin_array (work_dev, work_dev_counts, debug),
calibrate_lin_array, esprit_linear_array, rootMUSIC_linear_array, MUSIC_array, music_pipeline (work_dev, work_dev_auto,
work_dev_batches) and root_pipeline's ESPRIT auto mode, and then every recipe of tests/route_census.py (one call and one row,
labelled "census:<entry>", per kernel instantiation the launch plan can select), with a marker kernel (a one-element int32 fill) in front of every call,
and writes what it called: per call a label and, for each of the three routed stages the call runs, the shape in the form
doa_hip_launch_route_debug takes (gr-doa_amd/csrc/launch_routes.hpp).  The shapes are written down here from the arguments of
the call and from what include/doa_hip.h says the entries do; no route function is asked.  `write` splits the kernel trace at
the markers and writes one row per call: the entry, the shapes, and the kernels in launch order, each as [index into `names`
(every kernel name as traced, once), grid and workgroup size as traced, in work-items]; and the device's compute-unit count.  DOA_HIP_LIB selects the library (a build of another commit gives
the file that commit's launches).  The golden file is never edited by hand."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "gr-doa_amd", "python"))     # (PYTHONPATH first: another commit's package beside its library)

K1, EVD, SCAN = 0, 1, 2
FIXED, COUNTS, RECORD, FULL, CALIBRATE, GROUP = range(6)
MARKER = "FillFunctor<int>"
LENGTHS = (64, 100, 256, 512, 1024, 2048, 4096, 4160, 8192)


def cov_shape(N, K, ovl, avg, n_out, fmt, pair, group=0):
    S = K - ovl
    wants_ws = (not group) and ovl > 0 and N <= 8 and S % 2 == 0 and (K % S) % 2 == 0     # the handles supply it exactly then
    return [K1, [N, K, ovl, avg, n_out, fmt, int(pair), int(wants_ws), group]]


def evd_shape(N, M, bits, n, mode=FIXED, pn=0, cheb=0, es=0):
    return [EVD, [N, M, bits, n, mode, pn, cheb, es]]


def has_cheb(N, bits):
    return int(N <= 4 and bits == 64)           # spectrum_plan: the Chebyshev record exists


def scan_shape(N, bits, P, n, aligned=1, q=0, pick=0, M=0, store=1, group=0):
    return [SCAN, [N, bits, P, n, int(aligned), q, pick, M if pick else 0, store if pick else 1, has_cheb(N, bits), group]]


def run(calls_path):
    import numpy as np
    import torch
    import doa

    torch.cuda.set_device(0)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    big, over = 16 * cu, 16 * cu + 4 * cu - 120         # 4096 and 5000 on 256 compute units: both sides of the 16-waves-per-CU cap
    lean16 = 64 * cu                                    # first size at which the lean scan goes to 16 waves per CU
    rng = np.random.default_rng(1)
    K = 64
    n_samples = (over + 2) * K + 8
    fc = [torch.from_numpy((rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)).astype(np.complex64)).cuda() for _ in range(16)]
    sc = [torch.from_numpy(rng.integers(-2000, 2000, 2 * n_samples).astype(np.int16)).cuda() for _ in range(16)]
    n_max = max(lean16, big)
    cov = {}
    for N in range(2, 17):                              # Hermitian items with a plain spectrum, enough for every call
        n = n_max if N <= 4 else big
        a = (rng.standard_normal((64, N, 2 * N)) + 1j * rng.standard_normal((64, N, 2 * N))).astype(np.complex64)
        R = (a @ a.conj().transpose(0, 2, 1) / (2 * N)).astype(np.complex64)
        cov[N] = torch.from_numpy(np.tile(R.reshape(64, N * N), (n // 64 + 1, 1))[:n].copy()).cuda()
    spec = torch.empty(max(n_max * 256, big * 8192) + 4, dtype=torch.float32, device="cuda")
    outs = [torch.empty((over + 8) * 16 * 16 * 2, dtype=torch.float32, device="cuda") for _ in range(2)]
    counts = torch.from_numpy(np.ones(n_max, np.int32)).cuda()          # (uploads, not fills: the only int32 fill is the marker)
    marker = torch.from_numpy(np.zeros(1, np.int32)).cuda()
    torch.cuda.synchronize()
    calls = []

    def call(label, stages, fn):
        marker.fill_(len(calls))
        fn()
        torch.cuda.synchronize()
        calls.append({"call": label, "stages": stages})

    def streams(N, fmt, offset):
        bufs, sb = (sc, 4) if fmt else (fc, 8)
        return [bufs[k].data_ptr() + offset * sb for k in range(N)]

    # ---- K1 through autocorrelate.work_dev ----
    windows = [(64, 0), (63, 0), (64, 32), (64, 16), (64, 33)]
    k1 = []
    for N in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
        k1 += [(N, Kk, ovl, 0, 3, 0, 0) for Kk, ovl in (windows if N in (1, 4, 8, 9) else windows[:3:2])]
        if N in (1, 4, 5, 8, 9, 16):
            k1 += [(N, Kk, ovl, 0, 3, fmt, off) for Kk, ovl in windows[:3:2] for fmt, off in ((0, 1), (1, 0))]
        if N in (2, 4, 6, 8, 9, 16):
            k1 += [(N, Kk, ovl, 0, n, 0, 0) for Kk, ovl in windows[:3:2] for n in (big, over)]
    k1 += [(N, Kk, ovl, 0, 3, 1, 1) for N in (4, 9) for Kk, ovl in windows[:3:2]]
    k1 += [(9, 64, 0, 1, 3, 0, 0), (9, 64, 0, 1, big, 0, 0), (9, 64, 32, 1, 3, 0, 0)]
    for N, Kk, ovl, avg, n, fmt, off in k1:
        blk = (doa.autocorrelate_sc16 if fmt else doa.autocorrelate)(N, Kk, ovl, avg)
        call("autocorrelate.work_dev",
             [cov_shape(N, Kk, ovl, avg, n, fmt, off == 0)],
             lambda: blk.work_dev(n, streams(N, fmt, off), outs[0].data_ptr()))
        blk.close()

    # ---- the eigen stage (and the scan behind it) through the item blocks ----
    def sources(N):
        return sorted({m for m in (1, 2, 3, 4, N - 1) if 1 <= m < N})

    some = (2, 4, 5, 8, 9, 16)
    for bits in (64, 32):
        for N in (range(2, 17) if bits == 64 else (4, 8, 16)):
            for M in (sources(N) if N in (2, 3) + some else (1,)):
                blk = doa.MUSIC_lin_array(0.5, M, N, 64)
                blk.set_internal_precision(bits)
                for n in ((1, 70) if M == 1 and bits == 64 and N in (4, 8, 16) else (70,)):
                    call("MUSIC_lin_array.work_dev",
                         [evd_shape(N, M, bits, n, cheb=has_cheb(N, bits)), scan_shape(N, bits, 64, n)],
                         lambda: blk.work_dev(n, cov[N].data_ptr(), spec.data_ptr()))
                if M in (1, 2, N - 1) and N in (4, 8, 16):
                    host = cov[N][:70].cpu().numpy()
                    call("MUSIC_lin_array.debug",
                         [evd_shape(N, M, bits, 70, pn=1, cheb=has_cheb(N, bits)), scan_shape(N, bits, 64, 70, q=1)],
                         lambda: blk.debug(host))
                blk.close()
            if N not in some:
                continue
            blk = doa.calibrate_lin_array(0.5, N, 45.0)
            blk.set_internal_precision(bits)
            call("calibrate_lin_array.work_dev", [evd_shape(N, 1, bits, 70, CALIBRATE)],
                 lambda: blk.work_dev(70, cov[N].data_ptr(), outs[0].data_ptr()))
            blk.close()
    for N, P, bits in ((4, 4096, 64), (16, 4096, 64), (16, 2048, 64), (4, 4096, 32)):    # Q wanted on long rows: the fast kernel
        blk = doa.MUSIC_lin_array(0.5, 1, N, P)
        blk.set_internal_precision(bits)
        host = cov[N][:3].cpu().numpy()
        call("MUSIC_lin_array.debug", [evd_shape(N, 1, bits, 3, pn=1, cheb=has_cheb(N, bits)), scan_shape(N, bits, P, 3, q=1)],
             lambda: blk.debug(host))
        blk.close()
    for N in some:
        for n in (1, 70):
            blk = doa.MUSIC_lin_array(0.5, 1, N, 64)
            call("MUSIC_lin_array.work_dev_counts",
                 [evd_shape(N, 0, 64, n, COUNTS, cheb=has_cheb(N, 64)), scan_shape(N, 64, 64, n)],
                 lambda: blk.work_dev_counts(n, cov[N].data_ptr(), counts.data_ptr(), spec.data_ptr()))
            blk.close()
        blk = doa.esprit_linear_array(0.5, 1, N)
        call("esprit_linear_array.work_dev", [evd_shape(N, 1, 64, 70, RECORD)],
             lambda: blk.work_dev(70, cov[N].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()))
        blk.close()
        blk = doa.rootMUSIC_linear_array(0.5, 1, N)
        call("rootMUSIC_linear_array.work_dev", [evd_shape(N, 1, 64, 70)],
             lambda: blk.work_dev(70, cov[N].data_ptr(), outs[0].data_ptr()))
        call("rootMUSIC_linear_array.work_dev_counts", [evd_shape(N, 0, 64, 70, COUNTS)],
             lambda: blk.work_dev_counts(70, cov[N].data_ptr(), counts.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()))
        blk.close()
        steering = np.exp(1j * rng.uniform(0, 6.28, (32, N)))
        blk = doa.MUSIC_array(1, steering)
        call("MUSIC_array.work_dev", [evd_shape(N, 1, 64, 70, FULL)],
             lambda: blk.work_dev(70, cov[N].data_ptr(), spec.data_ptr()))
        blk.close()
        # a count per item together with the signal-subspace record: root_pipeline's ESPRIT auto mode
        blk = doa.root_pipeline(N, K, 0, 0, 0.5, 1, 128)
        blk.set_estimator("esprit")
        call("root_pipeline[esprit].work_dev_auto",
             [cov_shape(N, K, 0, 0, 70, 0, True), evd_shape(N, 0, 64, 70, COUNTS, es=1)],
             lambda: blk.work_dev_auto(70, streams(N, 0, 0), outs[0].data_ptr(), counts.data_ptr(), d_status_ptr=outs[1].data_ptr()))
        blk.close()

    # ---- the scan through MUSIC_lin_array.work_dev (no pick) and music_pipeline (picks) ----
    for bits in (64, 32):
        for N in (2, 3, 4, 5, 6, 8, 9, 12, 16):
            for P in LENGTHS:
                if (bits == 32 and (N not in (4, 16) or P not in (64, 1024, 2048, 4096, 8192))) or (N not in (4, 5, 16) and P not in (256, 4096)):
                    continue
                sizes = [3]
                if (N in (4, 8, 16) and P in (100, 256, 1024, 4096, 4160, 8192) and bits == 64) or (N in (4, 16) and P in (1024, 4096) and bits == 32):
                    sizes.append(big)
                if P == 256 and N == 4 and bits == 64:
                    sizes.append(lean16)
                blk = doa.MUSIC_lin_array(0.5, 1, N, P)
                blk.set_internal_precision(bits)
                for n in sizes:
                    call("MUSIC_lin_array.work_dev",
                         [evd_shape(N, 1, bits, n, cheb=has_cheb(N, bits)), scan_shape(N, bits, P, n)],
                         lambda: blk.work_dev(n, cov[N].data_ptr(), spec.data_ptr()))
                if N in (4, 8) and P in (256, 4096) and bits == 64:
                    call("MUSIC_lin_array.work_dev",
                         [evd_shape(N, 1, bits, 3, cheb=has_cheb(N, bits)), scan_shape(N, bits, P, 3, aligned=0)],
                         lambda: blk.work_dev(3, cov[N].data_ptr(), spec.data_ptr() + 4))
                blk.close()
    pipes = [(N, M, P, 64, 3) for N in (4, 6, 16) for M in (1, 2) for P in (100, 256, 1024, 4096, 4160)]
    pipes += [(4, 1, P, 32, 3) for P in (256, 1024, 4096)]
    pipes += [(4, 1, 1024, 64, big), (4, 2, 1024, 64, big), (8, 2, 4096, 64, big), (4, 1, 256, 64, lean16), (16, 1, 1024, 32, big)]
    for N, M, P, bits, n in pipes:
        pipe = doa.music_pipeline(N, K, 0, 0, 0.5, M, P, max_batch=n)
        pipe.set_internal_precision(bits)
        for store in ((1, 0) if n == 3 and bits == 64 and P in (256, 1024, 4096) else (1,)):
            call("music_pipeline.work_dev",
                 [cov_shape(N, K, 0, 0, n, 0, True), evd_shape(N, M, bits, n, cheb=has_cheb(N, bits)),
                  scan_shape(N, bits, P, n, pick=1, M=M, store=store)],
                 lambda: pipe.work_dev(n, streams(N, 0, 0), None, spec.data_ptr() if store else None, outs[0].data_ptr(), outs[1].data_ptr()))
        if bits == 64 and n == 3 and P == 1024:
            call("music_pipeline.work_dev_auto",
                 [cov_shape(N, K, 0, 0, n, 0, True), evd_shape(N, 0, 64, n, COUNTS, cheb=has_cheb(N, 64)), scan_shape(N, 64, P, n)],
                 lambda: pipe.work_dev_auto(n, streams(N, 0, 0), outs[0].data_ptr(), outs[1].data_ptr(), counts.data_ptr(),
                                            d_spec_ptr=spec.data_ptr()))
        pipe.close()
    # a smoothed handle: the table is the subarray's, the covariance stage sees every element
    for N, S, P in ((6, 4, 1024), (8, 5, 256), (16, 9, 1024)):
        pipe = doa.music_pipeline(N, K, 0, 0, 0.5, 1, P, max_batch=8)
        pipe.set_spatial_smoothing(S, True)
        call("music_pipeline.work_dev",
             [cov_shape(N, K, 0, 0, 3, 0, True), evd_shape(S, 1, 64, 3, cheb=has_cheb(S, 64)), scan_shape(S, 64, P, 3, pick=1, M=1)],
             lambda: pipe.work_dev(3, streams(N, 0, 0), None, spec.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()))
        pipe.close()
    # ---- groups of batches: one lane, so that a call is one group where the shape allows one ----
    n = 17
    variants = ((2, 0, 1), (8, 0, 1), (8, 1, 1), (2, 0, 0))
    # (K = 63: consecutive batches of one buffer lie an odd number of samples apart, so their alignment alternates; with an odd
    # step every batch takes the single loads all the same, and the batches form one group)
    for N, M, P, Kg in ((2, 1, 256, K), (3, 2, 512, K), (4, 1, 1024, K), (4, 3, 256, K), (4, 2, 1024, K), (6, 1, 1024, K), (4, 1, 1024, 63), (3, 1, 256, 63)):
        for nb, off, store in (variants if (N, M, Kg) in ((2, 1, K), (4, 1, K)) else variants[:2] if Kg == 63 else variants[:1]):
            pipe = doa.music_pipeline(N, Kg, 0, 0, 0.5, M, P, max_batch=n)
            pipe.set_lanes(1)
            ins = [[p + b * n * Kg * 8 for p in streams(N, 0, off)] for b in range(nb)]
            specs = [spec.data_ptr() + b * n * P * 4 for b in range(nb)] if store else None
            mx = [outs[0].data_ptr() + b * n * M * 4 for b in range(nb)]
            am = [outs[1].data_ptr() + b * n * M * 4 for b in range(nb)]
            grouped = N <= 4 and (N, M) != (4, 2) and P in (256, 512, 1024)
            if grouped:
                stages = [cov_shape(N, Kg, 0, 0, nb * n, 0, off == 0 and Kg % 2 == 0, group=1), evd_shape(N, M, 64, nb * n, GROUP),
                          scan_shape(N, 64, P, nb * n, pick=1, M=M, store=store, group=1)]
            else:
                stages = nb * [cov_shape(N, Kg, 0, 0, n, 0, off == 0), evd_shape(N, M, 64, n, cheb=has_cheb(N, 64)),
                               scan_shape(N, 64, P, n, pick=1, M=M, store=store)]
            call("music_pipeline.work_dev_batches", stages,
                 lambda: (pipe.work_dev_batches(n, ins, None, specs, mx, am), pipe.synchronize()))
            pipe.close()
    # ---- the census (tests/route_census.py): every kernel the plan can select, through its recipe; one row per recipe ----
    def recipe_call(entry, a):
        """(handle, the call) of a recipe: the entry with the recipe's arguments on the buffers above"""
        N, n = a["N"], a["n"]
        if entry == "autocorrelate.work_dev":
            blk = (doa.autocorrelate_sc16 if a["fmt"] else doa.autocorrelate)(N, a["K"], a["ovl"], a["avg"])
            return blk, lambda: blk.work_dev(n, streams(N, a["fmt"], a["off"]), outs[0].data_ptr())
        if entry.startswith("MUSIC_lin_array."):
            blk = doa.MUSIC_lin_array(0.5, a["M"], N, a["P"])
            blk.set_internal_precision(a["bits"])
            if entry.endswith(".debug"):
                host = cov[N][:n].cpu().numpy()
                return blk, lambda: blk.debug(host)
            if entry.endswith(".work_dev_counts"):
                return blk, lambda: blk.work_dev_counts(n, cov[N].data_ptr(), counts.data_ptr(), spec.data_ptr())
            return blk, lambda: blk.work_dev(n, cov[N].data_ptr(), spec.data_ptr() + a["off"])
        if entry == "root_pipeline[esprit].work_dev_auto":
            blk = doa.root_pipeline(N, a["K"], 0, 0, 0.5, a["M"], max_batch=n)
            blk.set_estimator("esprit")
            return blk, lambda: blk.work_dev_auto(n, streams(N, 0, 0), outs[0].data_ptr(), counts.data_ptr(), d_status_ptr=outs[1].data_ptr())
        if entry == "esprit_linear_array.work_dev":
            blk = doa.esprit_linear_array(0.5, a["M"], N)
            return blk, lambda: blk.work_dev(n, cov[N].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr())
        if entry == "MUSIC_array.work_dev":
            blk = doa.MUSIC_array(a["M"], np.exp(1j * rng.uniform(0, 6.28, (32, N))))
            return blk, lambda: blk.work_dev(n, cov[N].data_ptr(), spec.data_ptr())
        if entry == "calibrate_lin_array.work_dev":
            blk = doa.calibrate_lin_array(0.5, N, 45.0)
            blk.set_internal_precision(a["bits"])
            return blk, lambda: blk.work_dev(n, cov[N].data_ptr(), outs[0].data_ptr())
        if entry == "music_pipeline.work_dev":
            blk = doa.music_pipeline(N, a["K"], 0, 0, 0.5, a["M"], a["P"], max_batch=n)
            blk.set_internal_precision(a["bits"])
            return blk, lambda: blk.work_dev(n, streams(N, 0, 0), None, spec.data_ptr() if a["store"] else None, outs[0].data_ptr(), outs[1].data_ptr())
        assert entry == "music_pipeline.work_dev_batches", entry
        blk = (doa.music_pipeline_sc16 if a["fmt"] else doa.music_pipeline)(N, a["K"], 0, a["avg"], 0.5, a["M"], a["P"], max_batch=n)
        blk.set_lanes(1)
        nb, sb = a["nb"], 4 if a["fmt"] else 8
        ins = [[p + b * n * a["K"] * sb for p in streams(N, a["fmt"], a["off"])] for b in range(nb)]
        specs = [spec.data_ptr() + b * n * a["P"] * 4 for b in range(nb)] if a["store"] else None
        mx = [outs[0].data_ptr() + b * n * a["M"] * 4 for b in range(nb)]
        am = [outs[1].data_ptr() + b * n * a["M"] * 4 for b in range(nb)]
        return blk, lambda: (blk.work_dev_batches(n, ins, None, specs, mx, am), blk.synchronize())

    sys.path.append(os.path.join(ROOT, "tests"))
    import route_census
    for stage, recipes in sorted(route_census.RECIPES.items()):
        for kernel in sorted(recipes):
            r = recipes[kernel]
            blk, fn = recipe_call(r["entry"], r["args"])
            call("census:" + r["entry"], r["stages"], fn)
            blk.close()
    marker.fill_(len(calls))
    torch.cuda.synchronize()
    json.dump({"cu_count": cu, "calls": calls}, open(calls_path, "w"))
    print(f"{len(calls)} calls on {cu} compute units -> {calls_path}")


def write(trace_dir, out_path):
    calls = json.load(open(os.path.join(trace_dir, "calls.json")))
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    trace = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    segments, cur = [], None
    for r in trace:
        if MARKER in r["Kernel_Name"]:
            cur = []
            segments.append(cur)
        elif cur is not None:
            cur.append([r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"])])
    assert len(segments) == len(calls["calls"]) + 1 and not segments[-1], (len(segments), len(calls["calls"]))
    assert all(segments[:-1]), "a call without a kernel"
    names = sorted({k[0] for seg in segments for k in seg})         # each traced name once; the rows hold its index
    rows = [[c["call"], c["stages"], [[names.index(k[0]), k[1], k[2]] for k in seg]] for c, seg in zip(calls["calls"], segments)]
    with open(out_path, "w") as f:
        f.write('{"cu_count": %d,\n"names": [\n' % calls["cu_count"])
        f.write(",\n".join(json.dumps(n) for n in names))
        f.write('\n],\n"rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} rows -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "write":
        write(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
