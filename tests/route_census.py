"""The census of the launch plan: every kernel instantiation gr-doa_amd/csrc/launch_routes.hpp can select for a shape that some
public entry produces, and for each the public call (the recipe) that makes the library launch it.  No device is needed: the
plan is asked through doa_hip_launch_route_debug with the route() helper of tests/test_cpu_launch_routes.py.
tests/test_cpu_route_census.py checks the census and the recipes, tests/test_gpu_route_parity.py runs every recipe against the
fp64 oracle, tools/record_launch_routes.py traces every recipe for tests/golden/launch_routes.json.

THE GRID (stage shapes in the form doa_hip_launch_route_debug takes; M < N everywhere, a pick's M is num_targets):
  K1     N 1..16; (K, overlap) in WINDOWS; fc32 / sc16; streams aligned or offset one sample; avg 0 / 1; 5 snapshots; the
         piece-sum workspace supplied exactly when cov_workspace_bytes is non-zero (the handles do that).  Groups: N 2..4,
         K 64 / 63, both alignments, both formats, both avg, 2 batches of 5.
  eigen  N 2..16, every M < N, 64 / 32 bits, 70 items; Fixed (pn 0 / 1), Counts (the record MUSIC_lin_array asks for, which is
         the Chebyshev one exactly where spectrum_plan has it; and the signal-subspace record), Record, Full, Calibrate,
         Group (2 batches of 5).
  scan   P in LENGTHS (outermost, so that the first P of the list that reaches an instantiation is the one the census keeps:
         ragged lengths first, a partial last chunk wherever the kernel allows one); N 2..16; 64 / 32 bits; 5 items; no pick
         on an aligned row, on a row offset by 4 bytes, with Q; a pick of M in {1, 2} with the row stored or angles only; the
         Chebyshev record supplied exactly where spectrum_plan has it; groups of N 2..4 (M in {1, 2, 3}, not N = 4 with M = 2,
         which no group takes: launch_routes.hpp, group_routes_accept).

census() -> per stage {kernel name: the first grid shape that selects it}.  RECIPES -> per stage {kernel name: recipe}; a
recipe is the entry, its arguments, and the stage shapes the call runs, written down from the arguments alone as
tools/record_launch_routes.py does (no route function is asked); recipe["at"] is the index of the stage the recipe is for.

FINDING: kernels the plan can name for shapes no entry accepts (every entry wants num_targets < inputs, so N = 2 never has two
targets; they are compiled, but nothing public launches them, and they are not in the census):
  music_scan_peak1_kernel<2,CH,T,true,true,STORE,0,ScanOne>   CH in 1, 2, 4; T in double, float; STORE in true, false   (12)
  music_scan_peak1_kernel<2,CH,double,true,true,STORE,0,ScanGroup>   CH in 1, 2, 4; STORE in true, false                  (6)
Nothing else: with M < N the plan's reach and the entries' reach are the same 565 kernels, and UNREACHABLE is empty.

FINDING: a walk of the plan over both precisions in the Counts mode used to name three more eigen kernels,
music_evd_kernel<2|3|4,float,EvdOneCounts>.  They do not exist: the count-per-item form of the one-lane kernel is compiled in
double only (music_evd.hip, launch_evd_one_lane), launch_evd_counts forms its shape at 64 bits whatever the handle's precision,
and every counted entry refuses a handle at 32 bits before it gets there (block_host.hpp, need_bits64).  Only the text of
doa_hip_launch_route_debug said "float"; it now names the kernel launch_evd would launch, and the eigen census is 47, not 50."""
import ctypes as C

from doa import _lib

K1, EVD, SCAN = 0, 1, 2
STAGES = ("K1", "eigen", "scan")
FIXED, COUNTS, RECORD, FULL, CALIBRATE, GROUP = range(6)
CU = 256                            # the routes' kernel names do not depend on it; the grids do, and are not compared here
WINDOWS = ((64, 0), (63, 0), (64, 32), (64, 16), (64, 33))
LENGTHS = (244, 500, 1012, 2036, 4084, 256, 512, 1024, 2048, 2112, 4096, 2500, 3100, 1001, 63, 4100, 8192, 16384)
N_K1, N_EVD, N_SCAN, GROUP_BATCHES = 5, 70, 5, 2
D = 0.5                             # element spacing of every recipe, in wavelengths

# {stage: {kernel name: "file:line of the host check that refuses every shape that would launch it"}}; at most 5 % of a stage
UNREACHABLE = {K1: {}, EVD: {}, SCAN: {}}


def route(stage, shape, cu=CU):
    """-> (status or number of launches, [(kernel, grid, block, lanes, work, strides)], {further facts})"""
    text = C.create_string_buffer(2048)
    arr = (C.c_int * len(shape))(*[int(v) for v in shape])
    rc = _lib.lib.doa_hip_launch_route_debug(stage, arr, len(shape), cu, text, len(text))
    launches, facts = [], {}
    if rc >= 0:
        for line in text.value.decode().splitlines():
            f = line.split(" ")
            if len(f) == 6:
                launches.append((f[0],) + tuple(int(v) for v in f[1:]))
            else:
                assert len(f) == 2, line
                facts[f[0]] = int(f[1])
        assert rc == len(launches) and rc >= 1, text.value
    return rc, launches, facts


def family(kernel):
    return kernel.split("<")[0]


# ---- stage shapes from a call's arguments (as tools/record_launch_routes.py writes them) ---------------------------------------
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


# ---- the grid --------------------------------------------------------------------------------------------------------------------
def grid(stage):
    """the stage's grid, in census order"""
    if stage == K1:
        for N in range(1, 17):
            for K, ovl in WINDOWS:
                for fmt in (0, 1):
                    for pair in (1, 0):
                        for avg in (0, 1):
                            yield cov_shape(N, K, ovl, avg, N_K1, fmt, pair)[1]
        for N in (2, 3, 4):
            for K in (64, 63):
                for fmt in (0, 1):
                    for pair in (1, 0):
                        for avg in (0, 1):
                            yield cov_shape(N, K, 0, avg, GROUP_BATCHES * N_K1, fmt, pair, group=1)[1]
    elif stage == EVD:
        for N in range(2, 17):
            for M in range(1, N):
                for bits in (64, 32):
                    for pn in (0, 1):
                        yield evd_shape(N, M, bits, N_EVD, FIXED, pn, has_cheb(N, bits))[1]
                    yield evd_shape(N, 0, bits, N_EVD, COUNTS, cheb=has_cheb(N, bits))[1]
                    yield evd_shape(N, 0, bits, N_EVD, COUNTS, es=1)[1]
                    for mode in (RECORD, FULL, CALIBRATE):
                        yield evd_shape(N, M, bits, N_EVD, mode)[1]
                    yield evd_shape(N, M, bits, GROUP_BATCHES * N_SCAN, GROUP)[1]
    else:
        for P in LENGTHS:
            for N in range(2, 17):
                for bits in (64, 32):
                    yield scan_shape(N, bits, P, N_SCAN)[1]
                    yield scan_shape(N, bits, P, N_SCAN, aligned=0)[1]
                    yield scan_shape(N, bits, P, N_SCAN, q=1)[1]
                    for M in (1, 2):
                        for store in (1, 0):
                            if M < N:
                                yield scan_shape(N, bits, P, N_SCAN, pick=1, M=M, store=store)[1]
                    for M in (1, 2, 3):
                        for store in (1, 0):
                            if M < N and (N, M) != (4, 2):
                                yield scan_shape(N, bits, P, GROUP_BATCHES * N_SCAN, pick=1, M=M, store=store, group=1)[1]


def census():
    """-> {stage: {kernel name: the first grid shape that selects it}} (shapes the plan refuses select nothing)"""
    out = {}
    for stage in (K1, EVD, SCAN):
        found = out.setdefault(stage, {})
        for shape in grid(stage):
            rc, launches, _ = route(stage, shape)
            for launch in launches if rc >= 1 else ():
                found.setdefault(launch[0], shape)
    return out


# ---- the recipes -----------------------------------------------------------------------------------------------------------------
def stages_of(entry, a):
    """the routed stages a public call runs, from its arguments"""
    if entry == "autocorrelate.work_dev":
        return [cov_shape(a["N"], a["K"], a["ovl"], a["avg"], a["n"], a["fmt"], a["off"] == 0)]
    if entry == "MUSIC_lin_array.work_dev":
        return [evd_shape(a["N"], a["M"], a["bits"], a["n"], cheb=has_cheb(a["N"], a["bits"])),
                scan_shape(a["N"], a["bits"], a["P"], a["n"], aligned=a["off"] == 0)]
    if entry == "MUSIC_lin_array.debug":
        return [evd_shape(a["N"], a["M"], a["bits"], a["n"], pn=1, cheb=has_cheb(a["N"], a["bits"])),
                scan_shape(a["N"], a["bits"], a["P"], a["n"], q=1)]
    if entry == "MUSIC_lin_array.work_dev_counts":
        return [evd_shape(a["N"], 0, a["bits"], a["n"], COUNTS, cheb=has_cheb(a["N"], a["bits"])), scan_shape(a["N"], a["bits"], a["P"], a["n"])]
    if entry == "root_pipeline[esprit].work_dev_auto":
        return [cov_shape(a["N"], a["K"], 0, 0, a["n"], 0, True), evd_shape(a["N"], 0, 64, a["n"], COUNTS, es=1)]
    if entry == "esprit_linear_array.work_dev":
        return [evd_shape(a["N"], a["M"], 64, a["n"], RECORD)]
    if entry == "MUSIC_array.work_dev":
        return [evd_shape(a["N"], a["M"], 64, a["n"], FULL)]
    if entry == "calibrate_lin_array.work_dev":
        return [evd_shape(a["N"], 1, a["bits"], a["n"], CALIBRATE)]
    if entry == "music_pipeline.work_dev":
        return [cov_shape(a["N"], a["K"], 0, 0, a["n"], 0, True), evd_shape(a["N"], a["M"], a["bits"], a["n"], cheb=has_cheb(a["N"], a["bits"])),
                scan_shape(a["N"], a["bits"], a["P"], a["n"], pick=1, M=a["M"], store=a["store"])]
    if entry == "music_pipeline.work_dev_batches":          # one lane: the batches are one group
        total = a["nb"] * a["n"]
        return [cov_shape(a["N"], a["K"], 0, a["avg"], total, a["fmt"], a["off"] == 0 and a["K"] % 2 == 0, group=1),
                evd_shape(a["N"], a["M"], 64, total, GROUP), scan_shape(a["N"], 64, a["P"], total, pick=1, M=a["M"], store=a["store"], group=1)]
    raise KeyError(entry)


def recipe_for(stage, kernel, shape):
    """the public call that produces a grid shape: (entry, arguments, index of the stage among the call's stages)"""
    if stage == K1:
        N, K, ovl, avg, n_out, fmt, pair, _ws, group = shape
        if group:       # (K = 63: consecutive batches lie an odd number of samples apart; with an odd step all take single loads)
            return "music_pipeline.work_dev_batches", dict(N=N, M=1, P=256, K=K, avg=avg, fmt=fmt, off=0 if pair or K % 2 else 1, store=1,
                                                           nb=GROUP_BATCHES, n=n_out // GROUP_BATCHES), 0
        return "autocorrelate.work_dev", dict(N=N, K=K, ovl=ovl, avg=avg, fmt=fmt, off=0 if pair else 1, n=n_out), 0
    if stage == EVD:
        N, M, bits, n, mode, pn, _cheb, es = shape
        if mode == FIXED:
            return "MUSIC_lin_array.debug" if pn else "MUSIC_lin_array.work_dev", dict(N=N, M=M, bits=bits, P=64, n=n, off=0), 0
        if mode == COUNTS and es:
            return "root_pipeline[esprit].work_dev_auto", dict(N=N, M=min(2, N - 1), K=64, n=n), 1
        if mode == COUNTS:
            return "MUSIC_lin_array.work_dev_counts", dict(N=N, M=1, bits=bits, P=64, n=n), 0
        if mode == GROUP:
            return "music_pipeline.work_dev_batches", dict(N=N, M=M, P=256, K=64, avg=0, fmt=0, off=0, store=1, nb=GROUP_BATCHES, n=n // GROUP_BATCHES), 1
        entry = {RECORD: "esprit_linear_array.work_dev", FULL: "MUSIC_array.work_dev", CALIBRATE: "calibrate_lin_array.work_dev"}[mode]
        return entry, dict(N=N, M=M, bits=bits, n=n), 0
    N, bits, P, n, aligned, q, pick, M, store, _cheb, group = shape
    if group:
        return "music_pipeline.work_dev_batches", dict(N=N, M=M, P=P, K=64, avg=0, fmt=0, off=0, store=store, nb=GROUP_BATCHES, n=n // GROUP_BATCHES), 2
    if pick:
        return "music_pipeline.work_dev", dict(N=N, M=M, P=P, K=64, bits=bits, store=store, n=n), 2
    return "MUSIC_lin_array.debug" if q else "MUSIC_lin_array.work_dev", dict(N=N, M=1, bits=bits, P=P, n=n, off=0 if aligned else 4), 1


def recipes():
    out = {}
    for stage, kernels in census().items():
        for kernel, shape in kernels.items():
            if kernel in UNREACHABLE[stage]:
                continue
            entry, args, at = recipe_for(stage, kernel, shape)
            out.setdefault(stage, {})[kernel] = dict(kernel=kernel, stage=stage, entry=entry, args=args, stages=stages_of(entry, args), at=at)
    return out


RECIPES = recipes()
