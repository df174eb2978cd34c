"""Which kernel a shape launches, and with which grid (gr-doa_amd/csrc/launch_routes.hpp: cov_route, evd_route, scan_route),
through doa_hip_launch_route_debug.  No device is needed.

Two kinds of test.  The golden rows (tests/golden/launch_routes.json, written by tools/record_launch_routes.py from a kernel
trace of the public entries on the device, never by hand) pin the routes to what the library really launched: same kernels of
the three stages in the same order, same template arguments, grids and workgroup sizes, at the recorded compute-unit count.
The property tests need no recorded data and run over every array size, source count, precision and spectrum length."""
import ctypes as C
import itertools
import json
import os
import re

import pytest

from doa import _lib

DOA_OK, DOA_ERR_INVALID_ARG, DOA_ERR_UNSUPPORTED = 0, -1, -4
K1, EVD, SCAN = 0, 1, 2
FIXED, COUNTS, RECORD, FULL, CALIBRATE, GROUP = range(6)
SIZES = range(2, 17)
LENGTHS = (64, 100, 256, 512, 1024, 2048, 4096, 4160, 8192)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_routes.json")


def route(stage, shape, cu=256):
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


def cov_shape(N, K=64, ovl=0, avg=0, n_out=3, fmt=0, pair=1, ws=0, group=0):
    return [N, K, ovl, avg, n_out, fmt, pair, ws, group]


def evd_shape(N, M, bits=64, n=70, mode=FIXED, pn=0, cheb=0, es=0):
    return [N, M, bits, n, mode, pn, cheb, es]


def scan_shape(N, bits=64, P=1024, n=70, aligned=1, q=0, pick=0, M=0, store=1, cheb=1, group=0):
    return [N, bits, P, n, aligned, q, pick, M, store, cheb, group]


def wave_cap(kernel, cu, work):
    """the most waves a launch of a striding kernel may hold, from DESIGN.md section 3 (None: no cap).  K1: 16 waves per CU up to
    four elements and on the matrix cores, 8 for five to eight, none for a group; scan: 8, the LDS-row kernel two workgroups
    per CU, the rolled two-pass kernel 16, the lean kernel 12 and from four items per wave at 16 waves per CU on 16"""
    name, _, args = kernel.partition("<")
    args = args.rstrip(">").split(",")
    if name in ("cov_wave_kernel", "cov_piece_kernel"):
        return None if args[-1] == "CovGroupArgs" else cu * (16 if int(args[1]) <= 4 else 8)
    if name == "music_scan_peak1_kernel":
        return cu * (16 if work // (16 * cu) >= 4 else 12)
    return cu * {"cov_mfma_kernel": 16, "music_scan_peak_long_kernel": 8, "music_scan_stream_kernel": 16, "music_scan_kernel": 8,
                 "music_scan_generic_kernel": 8}[name]


def well_formed(launches, cu=256):
    for kernel, grid, block, lanes, work, strides in launches:
        assert grid > 0 and block in (64, 128, 192, 256) and 1 <= lanes <= 64 and work >= 1, launches
        assert re.fullmatch(r"\w+(<[\w,]+>)?", kernel), kernel
        slots = grid * block // lanes                   # work items in flight at once
        if not strides:                                 # one slot per work item, and no workgroup without one
            assert slots >= work > (grid - 1) * block // lanes, (kernel, grid, block, lanes, work)
            continue
        # a striding kernel: one wave per item up to its cap, never a workgroup more than the work needs
        assert lanes == 64 and block == 256
        cap, per_block = wave_cap(kernel, cu, work), block // 64
        want = -(-work // per_block)
        if cap is not None and want > cap // per_block:
            want = cap // per_block
            if kernel.startswith("music_scan_peak1_kernel<"):       # every wave the same number of items, in as few rounds as the cap allows
                rounds = -(-work // cap)
                want = -(-(-(-work // rounds)) // per_block)
                assert slots * rounds >= work > (slots - per_block) * rounds, (kernel, grid, work)
        assert grid == want, (kernel, grid, block, work, cu)


# ---- the golden rows --------------------------------------------------------------------------------------------------------
STAGE_KERNELS = re.compile(r"^(void)?(cov_|music_evd_|music_scan_)")


def normalised(traced):
    """a kernel name as traced, without namespaces and white space (nothing else is dropped)"""
    return re.sub(r"\s+", "", re.sub(r"\b\w+::", "", traced))


def same_kernel(traced, routed):
    t = normalised(traced)
    return t == routed or t.startswith(("void" if "<" in routed else "") + routed + "(")


def test_golden_rows_match_the_routes():
    assert os.path.exists(GOLDEN), "tests/golden/launch_routes.json is missing: tools/record_launch_routes.py writes it on the device"
    gold = json.load(open(GOLDEN))
    cu, names = gold["cu_count"], gold["names"]
    assert cu >= 1 and len(gold["rows"]) >= 100
    for call, stages, kernels in gold["rows"]:
        expected = []
        for stage, shape in stages:
            rc, launches, _ = route(stage, shape, cu)
            assert rc >= 1, (call, stage, shape, _lib.last_error())
            expected += launches
        traced = [(names[k], g, wg) for k, g, wg in kernels if STAGE_KERNELS.match(normalised(names[k]))]
        assert len(traced) == len(expected), (call, stages, [k[0] for k in traced], [e[0] for e in expected])
        for (name, grid_threads, wg), (kernel, grid, block, *_rest) in zip(traced, expected):
            assert same_kernel(name, kernel), (call, stages, name, kernel)
            assert wg == block and grid_threads == grid * block, (call, stages, name, grid_threads, wg, grid, block)


# ---- properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (64, 32))
def test_every_shape_has_exactly_one_eigen_route_or_a_refusal(bits):
    for N in SIZES:
        for M in range(1, N):
            for mode, pn, cheb, es in [(FIXED, 0, 0, 0), (FIXED, 1, 0, 0), (COUNTS, 0, 0, 0), (COUNTS, 0, 1, 0), (COUNTS, 0, 0, 1), (COUNTS, 0, 1, 1),
                                       (RECORD, 0, 0, 0), (FULL, 0, 0, 0), (CALIBRATE, 0, 0, 0), (GROUP, 0, 0, 0)]:
                for n in (1, 70):
                    rc, launches, facts = route(EVD, evd_shape(N, M, bits, n, mode, pn, cheb, es))
                    if rc < 0:
                        assert rc in (DOA_ERR_INVALID_ARG, DOA_ERR_UNSUPPORTED) and _lib.last_error()
                        # the refusals: a group outside N <= 4 / double / not (4, 2); both records from the 4-lane count form
                        assert (mode == GROUP and (N > 4 or bits == 32 or (N, M) == (4, 2))) or (mode == COUNTS and N <= 4 and cheb and es), (N, M, mode)
                        continue
                    assert rc == 1 and set(facts) == {"counts_fallbacks"}
                    well_formed(launches)
    for N in (0, 1, 17):
        for mode in (FIXED, COUNTS, RECORD, FULL):
            assert route(EVD, evd_shape(N, 1, bits, 70, mode))[0] == DOA_ERR_UNSUPPORTED
        assert route(EVD, evd_shape(N, 1, bits, 70, GROUP))[0] == DOA_ERR_INVALID_ARG


@pytest.mark.parametrize("bits", (64, 32))
def test_every_shape_has_exactly_one_scan_route_or_a_refusal(bits):
    for N, P in itertools.product(SIZES, LENGTHS):
        for aligned, q, pick, M, store, cheb in [(1, 0, 0, 0, 1, 1), (1, 0, 1, 1, 1, 1), (1, 0, 1, 2, 1, 1), (1, 0, 1, 1, 0, 1), (1, 0, 1, 2, 0, 1),
                                                  (1, 1, 0, 0, 1, 1), (1, 1, 1, 1, 1, 1), (0, 0, 1, 1, 1, 1), (1, 0, 1, 1, 1, 0)]:
            for n in (3, 4096):
                rc, launches, facts = route(SCAN, scan_shape(N, bits, P, n, aligned, q, pick, M, store, cheb))
                assert rc == 1 and set(facts) == {"reads_cheb", "picked"}, (N, P, _lib.last_error())
                well_formed(launches)
                assert not facts["picked"] or pick              # a pick nobody asked for never runs
    for N in (0, 1, 17):
        assert route(SCAN, scan_shape(N, bits))[0] == DOA_ERR_UNSUPPORTED


def plan_has_cheb(N, bits):
    out = (C.c_longlong * 5)()
    assert _lib.lib.doa_hip_spectrum_plan_debug(0, 0, N, bits, 0, out) == DOA_OK
    return out[1] > 0


@pytest.mark.parametrize("bits", (64, 32))
def test_the_scan_reads_the_chebyshev_record_exactly_when_the_plan_has_one(bits):
    """The lean kernel is the one reader of the record.  On its shapes (the three lengths, an aligned row, no diagnostics) the
    route reads the record exactly when spectrum_plan sizes one; a supplied record is what makes those shapes lean where the
    plan has one; no other kernel ever reads it."""
    for N, P in itertools.product(SIZES, LENGTHS):
        for pick in (0, 1):
            _, launches, facts = route(SCAN, scan_shape(N, bits, P, 70, 1, 0, pick, pick, 1, 1))
            lean = launches[0][0].startswith("music_scan_peak1_kernel<")
            if P in (256, 512, 1024) and N in (2, 3, 4, 6, 8, 12, 16):
                assert lean and facts["reads_cheb"] == int(plan_has_cheb(N, bits)), (N, P)
            else:
                assert not lean and not facts["reads_cheb"], (N, P)
            # without a record the shapes whose plan has one leave the lean kernel; the others do not notice
            _, launches0, facts0 = route(SCAN, scan_shape(N, bits, P, 70, 1, 0, pick, pick, 1, 0))
            assert not facts0["reads_cheb"]
            assert (launches0 == launches) == (not (lean and plan_has_cheb(N, bits))), (N, P)


def test_group_mode_accepts_exactly_the_shapes_work_dev_batches_groups():
    """N <= 4, double, not N = 4 with two sources, P = 256 / 512 / 1024: both group modes have to accept"""
    for N, bits, P in itertools.product(SIZES, (64, 32), LENGTHS):
        for M in range(1, N):
            evd_ok = route(EVD, evd_shape(N, M, bits, 70, GROUP))[0] == 1
            rc, launches, facts = route(SCAN, scan_shape(N, bits, P, 70, 1, 0, 1, M, 1, 1, 1))
            scan_ok = rc == 1
            assert (evd_ok and scan_ok) == (N <= 4 and bits == 64 and (N, M) != (4, 2) and P in (256, 512, 1024)), (N, M, bits, P)
            if scan_ok:
                assert facts == {"reads_cheb": 1, "picked": 1} and launches[0][0].endswith(",ScanGroup>")
    # a group without its records, or with a row that is not 16-byte aligned, is refused
    assert route(SCAN, scan_shape(4, 64, 1024, 70, 1, 0, 1, 1, 1, 0, 1))[0] == DOA_ERR_INVALID_ARG
    assert route(SCAN, scan_shape(4, 64, 1024, 70, 0, 0, 1, 1, 1, 1, 1))[0] == DOA_ERR_INVALID_ARG
    for N in range(1, 17):
        assert (route(K1, cov_shape(N, group=1))[0] >= 1) == (2 <= N <= 4)


@pytest.mark.parametrize("fmt", (0, 1))
def test_every_covariance_shape_has_one_route(fmt):
    for N in range(1, 17):
        for (K, ovl), pair, ws, avg, n_out in itertools.product([(64, 0), (63, 0), (64, 32), (64, 16), (64, 33)], (0, 1), (0, 1), (0, 1), (3, 4096, 5000)):
            rc, launches, facts = route(K1, cov_shape(N, K, ovl, avg, n_out, fmt, pair, ws))
            assert rc >= 1 and set(facts) == {"workspace_bytes"}, _lib.last_error()
            well_formed(launches)
            S = K - ovl
            wants_ws = ovl > 0 and N <= 8 and S % 2 == 0 and (K % S) % 2 == 0
            assert facts["workspace_bytes"] == ((n_out + K // S) * 2 * N * N * 8 if wants_ws else 0)
            pieces = launches[0][0].startswith("cov_piece_kernel<")
            assert pieces == bool(wants_ws and ws and pair) and (len(launches) == 2) == (pieces or (N > 8 and avg == 1))
            assert launches[0][0].split("<")[0] == ("cov_piece_kernel" if pieces else "cov_wave_kernel" if N <= 8 else "cov_mfma_kernel")


@pytest.mark.parametrize("cu", (1, 304))
def test_routes_are_well_formed_at_other_compute_unit_counts(cu):
    for N in range(1, 17):
        for n_out in (1, 3, 4096, 100000):
            for ovl, ws in ((0, 0), (32, 1)):
                well_formed(route(K1, cov_shape(N, 64, ovl, 1, n_out, 0, 1, ws), cu)[1], cu)
    for N, P, n in itertools.product(SIZES, LENGTHS, (1, 3, 4096, 16384, 100000)):
        for bits, pick in ((64, 1), (32, 0)):
            rc, launches, _ = route(SCAN, scan_shape(N, bits, P, n, 1, 0, pick, pick), cu)
            assert rc == 1
            well_formed(launches, cu)
    # the caps: a launch never holds more workgroups than its waves-per-CU cap allows, and the lean kernel's trim keeps every
    # wave's share equal: 4096 items on a cap of 3072 waves are 2048 waves of two
    (_, grid, block, *_r), = route(SCAN, scan_shape(4, 64, 1024, 4096, 1, 0, 1, 1), 256)[1]
    assert (grid, block) == (512, 256)
    (_, grid, block, *_r), = route(SCAN, scan_shape(4, 64, 256, 16384, 1, 0, 1, 1), 256)[1]
    assert grid * block // 64 == 4096                      # 16 waves per CU from four items per wave on
    (_, grid, block, *_r), = route(K1, cov_shape(4, n_out=5000), 256)[1]
    assert grid == 256 * 16 // 4


def test_bad_arguments():
    f = _lib.lib.doa_hip_launch_route_debug
    text = C.create_string_buffer(256)
    ok = (C.c_int * 9)(*cov_shape(4))
    for args in [(3, ok, 9, 256, text, 256), (-1, ok, 9, 256, text, 256), (K1, None, 9, 256, text, 256), (K1, ok, 8, 256, text, 256),
                 (K1, ok, 9, 0, text, 256), (K1, ok, 9, 256, None, 256), (K1, ok, 9, 256, text, 0), (K1, ok, 9, 256, text, 8)]:
        assert f(*args) == DOA_ERR_INVALID_ARG, args
        assert "hip_launch_route_debug" in _lib.last_error()
    bad_mode = (C.c_int * 8)(*evd_shape(4, 1, mode=6))
    assert f(EVD, bad_mode, 8, 256, text, 256) == DOA_ERR_INVALID_ARG
