"""The refusals of the entries that take "a snapshot of bins" (csrc/bin_plan.hpp states their shared rules once): the return
value and the exact doa_last_error text of every bad argument tuple below are those of the library as it was before the rules
were shared (tests/golden/bin_plan_refusals.json, recorded at the commit the file names).  A tuple that breaks two rules pins
the order of the checks as well.  Every create tuple is refused before a device is looked for, so this runs without one; the
refusals that need a handle (channel_covariance's set_bins, the call-size limit of the two work_dev entries) are in the same
file and are compared by tests/test_cpu_channel_covariance.py and tests/test_gpu_bin_rule.py.

The fixture is written by `python tests/test_cpu_bin_plan_refusals.py record <commit>` with DOA_HIP_LIB naming a build of that
commit, never from the library under test: without a device it records the create tuples and keeps the handle section it
finds, with a device it records both."""
import ctypes as C
import json
import os
import sys

import numpy as np

if __name__ == "__main__":                                      # recording: the paths tests/conftest.py sets for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_root, "gr-doa_amd", "python"))

from doa import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bin_plan_refusals.json")
NAN, INF = float("nan"), float("inf")

# doa_wideband_music_create(norm_spacing, num_targets, num_ant_ele, pspectrum_len, fft_len, first_bin, num_bins, rate_over_carrier, combine)
WB = "doa_wideband_music_create"
# doa_rss_focusing_matrices(norm_spacing, num_ant_ele, fft_len, first_bin, num_bins, rate_over_carrier, n_focus, angles, regularization, out)
# angles: a list, or None for NULL; out: "out" for a buffer large enough, or None
RSS = "doa_rss_focusing_matrices"
# doa_focus_covariance_create(num_ant_ele, num_bins, matrices); matrices: "eye", "nan5" (bin slot 5 has a NaN) or None
FC = "doa_focus_covariance_create"
# doa_channel_covariance_create(inputs, snapshot_size, overlap_size, fft_len, window = NULL)
CC = "doa_channel_covariance_create"

CASES = [
    # ---- wideband_music: each rule alone --------------------------------------------------------------------------------
    (WB, (0.0, 1, 4, 64, 16, 0, 16, 0.4, 0)),                   # the spacing at the carrier
    (WB, (0.6, 1, 4, 64, 16, 0, 16, 0.4, 0)),
    (WB, (NAN, 1, 4, 64, 16, 0, 16, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 8, 0, 8, 0.4, 0)),                     # the transform size: the neighbours of the five good ones
    (WB, (0.4, 1, 4, 64, 48, 0, 8, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 512, 0, 8, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 0, 0, 1, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, -16, 0, 1, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 16, 16, 1, 0.4, 0)),                   # the five good sizes pass that check: the selection is refused
    (WB, (0.4, 1, 4, 64, 32, 32, 1, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 64, 64, 1, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 128, 128, 1, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 256, 256, 1, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 16, -1, 4, 0.4, 0)),                   # the selection
    (WB, (0.4, 1, 4, 64, 16, 0, 0, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 16, 3, 17, 0.4, 0)),
    (WB, (0.4, 1, 4, 64, 16, 0, 16, -0.1, 0)),                  # the band
    (WB, (0.4, 1, 4, 64, 16, 0, 16, NAN, 0)),
    (WB, (0.4, 1, 4, 64, 16, 0, 16, INF, 0)),
    (WB, (0.4, 1, 4, 64, 64, 0, 64, 3.0, 0)),                   # the spacing at a bin: too wide first in bin 6
    (WB, (0.5, 1, 4, 64, 64, 0, 64, 0.4, 0)),                   # bin 1
    (WB, (0.4, 1, 4, 64, 64, 32, 8, 3.0, 0)),                   # not positive at bin 32
    (WB, (0.4, 1, 4, 64, 64, 62, 12, 3.0, 0)),                  # a selection that wraps: 62, 63 and 0..5 pass, bin 6 does not
    # ---- wideband_music: two rules at once, the first in the entry's order is reported ---------------------------------
    (WB, (0.6, 1, 4, 64, 48, 0, 8, 0.4, 0)),                    # spacing, then fft_len
    (WB, (0.4, 1, 4, 0, 16, 0, 16, -1.0, 0)),                   # pspectrum_len, then the band
    (WB, (0.4, 1, 4, 64, 48, 48, 0, 0.4, 0)),                   # fft_len, then the selection
    (WB, (0.4, 1, 4, 64, 16, 16, 1, INF, 0)),                   # the selection, then the band
    (WB, (0.4, 1, 4, 64, 16, 0, 16, -0.1, 7)),                  # the band, then combine
    (WB, (0.4, 1, 4, 64, 64, 0, 64, 3.0, 7)),                   # a bin's spacing, then combine
    (WB, (0.0, 4, 4, 0, 48, -1, 0, NAN, 7)),                    # everything: the source count comes first
    # ---- rss_focusing_matrices ------------------------------------------------------------------------------------------
    (RSS, (0.0, 4, 64, 0, 64, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.6, 4, 64, 0, 64, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 8, 0, 8, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 48, 0, 8, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 512, 0, 8, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 16, 16, 1, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 32, 32, 1, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, 64, 1, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 128, 128, 1, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 256, 256, 1, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, -1, 4, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, 0, 65, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, 0, 64, -0.1, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, 0, 64, NAN, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, 0, 64, 3.0, 1, [60.0], 1e-3, "out")),
    (RSS, (0.5, 4, 64, 0, 64, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 4, 64, 32, 8, 3.0, 1, [60.0], 1e-3, "out")),
    (RSS, (0.4, 17, 64, 0, 64, 0.4, 1, [60.0], 1e-3, "out")),
    (RSS, (0.6, 1, 48, 0, 8, 0.4, 1, [60.0], 1e-3, "out")),    # num_ant_ele, then spacing, then fft_len
    (RSS, (0.6, 4, 48, 0, 8, 0.4, 1, [60.0], 1e-3, "out")),    # spacing, then fft_len
    (RSS, (0.4, 4, 48, 48, 0, 0.4, 1, [60.0], 1e-3, "out")),   # fft_len, then the selection
    (RSS, (0.4, 4, 64, 64, 1, -0.1, 1, [60.0], 1e-3, "out")),  # the selection, then the band
    (RSS, (0.4, 4, 64, 0, 64, -0.1, 0, [], 1e-3, "out")),      # the band, then n_focus
    (RSS, (0.4, 4, 64, 0, 64, 3.0, 0, [], 1e-3, "out")),       # n_focus, then a bin's spacing
    (RSS, (0.4, 4, 64, 0, 64, 3.0, 1, None, 1e-3, "out")),     # a NULL pointer, then a bin's spacing
    (RSS, (0.4, 4, 64, 0, 64, 3.0, 1, [NAN], 1e-3, "out")),    # a focus angle, then a bin's spacing
    (RSS, (0.4, 4, 64, 0, 64, 3.0, 1, [60.0], 0.0, "out")),    # the regularization, then a bin's spacing
    # ---- focus_covariance: its table of num_bins matrices ---------------------------------------------------------------
    (FC, (1, 8, "eye")),
    (FC, (17, 8, "eye")),
    (FC, (4, 0, "eye")),
    (FC, (4, 257, "eye")),
    (FC, (4, 8, None)),
    (FC, (4, 8, "nan5")),
    (FC, (1, 0, None)),                                         # num_ant_ele, then num_bins, then the table
    (FC, (4, 257, None)),                                       # num_bins, then the table
    # ---- channel_covariance ---------------------------------------------------------------------------------------------
    (CC, (4, 1024, 0, 8)),
    (CC, (4, 1024, 0, 48)),
    (CC, (4, 1024, 0, 512)),
    (CC, (4, 1024, 0, 0)),
    (CC, (4, 1024, 0, -16)),
    (CC, (4, 17, 0, 16)),                                       # the five good sizes pass that check: the snapshot is refused
    (CC, (4, 33, 0, 32)),
    (CC, (4, 65, 0, 64)),
    (CC, (4, 129, 0, 128)),
    (CC, (4, 257, 0, 256)),
    (CC, (0, 1024, 0, 48)),                                     # inputs and fft_len share a message
    (CC, (9, 1024, 0, 48)),                                     # a size that is not built in, then fft_len
    (CC, (4, 100, 100, 48)),                                    # fft_len, then the snapshot
]

# (first_bin, num_bins) of doa_channel_covariance_set_bins on a handle with fft_len 64: tests/test_cpu_channel_covariance.py
SET_BINS = [(-1, 4), (64, 1), (0, 0), (0, 65), (3, -2)]
# (entry, snapshots) on a handle of 16 bins: 2^27 snapshots of 16 bins are 2^31 items.  tests/test_gpu_bin_rule.py
CALL_SIZE = [("doa_wideband_music_work_dev", 1 << 27), ("doa_focus_covariance_work_dev", 1 << 27)]


def case_key(entry, args) -> str:
    return f"{entry}{args!r}"


def call_case(entry, args):
    """The entry on the tuple: (return value or None for NULL, doa_last_error).  A handle, which no tuple here gives, is destroyed."""
    lib = _lib.lib
    keep = []                                                   # the arrays behind the pointers
    if entry == RSS:
        *head, angles, reg, out = args
        a = None if angles is None else np.array(angles, np.float64)
        o = None if out is None else np.empty(2 * 256 * 16 * 16, np.float64)
        keep += [a, o]
        ret = lib.doa_rss_focusing_matrices(*head, None if a is None else a.ctypes.data, reg, None if o is None else o.ctypes.data)
        return int(ret), _lib.last_error()
    if entry == FC:
        N, nb, table = args
        t = None
        if table is not None:
            t = np.broadcast_to(np.eye(max(N, 1), dtype=np.complex128), (max(nb, 1), max(N, 1), max(N, 1))).copy()
            if table == "nan5":
                t[5, 1, 2] = np.nan
        keep.append(t)
        h = lib.doa_focus_covariance_create(N, nb, None if t is None else t.ctypes.data)
        destroy = lib.doa_focus_covariance_destroy
    elif entry == CC:
        h = lib.doa_channel_covariance_create(*args, None)
        destroy = lib.doa_channel_covariance_destroy
    else:
        h = lib.doa_wideband_music_create(*args)
        destroy = lib.doa_wideband_music_destroy
    err = _lib.last_error()
    if h:
        destroy(h)
    return (int(h) if h else None), err


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_table_covers_every_entry_and_the_fixture_covers_the_table():
    fx = load_fixture()
    assert len(CASES) >= 40 and len({case_key(*c) for c in CASES}) == len(CASES)
    assert {c[0] for c in CASES} == {WB, RSS, FC, CC}
    assert sorted(fx["create"]) == sorted(case_key(*c) for c in CASES)
    for entry in (WB, RSS, CC):                                 # the five good transform sizes and their neighbours
        sizes = {c[1][{WB: 4, RSS: 2, CC: 3}[entry]] for c in CASES if c[0] == entry}
        assert {16, 32, 64, 128, 256, 8, 48, 512} <= sizes, entry
    assert len(fx["recorded_at"]) >= 7


def test_every_refusal_is_the_recorded_one():
    fx = load_fixture()["create"]
    wrong = []
    for entry, args in CASES:
        ret, err = call_case(entry, args)
        want_ret, want_err = fx[case_key(entry, args)]
        assert want_err and "no HIP device" not in want_err and want_ret in (None, -1), (entry, args)   # a refusal of the arguments
        if (ret, err) != (want_ret, want_err):
            wrong.append((entry, args, ret, err, want_ret, want_err))
    assert not wrong, wrong


def record(commit):
    """Writes the fixture from the library that is loaded (DOA_HIP_LIB): run by hand, on a build of the parent commit only."""
    import doa
    try:
        old = load_fixture()
    except FileNotFoundError:
        old = {}
    fx = {"recorded_at": commit,
          "create": {case_key(e, a): list(call_case(e, a)) for e, a in CASES},
          "set_bins": old.get("set_bins", {}), "call_size": old.get("call_size", {})}
    if doa.device_count() > 0:
        lib = _lib.lib
        h = lib.doa_channel_covariance_create(4, 1024, 0, 64, None)
        assert h, _lib.last_error()
        fx["set_bins"] = {repr(t): [int(lib.doa_channel_covariance_set_bins(h, *t)), _lib.last_error()] for t in SET_BINS}
        lib.doa_channel_covariance_destroy(h)
        fx["call_size"] = {entry: list(call_size_case(entry, n)) for entry, n in CALL_SIZE}
    out = os.environ.get("BIN_PLAN_FIXTURE_OUT", FIXTURE)
    with open(out, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(fx['create'])} create tuples, {len(fx['set_bins'])} set_bins tuples, {len(fx['call_size'])} call sizes -> {out}")


def call_size_case(entry, n):
    """The work_dev entry of a handle of 16 bins asked for n snapshots: (return value, doa_last_error).  The pointers are
    never read: the call is refused on its sizes (needs a device for the handle)."""
    lib = _lib.lib
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    if entry == "doa_wideband_music_work_dev":
        h = lib.doa_wideband_music_create(0.4, 1, 4, 64, 16, 0, 16, 0.4, 0)
        assert h, _lib.last_error()
        ret = lib.doa_wideband_music_work_dev(h, n, p, None, p, None, None, None)
        err = _lib.last_error()
        lib.doa_wideband_music_destroy(h)
    else:
        t = np.broadcast_to(np.eye(4, dtype=np.complex128), (16, 4, 4)).copy()
        h = lib.doa_focus_covariance_create(4, 16, t.ctypes.data)
        assert h, _lib.last_error()
        ret = lib.doa_focus_covariance_work_dev(h, n, p, None, p, None, None)
        err = _lib.last_error()
        lib.doa_focus_covariance_destroy(h)
    return int(ret), err


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "record", "usage: test_cpu_bin_plan_refusals.py record <commit>"
    record(sys.argv[2])
