"""The census of the launch plan (tests/route_census.py): its size per kernel family, one recipe per kernel whose stated stage
shape the plan routes to that kernel, and every kernel that is known to launch (tests/golden/launch_routes.json) inside it.
No device is needed.  A new template argument or compiled size in launch_routes.hpp changes the counts pinned here, and this
file fails until the new kernels have recipes (and with them a case in tests/test_gpu_route_parity.py)."""
import collections
import json
import os
import re

import route_census as rc
from route_census import K1, EVD, SCAN
from test_cpu_launch_routes import GOLDEN, STAGE_KERNELS, normalised

FAMILIES = {
    K1: {"cov_wave_kernel": 44, "cov_piece_kernel": 16, "cov_mfma_kernel": 4, "cov_combine_kernel": 1, "cov_fb_kernel": 1},
    EVD: {"music_evd_kernel": 12,      # N 2..4 x (double, float, double with counts, double in a group)
          "music_evd_subspace_kernel": 16, "music_evd_quad_kernel": 2,
          # the group / block16 forms: 17
          "music_evd_group_kernel": 4, "music_evd_group_counts_kernel": 2, "music_evd_group_record_kernel": 2, "music_evd_group_full_kernel": 2,
          "music_evd_block16_kernel": 4, "music_evd_block16_counts_kernel": 1, "music_evd_block16_record_kernel": 1, "music_evd_block16_full_kernel": 1},
    SCAN: {"music_scan_peak1_kernel": 228, "music_scan_kernel": 196, "music_scan_generic_kernel": 14, "music_scan_peak_long_kernel": 7,
           "music_scan_stream_kernel": 7},
}
CENSUS = rc.census()


def test_the_census_sizes_are_pinned():
    assert {s: len(k) for s, k in CENSUS.items()} == {K1: 66, EVD: 47, SCAN: 452}
    for stage, kernels in CENSUS.items():
        assert dict(collections.Counter(rc.family(k) for k in kernels)) == FAMILIES[stage], rc.STAGES[stage]
    assert sum(n for f, n in FAMILIES[EVD].items() if f.startswith(("music_evd_group", "music_evd_block16"))) == 17


def test_the_lengths_are_the_issue_s_list_in_its_order():
    assert rc.LENGTHS == (244, 500, 1012, 2036, 4084, 256, 512, 1024, 2048, 2112, 4096, 2500, 3100, 1001, 63, 4100, 8192, 16384)
    # the census keeps the first length of the list that reaches a kernel
    reached = collections.defaultdict(set)
    for shape in rc.grid(SCAN):
        rcode, launches, _ = rc.route(SCAN, shape)
        if rcode >= 1:
            reached[launches[0][0]].add(shape[2])
    for kernel, shape in CENSUS[SCAN].items():
        assert shape[2] == min(reached[kernel], key=rc.LENGTHS.index), (kernel, shape, sorted(reached[kernel]))


def test_every_census_kernel_has_one_recipe_that_routes_to_it():
    for stage, kernels in CENSUS.items():
        recipes, gone = rc.RECIPES[stage], rc.UNREACHABLE[stage]
        assert set(recipes) | set(gone) == set(kernels) and not set(recipes) & set(gone), rc.STAGES[stage]
        for kernel, r in recipes.items():
            assert r["kernel"] == kernel and r["stage"] == stage
            assert r["stages"] == rc.stages_of(r["entry"], r["args"])               # written from the call's arguments
            st, shape = r["stages"][r["at"]]
            assert st == stage
            # every stage of the call has a route, and the recipe's stage launches the recipe's kernel
            for s2, shape2 in r["stages"]:
                assert rc.route(s2, shape2)[0] >= 1, (kernel, r["entry"], r["args"], s2, shape2)
            assert kernel in [launch[0] for launch in rc.route(st, shape)[1]], (kernel, r["entry"], r["args"], shape)
            # the entries' own argument rules (include/doa_hip.h): num_targets < inputs
            assert r["args"].get("M", 0) < r["args"]["N"], (kernel, r["args"])


def test_item_counts():
    """70 items in the eigen recipes (more than a wave of every lanes-per-item form, ragged), 5 in the scan and K1 recipes (a
    full four-wave workgroup and a ragged one), 2 batches of 5 in the groups"""
    for stage, recipes in rc.RECIPES.items():
        for r in recipes.values():
            n = r["stages"][r["at"]][1][{K1: 4, EVD: 3, SCAN: 3}[stage]]
            assert n == (10 if r["entry"].endswith("work_dev_batches") else 70 if stage == EVD else 5), (r["kernel"], n)


def test_unreachable_entries_name_the_host_check_and_stay_under_five_percent():
    for stage, gone in rc.UNREACHABLE.items():
        assert len(gone) * 20 <= len(CENSUS[stage]), rc.STAGES[stage]
        for kernel, where in gone.items():
            assert kernel in CENSUS[stage]
            m = re.fullmatch(r"([\w./-]+):(\d+)", where)
            assert m, (kernel, where)
            path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), m.group(1))
            assert os.path.exists(path) and int(m.group(2)) <= sum(1 for _ in open(path)), where


def routed_name(traced):
    """a normalised traced name as the plan writes it: without the return type and the parameter list"""
    return (traced[4:] if traced.startswith("void") else traced).split("(")[0]


def test_every_traced_stage_kernel_is_in_the_census():
    gold = json.load(open(GOLDEN))
    traced = {normalised(n) for n in gold["names"] if STAGE_KERNELS.match(normalised(n))}
    everything = {k for kernels in CENSUS.values() for k in kernels}
    assert len(traced) >= 177
    missing = sorted(routed_name(t) for t in traced if routed_name(t) not in everything)
    assert not missing, missing


def test_the_golden_trace_has_a_row_for_every_recipe_and_the_recipe_s_kernel_in_it():
    """recipe = launch, on recorded data: tools/record_launch_routes.py traces every recipe ("census:<entry>" rows), and
    test_golden_rows_match_the_routes holds every row to the plan"""
    gold = json.load(open(GOLDEN))
    rows = collections.defaultdict(list)
    for call, stages, kernels in gold["rows"]:
        if call.startswith("census:"):
            rows[(call[7:], json.dumps(stages))].append({routed_name(normalised(gold["names"][k])) for k, _, _ in kernels})
    n = 0
    for recipes in rc.RECIPES.values():
        for kernel, r in recipes.items():
            traced = rows[(r["entry"], json.dumps(r["stages"]))]
            assert traced and all(kernel in names for names in traced), (kernel, r["entry"], r["args"])
            n += 1
    assert n == 565 == sum(len(v) for v in rows.values())
