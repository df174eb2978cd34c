"""The plan of a doa_*_pipeline_work_dev_batches call (gr-doa_amd/csrc/batch_plan.hpp) through doa_hip_batch_plan_debug: which
consecutive batches form a group, which lane a group runs on, which groups join the lanes first.  No device is needed.  The
random part asserts the contract include/doa_hip.h gives under GROUPS and ORDER, not the algorithm; the literal plans pin what
the planning loop gave before it became a function (the reference has no counterpart: GNU Radio hands a block one work() call
at a time)."""
import ctypes as C
import random

import pytest

from doa import _lib

LEAN, STORE, VEC2 = 1, 2, 4


def plan(outputs, flags, caps, n_lanes, rot_in):
    """outputs: per batch up to four pointer values (0 / None = absent).  Returns (group, lane, sync_first per batch, rot_out)."""
    nb = len(outputs)
    flat = (C.c_void_p * (4 * nb + 1))()
    for b, out in enumerate(outputs):
        for k, p in enumerate(out):
            flat[4 * b + k] = p or None
    fl = (C.c_ubyte * (nb + 1))(*flags)
    cp = (C.c_int * (nb + 1))(*caps)
    grp, lane, sync = (C.c_int * (nb + 1))(), (C.c_int * (nb + 1))(), (C.c_int * (nb + 1))()
    rot = C.c_int(-1)
    n_groups = _lib.lib.doa_hip_batch_plan_debug(nb, flat, fl, cp, n_lanes, rot_in, grp, lane, sync, C.byref(rot))
    assert n_groups >= 0, _lib.last_error()
    g = list(grp[:nb])
    assert n_groups == (g[-1] + 1 if nb else 0)
    return g, list(lane[:nb]), list(sync[:nb]), rot.value


def random_call(rng):
    nb, L = rng.randint(1, 30), rng.randint(1, 8)
    pool = rng.choice((4, 8, 40, 1000))          # aliasing frequent ... rare
    outputs = []
    for _ in range(nb):
        present = [rng.random() < 0.67, rng.random() < 0.67, True, True]      # covariance and spectrum are optional
        ptrs = rng.sample(range(1, pool + 1), sum(present))                   # a batch's own pointers are distinct
        outputs.append([0x7F0000000000 + 256 * ptrs.pop() if p else 0 for p in present])
    flags = [(LEAN if rng.random() < 0.75 else 0) | (STORE if rng.random() < 0.5 else 0) | (VEC2 if rng.random() < 0.25 else 0)
             for _ in range(nb)]
    caps = [rng.choice((1, 2, 4, 8)) for _ in range(nb)]
    return outputs, flags, caps, L, rng.randrange(L)


def check_contract(outputs, flags, caps, L, rot_in, stats):
    grp, lane, sync, rot_out = plan(outputs, flags, caps, L, rot_in)
    nb, n_groups = len(outputs), grp[-1] + 1
    # (a) groups are consecutive runs that cover every batch once
    assert grp[0] == 0 and all(grp[b + 1] - grp[b] in (0, 1) for b in range(nb - 1))
    members = [[b for b in range(nb) if grp[b] == g] for g in range(n_groups)]
    for m in members:
        # a group has one lane and one sync_first, (f) every lane is below L
        assert len({lane[b] for b in m}) == 1 and len({sync[b] for b in m}) == 1 and 0 <= lane[m[0]] < L
        # (b) more than one batch: all lean, uniform in store and vec2, no longer than the first batch's cap
        if len(m) > 1:
            assert all(flags[b] & LEAN for b in m) and len({flags[b] & (STORE | VEC2) for b in m}) == 1 and len(m) <= caps[m[0]]
        # (c) no output pointer twice inside a group
        ptrs = [p for b in m for p in outputs[b] if p]
        assert len(ptrs) == len(set(ptrs))
    # (d) a pointer an earlier group wrote last: same lane, or the later group joins the lanes first
    writer, shared = {}, False
    for g, m in enumerate(members):
        for b in m:
            for p in outputs[b]:
                if p and p in writer and writer[p] != g:
                    shared = True
                    assert lane[members[writer[p]][0]] == lane[m[0]] or sync[m[0]], (g, writer[p])
        for b in m:
            for p in outputs[b]:
                if p:
                    writer[p] = g
    # (e) nothing shared between groups: the plain rotation
    if not shared:
        assert [lane[m[0]] for m in members] == [(rot_in + i) % L for i in range(n_groups)]
        assert not any(sync) and rot_out == (rot_in + n_groups) % L
    assert 0 <= rot_out < L
    stats[0] += shared
    stats[1] += any(sync)


def test_random_calls_keep_the_contract():
    rng = random.Random(20261019)
    n_calls, stats = 12000, [0, 0]
    for _ in range(n_calls):
        check_contract(*random_call(rng), stats)
    # the generator reaches what it is for: most calls alias across groups, many need a host join
    assert stats[0] > n_calls // 2 and stats[1] > n_calls // 10, stats


def _sets(nb, ptrs_per_batch, base=0x10000, share=None):
    """distinct output pointers per batch (or per set share(b))"""
    return [[base + 0x1000 * (share(b) if share else b) + 0x100 * k if k < ptrs_per_batch else 0 for k in range(4)] for b in range(nb)]


def _runs(spec):
    """[(n_batches, lane, sync_first), ...] -> per-batch group, lane, sync_first"""
    grp, lane, sync = [], [], []
    for g, (n, ln, sy) in enumerate(spec):
        grp += [g] * n; lane += [ln] * n; sync += [sy] * n
    return grp, lane, sync


WANT_SPEC = [True, True, False, False, False, True, False, True, True, True, True, False, False, False, False, False, False, False, False]


@pytest.mark.parametrize("L,cap,runs,rot_out", [
    (2, 4, [(2, 0, 0), (3, 1, 0), (1, 0, 0), (1, 1, 0), (4, 0, 0), (4, 1, 0), (4, 0, 0)], 1),
    (1, 8, [(2, 0, 0), (3, 0, 0), (1, 0, 0), (1, 0, 0), (4, 0, 0), (8, 0, 0)], 0)])
def test_alias_free_music_call(L, cap, runs, rot_out):
    """19 lean batches with the spectrum flags of test_mixed_spectrum_flags_split_the_groups... (test_gpu_grouped_batches.py)"""
    outputs = _sets(19, 4)
    for b, w in enumerate(WANT_SPEC):
        if not w:
            outputs[b][1] = 0
    flags = [LEAN | VEC2 | (STORE if w else 0) for w in WANT_SPEC]
    assert plan(outputs, flags, [cap] * 19, L, 0) == (*_runs(runs), rot_out)


@pytest.mark.parametrize("L,lanes,rot_out", [
    (4, [b % 4 for b in range(20)], 0),
    (3, [0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 2, 0], 2),
    (5, [0, 1, 2, 3, 4, 0, 1, 2, 0, 1, 2, 3, 4, 0, 1, 2, 0, 1, 2, 3], 3)])
def test_root_pattern_of_eight_rotating_sets(L, lanes, rot_out):
    """the Root handle under the benchmark's pattern: no batch is lean, batch b writes set b % 8 (angles and status): a batch
    follows the earlier writer of its set on that batch's lane, and no host join is needed at any lane count"""
    outputs = [[0] + o[:3] for o in _sets(20, 2, share=lambda b: b % 8)]
    assert plan(outputs, [0] * 20, [1] * 20, L, 0) == (list(range(20)), lanes, [0] * 20, rot_out)


@pytest.mark.parametrize("L,runs", [
    (2, [(4, 0, 0), (4, 1, 0), (4, 0, 0), (4, 1, 0), (4, 0, 0), (1, 0, 0), (3, 1, 1)]),
    (4, [(4, 0, 0), (4, 1, 0), (4, 2, 0), (4, 3, 0), (4, 0, 0), (1, 0, 0), (3, 3, 1)])])
def test_outputs_last_written_on_two_lanes(L, runs):
    """the layout of test_partially_shared_outputs_and_outputs_shared_across_lanes: batch 17 shares its maxima with batch 1
    (its group follows that group's lane); batch 21 shares its maxima with batch 2 and its arg-max with batch 12, which sit on
    different lanes: it opens a group that joins the lanes first and takes the lane of the pointer seen last"""
    outputs = _sets(24, 4)
    outputs[17][2] = outputs[1][2]
    outputs[21][2] = outputs[2][2]
    outputs[21][3] = outputs[12][3]
    assert plan(outputs, [LEAN | STORE | VEC2] * 24, [4] * 24, L, 0) == (*_runs(runs), 1)


def test_rotation_carries_over_and_an_empty_call_plans_nothing():
    outputs = _sets(5, 3)
    assert plan(outputs, [0] * 5, [1] * 5, 3, 2) == ([0, 1, 2, 3, 4], [2, 0, 1, 2, 0], [0] * 5, 1)
    assert plan([], [], [], 3, 2) == ([], [], [], 2)
