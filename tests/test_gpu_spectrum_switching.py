"""GPU test of one music_pipeline handle switched through its estimators, geometries and precisions: after every switch the
handle must give, byte for byte, what a fresh handle created directly in that configuration gives.  The record slots between
the stage in front and the scan (coefficient, Chebyshev, full, status) are sized from one plan (spectrum_chain.hpp;
tests/test_cpu_spectrum_plan.py checks the plan itself); what can go wrong on the device is a slot that a configuration needs
but that was not reserved after a switch, and the scan then reads a stale or missing record.

N = 4 takes the one-lane eigen form and the Chebyshev record, N = 8 the 8-lane form and no Chebyshev record.  17 items: one past
a wave of 16 quads, no multiple of 4 or 8.  Item 2's samples are all zero, so Capon reports status 1 for it and the follow-up
launch has a row to overwrite.  Nothing here provokes a fault: every call is one the entries accept."""
import functools

import numpy as np
import pytest
import torch

import doa

pytestmark = pytest.mark.gpu

K, M, P, NB, D = 32, 2, 256, 17, 0.5
N_AZ = N_EL = 16
LOADING = 1e-2
ZERO_ITEM = 2
SIZES = (4, 8)


@functools.lru_cache(maxsize=None)
def _streams(N):
    """N device streams of NB * K samples: two tones 20 dB above the noise, item ZERO_ITEM silent"""
    rng = np.random.default_rng(20261020 + N)
    A = np.exp(-2j * np.pi * D * np.outer(np.arange(N), np.cos(np.deg2rad([50.0, 115.0]))))
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)      # noqa: E731
    x = (A @ cn(M, NB * K) + 0.1 * cn(N, NB * K)).astype(np.complex64)
    x[:, ZERO_ITEM * K:(ZERO_ITEM + 1) * K] = 0
    return tuple(doa.sim.stream_slab_torch([torch.from_numpy(np.array(a)).cuda() for a in x]))


@functools.lru_cache(maxsize=None)
def _table(N, grid):
    xy = doa.uca_positions(N, 0.5)
    t = doa.planar_steering_grid(xy, N_AZ, N_EL) if grid else doa.planar_steering_table(xy, P)
    t.setflags(write=False)
    return t


def _new(N):
    return doa.music_pipeline(N, K, 0, 0, D, M, P, max_batch=NB)


def _run(pipe, N, spec, auto=False):
    """one call -> the bytes of every output (cov, spec, max, argmax; auto: the counts too)"""
    am_width = 2 * M if pipe.steering_grid else M
    o = {"cov": torch.full((NB, N * N), -7.0, dtype=torch.complex64, device="cuda"),
         "mx": torch.full((NB, M), -7.0, dtype=torch.float32, device="cuda"),
         "am": torch.full((NB, am_width), -7.0, dtype=torch.float32, device="cuda")}
    if spec:
        o["spec"] = torch.full((NB, P), -7.0, dtype=torch.float32, device="cuda")
    ptrs = [t.data_ptr() for t in _streams(N)]
    st = torch.cuda.current_stream()
    sp = o["spec"].data_ptr() if spec else 0
    if auto:
        o["cnt"] = torch.full((NB,), -7, dtype=torch.int32, device="cuda")
        rc = pipe.work_dev_auto(NB, ptrs, o["mx"].data_ptr(), o["am"].data_ptr(), o["cnt"].data_ptr(), "mdl",
                                d_cov_ptr=o["cov"].data_ptr(), d_spec_ptr=sp or None, stream=st)
    else:
        rc = pipe.work_dev(NB, ptrs, o["cov"].data_ptr(), sp, o["mx"].data_ptr(), o["am"].data_ptr(), st)
    assert rc == NB
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in o.items()}


def _both(pipe, N, auto=False):
    return {"full": _run(pipe, N, True, auto), "angles only": _run(pipe, N, False, auto)}


# step -> (what the switched handle does, what a fresh handle does to get there directly)
def _music(p, N): p.set_estimator("music")                                            # noqa: E704
def _capon(p, N): p.set_estimator("capon", LOADING)                                   # noqa: E704
def _tab(p, N): p.set_steering_table(_table(N, False), 0.0, 360.0)                    # noqa: E704
def _grid(p, N): p.set_steering_grid(_table(N, True), N_AZ, N_EL)                     # noqa: E704
def _clear(p, N): p.set_steering_table(None)                                          # noqa: E704
def _b32(p, N): p.set_internal_precision(32)                                          # noqa: E704
def _b64(p, N): p.set_internal_precision(64)                                          # noqa: E704


STEPS = [
    ("1 MUSIC, ULA", [], [], 64, False),
    ("2 Capon, ULA", [_capon], [_capon], 64, False),
    ("3 MUSIC, table", [_tab, _music], [_tab], 64, False),
    ("4 Capon, table", [_capon], [_capon, _tab], 64, False),
    ("5 Capon, grid", [_grid], [_capon, _grid], 64, False),
    ("6 MUSIC, grid", [_music], [_grid], 64, False),
    ("7 MUSIC, ULA again", [_clear], [], 64, False),
    ("8 MUSIC, ULA, 32 bits", [_b32], [], 32, False),
    ("9 64 bits, auto", [_b64], [], 64, True),
]


@functools.lru_cache(maxsize=None)
def _fresh(N, step):
    """what a fresh handle created directly in the step's configuration gives (computed once)"""
    name, _, direct, bits, auto = STEPS[step]
    doa.set_internal_precision(bits)
    try:
        pipe = _new(N)
    finally:
        doa.set_internal_precision(64)
    for f in direct:
        f(pipe, N)
    out = _both(pipe, N)
    if auto:
        out["auto"] = _both(pipe, N, auto=True)
    return out


def _flat(d, path=()):
    """nested dicts of bytes -> {path: bytes}"""
    out = {}
    for k, v in d.items():
        out.update(_flat(v, path + (k,)) if isinstance(v, dict) else {path + (k,): v})
    return out


def _assert_same(got, want, where):
    got, want = _flat(got), _flat(want)
    assert sorted(got) == sorted(want), where
    for path in want:
        assert got[path] == want[path], where + path


@pytest.mark.parametrize("N", SIZES)
def test_a_switched_handle_equals_a_fresh_one(N):
    pipe = _new(N)
    for step, (name, switch, _, bits, auto) in enumerate(STEPS):
        for f in switch:
            f(pipe, N)
        got = _both(pipe, N)
        if auto:
            got["auto"] = _both(pipe, N, auto=True)
        _assert_same(got, _fresh(N, step), (N, name))
    # the silent item did give the follow-up work: under Capon its row and peaks are NaN
    capon = _fresh(N, 1)["full"]
    spec = np.frombuffer(capon["spec"], np.float32).reshape(NB, P)
    mx = np.frombuffer(capon["mx"], np.float32).reshape(NB, M)
    assert np.isnan(spec[ZERO_ITEM]).all() and np.isnan(mx[ZERO_ITEM]).all()
    assert not np.isnan(np.delete(spec, ZERO_ITEM, axis=0)).any()


@pytest.mark.parametrize("N", SIZES)
def test_a_handle_created_at_32_bits_reaches_the_double_ula_through_a_table(N):
    """the one route to MUSIC on the ULA in double that passes no setter which sized the ULA's records in double: created at 32
    bits (no Chebyshev record), a table set at 32 bits, 64 bits set while the table is there, the table cleared"""
    doa.set_internal_precision(32)
    try:
        pipe = _new(N)
    finally:
        doa.set_internal_precision(64)
    for f in (_tab, _b64, _clear):
        f(pipe, N)
    want = {k: v for k, v in _fresh(N, 0).items() if k != "auto"}
    _assert_same(_both(pipe, N), want, (N,))
