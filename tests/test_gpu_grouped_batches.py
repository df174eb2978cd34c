"""doa_music_pipeline_work_dev_batches launches K1, the EVD and the scan over GROUPS of consecutive batches on the lean route
(gr-doa_amd/csrc/pipeline.hip, kernels.hpp: BatchGroup; the reference has no counterpart -- GNU Radio hands each block one
work() call at a time).  Whatever the grouping does, every output of every batch -- covariance, spectrum, maximum, arg-max --
must equal, BIT FOR BIT, what one doa_music_pipeline_work_dev call per batch gives on a second handle: the per-item code of the
grouped kernels is the single-batch kernels' own, so there is no tolerance to grant."""
import numpy as np
import pytest
import torch

import doa
from doa.sim import to_sc16

pytestmark = pytest.mark.gpu

K_MAX_GROUP = 8                 # gr-doa_amd/csrc/kernels.hpp: kMaxGroup, the group size of a one-lane call
K_LANE_GROUP = 4                # gr-doa_amd/csrc/pipeline.hip: kLaneGroup, the group size when groups alternate over two lanes
SENTINEL = -77.25               # what output buffers hold before a call (a value no output takes)

LEAN = dict(N=4, K=128, ovl=0, fb=0, d=0.5, M=1, P=256)


def _span(shape, n):
    return (n - 1) * (shape["K"] - shape["ovl"]) + shape["K"]


def _inputs(shape, n, seed, sc16=False):
    """N device streams of one batch: one or M sources at seed-dependent directions, 20 dB SNR"""
    rng = np.random.default_rng(1000 + seed)
    th = np.sort(rng.uniform(25.0, 155.0, size=shape["M"]))
    if shape["M"] > 1:
        th = np.linspace(40.0, 140.0, shape["M"]) + rng.uniform(-8.0, 8.0, size=shape["M"])
    x = doa.sim.make_streams(shape["N"], _span(shape, n), list(th), shape["d"], snr_db=20.0, seed=seed)
    if sc16:
        q = to_sc16(x, 1.0 / 4096.0)
        return [torch.from_numpy(np.ascontiguousarray(q[k])).cuda() for k in range(shape["N"])]
    return [torch.from_numpy(np.ascontiguousarray(x[k])).cuda() for k in range(shape["N"])]


class Bufs:
    """one batch's output buffers, pre-filled with SENTINEL"""

    def __init__(self, shape, n, spec_offset_floats=0):
        N, M, P = shape["N"], shape["M"], shape["P"]
        self.cov = torch.full((n, N * N, 2), SENTINEL, dtype=torch.float32, device="cuda")
        self._spec = torch.full((n * P + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        self.spec = self._spec[spec_offset_floats:spec_offset_floats + n * P]
        self.mx = torch.full((n, M), SENTINEL, dtype=torch.float32, device="cuda")
        self.am = torch.full((n, M), SENTINEL, dtype=torch.float32, device="cuda")

    def host(self):
        return [t.cpu().numpy().copy() for t in (self.cov, self.spec, self.mx, self.am)]


def _pipe(shape, max_batch, sc16=False):
    cls = doa.music_pipeline_sc16 if sc16 else doa.music_pipeline
    args = (shape["N"], shape["K"], shape["ovl"], shape["fb"], shape["d"], shape["M"], shape["P"])
    return cls(*args, max_batch=max_batch) if not sc16 else cls(*args, scale=1.0 / 4096.0, max_batch=max_batch)


def _reference(shape, n, ins, want_cov, want_spec, max_batch, sc16=False, spec_offset=None):
    """one work_dev call per batch on a handle of its own; returns the host copies [cov, spec, mx, am] per batch"""
    p = _pipe(shape, max_batch, sc16)
    res = []
    for b, x in enumerate(ins):
        o = Bufs(shape, n, 0 if spec_offset is None else spec_offset[b])
        p.work_dev(n, [t.data_ptr() for t in x], o.cov.data_ptr() if want_cov[b] else 0, o.spec.data_ptr() if want_spec[b] else 0,
                   o.mx.data_ptr(), o.am.data_ptr(), torch.cuda.current_stream())
        torch.cuda.synchronize()
        res.append(o.host())
    return res


def _call(p, n, ins, outs, want_cov, want_spec, form, cov_array=True, spec_array=True):
    """one work_dev_batches call; form = 'attached' | 'detached'.  outs[b] may repeat (aliased buffers)."""
    cov = [o.cov.data_ptr() if w else 0 for o, w in zip(outs, want_cov)] if cov_array else None
    spec = [o.spec.data_ptr() if w else 0 for o, w in zip(outs, want_spec)] if spec_array else None
    st = doa.DETACHED if form == "detached" else torch.cuda.current_stream()
    r = p.work_dev_batches(n, [[t.data_ptr() for t in x] for x in ins], cov, spec, [o.mx.data_ptr() for o in outs],
                           [o.am.data_ptr() for o in outs], st)
    if form == "detached":
        p.synchronize()
    torch.cuda.synchronize()
    return r


def _same(got, want, what):
    for g, w, name in zip(got, want, ("cov", "spec", "max", "argmax")):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name)


def _check(shape, n, n_batches, lanes, form, max_batch=None, want_cov=None, want_spec=None, cov_array=True, spec_array=True,
           sc16=False, ins=None, spec_offset=None, calls=1):
    max_batch = max_batch or n
    want_cov = want_cov or [True] * n_batches
    want_spec = want_spec or [True] * n_batches
    if not cov_array:
        want_cov = [False] * n_batches
    if not spec_array:
        want_spec = [False] * n_batches
    ins = ins or [_inputs(shape, n, seed=b, sc16=sc16) for b in range(n_batches)]
    ref = _reference(shape, n, ins, want_cov, want_spec, max_batch, sc16, spec_offset)
    p = _pipe(shape, max_batch, sc16)
    p.set_lanes(lanes)
    for c in range(calls):                                # (later calls: the lane rotation carries over)
        outs = [Bufs(shape, n, 0 if spec_offset is None else spec_offset[b]) for b in range(n_batches)]
        assert _call(p, n, ins, outs, want_cov, want_spec, form, cov_array, spec_array) == n_batches * n
        for b in range(n_batches):
            # (a buffer the caller did not hand over keeps its sentinel in the reference and here alike)
            _same(outs[b].host(), ref[b], (c, b))
    return p


FORMS = [(1, "attached"), (2, "attached"), (4, "attached"), (2, "detached"), (4, "detached"), (1, "detached")]


@pytest.mark.parametrize("lanes,form", FORMS)
@pytest.mark.parametrize("n_batches", [1, K_LANE_GROUP - 1, K_LANE_GROUP, K_LANE_GROUP + 1, K_MAX_GROUP - 1, K_MAX_GROUP, K_MAX_GROUP + 1,
                                       2 * K_MAX_GROUP + 4])
def test_batch_counts_below_on_and_above_the_group_size(n_batches, lanes, form):
    _check(LEAN, 100, n_batches, lanes, form, max_batch=128)          # n % 64 != 0 and n < max_batch


@pytest.mark.parametrize("n", [1, 5, 63, 65, 130])
def test_ragged_batches(n):
    """n not a multiple of 64: the lanes of an EVD wave sit in different batches"""
    _check(LEAN, n, 11, 2, "detached", max_batch=200)
    _check(LEAN, n, 11, 1, "attached", max_batch=200)


@pytest.mark.parametrize("lanes,form", [(1, "attached"), (4, "attached"), (2, "detached")])
def test_covariance_array_null_or_with_null_entries(lanes, form):
    nb = 13
    _check(LEAN, 96, nb, lanes, form, cov_array=False)
    _check(LEAN, 96, nb, lanes, form, want_cov=[b % 3 != 1 for b in range(nb)])


@pytest.mark.parametrize("lanes,form", [(1, "attached"), (4, "attached"), (2, "detached")])
def test_mixed_spectrum_flags_split_the_groups_and_angles_only_touches_nothing(lanes, form):
    nb = 19
    flags = [True, True, False, False, False, True, False, True, True, True, True, False, False, False, False, False, False, False, False]
    _check(LEAN, 96, nb, lanes, form, want_spec=flags)                # sentinel rows of the angles-only batches are compared too
    _check(LEAN, 96, nb, lanes, form, spec_array=False)
    _check(LEAN, 96, nb, lanes, form, spec_array=False, cov_array=False)


def test_angles_only_groups_are_bounded_by_their_scratch_rows():
    """a handle whose max_batch rows make 16 MiB: angles-only groups hold two batches (32 MiB of scratch rows), results unchanged"""
    shape = dict(LEAN, P=1024)
    _check(shape, 300, 7, 2, "detached", max_batch=4096, spec_array=False)


@pytest.mark.parametrize("lanes,form", [(1, "attached"), (4, "attached"), (2, "detached"), (4, "detached")])
@pytest.mark.parametrize("k", [3, K_LANE_GROUP, 5, K_MAX_GROUP])
def test_batches_that_share_buffers_stay_ordered(k, lanes, form):
    """batches b and b + k write the same buffers: the later one must win, whether the inputs are the same or not"""
    n, nb = 96, 3 * K_MAX_GROUP + 2
    for same_inputs in (True, False):
        ins = [_inputs(LEAN, n, seed=(b % k) if same_inputs else b) for b in range(nb)]
        ref = _reference(LEAN, n, ins, [True] * nb, [True] * nb, n)
        sets = [Bufs(LEAN, n) for _ in range(k)]
        p = _pipe(LEAN, n)
        p.set_lanes(lanes)
        _call(p, n, ins, [sets[b % k] for b in range(nb)], [True] * nb, [True] * nb, form)
        for j in range(k):
            last = max(b for b in range(nb) if b % k == j)
            _same(sets[j].host(), ref[last], (same_inputs, j))


def test_partially_shared_outputs_and_outputs_shared_across_lanes():
    """one shared pointer is enough to order two batches; a batch whose outputs were last written on two different lanes
    is ordered behind both"""
    n, nb = 96, 24
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    ref = _reference(LEAN, n, ins, [True] * nb, [True] * nb, n)
    for lanes, form in ((4, "detached"), (2, "attached"), (4, "attached")):
        outs = [Bufs(LEAN, n) for _ in range(nb)]
        outs[17].mx = outs[1].mx                     # batch 17 shares only its maxima with batch 1 (another group)
        outs[21].mx = outs[2].mx                     # batch 21: the maxima of one earlier group ...
        outs[21].am = outs[12].am                    # ... and the arg-max of another, which sits on another lane
        p = _pipe(LEAN, n)
        p.set_lanes(lanes)
        _call(p, n, ins, outs, [True] * nb, [True] * nb, form)
        for b in range(nb):
            got, want = outs[b].host(), [a.copy() for a in ref[b]]
            if b == 1:
                want[2] = ref[17][2]
            if b == 2:
                want[2] = ref[21][2]
            if b == 12:
                want[3] = ref[21][3]
            _same(got, want, (lanes, form, b))


@pytest.mark.parametrize("lanes,form", [(1, "attached"), (2, "detached")])
def test_nan_sample_inside_a_group(lanes, form):
    n, nb = 96, 10
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    x = ins[4][2].cpu().numpy().copy()
    x[37 * LEAN["K"] + 5] = np.nan                   # item 37 of batch 4: the scan's irregular path
    ins[4][2] = torch.from_numpy(x).cuda()
    for kw in (dict(), dict(spec_array=False)):
        _check(LEAN, n, nb, lanes, form, ins=ins, **kw)


@pytest.mark.parametrize("lanes,form", [(1, "attached"), (4, "detached")])
def test_sc16_input(lanes, form):
    _check(LEAN, 100, 11, lanes, form, max_batch=128, sc16=True)


@pytest.mark.parametrize("shape", [dict(LEAN, N=2), dict(LEAN, N=3), dict(LEAN, N=4, P=512), dict(LEAN, N=4, K=1024, P=1024),
                                   dict(LEAN, N=4, M=2), dict(LEAN, N=3, M=2), dict(LEAN, N=4, M=3), dict(LEAN, K=127),
                                   dict(LEAN, fb=1), dict(N=4, K=2048, ovl=512, fb=1, d=0.4, M=2, P=1024),
                                   dict(LEAN, N=6, K=64), dict(LEAN, P=300), dict(LEAN, P=2048)],
                         ids=lambda s: "N%d_K%d_o%d_fb%d_M%d_P%d" % (s["N"], s["K"], s["ovl"], s["fb"], s["M"], s["P"]))
def test_shapes_on_and_off_the_lean_route(shape):
    for lanes, form in ((1, "attached"), (2, "detached"), (4, "attached")):
        _check(shape, 70, K_MAX_GROUP + 3, lanes, form, max_batch=80)


@pytest.mark.parametrize("lanes,form", [(1, "attached"), (4, "detached")])
def test_odd_snapshot_size_groups_batches_of_either_alignment(lanes, form):
    """K = 63, n = 17: batches cut one after the other from one buffer lie 1071 samples apart, so every second one is aligned to
    one sample only.  With an odd step K1 takes the single loads whatever the alignment: nothing mixes, the batches share
    their groups' launches, and every batch equals its own work_dev call bit for bit."""
    shape, n, nb = dict(LEAN, K=63), 17, 5
    whole = _inputs(shape, nb * n, seed=7)
    ins = [[t[b * n * 63:(b + 1) * n * 63] for t in whole] for b in range(nb)]
    assert {x[0].data_ptr() % 16 for x in ins} == {0, 8}
    _check(shape, n, nb, lanes, form, ins=ins)


def test_unaligned_spectrum_pointer_inside_a_call():
    """a batch whose spectrum pointer is not 16-byte aligned leaves the lean route on its own; its neighbours stay grouped"""
    nb = 10
    _check(LEAN, 96, nb, 2, "detached", spec_offset=[1 if b in (3, 4, 9) else 0 for b in range(nb)])


def test_float_internal_precision_keeps_per_batch_launches():
    n, nb = 96, 10
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    res = []
    for batches in (False, True):
        p = _pipe(LEAN, n)
        p.set_internal_precision(32)
        outs = [Bufs(LEAN, n) for _ in range(nb)]
        if batches:
            p.set_lanes(2)
            _call(p, n, ins, outs, [True] * nb, [True] * nb, "detached")
        else:
            for b in range(nb):
                p.work_dev(n, [t.data_ptr() for t in ins[b]], outs[b].cov.data_ptr(), outs[b].spec.data_ptr(), outs[b].mx.data_ptr(),
                           outs[b].am.data_ptr(), torch.cuda.current_stream())
            torch.cuda.synchronize()
        res.append([o.host() for o in outs])
    for b in range(nb):
        _same(res[1][b], res[0][b], b)


def test_several_calls_and_adopted_lane_streams():
    _check(LEAN, 100, K_MAX_GROUP + 5, 4, "detached", max_batch=128, calls=3)
    _check(LEAN, 100, K_MAX_GROUP + 5, 2, "attached", max_batch=128, calls=3)
    n, nb = 100, 2 * K_MAX_GROUP + 1
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    ref = _reference(LEAN, n, ins, [True] * nb, [True] * nb, n)
    streams = [torch.cuda.Stream() for _ in range(3)]
    p = _pipe(LEAN, n)
    p.set_lane_streams(streams)
    for form in ("attached", "detached"):
        outs = [Bufs(LEAN, n) for _ in range(nb)]
        _call(p, n, ins, outs, [True] * nb, [True] * nb, form)
        for b in range(nb):
            _same(outs[b].host(), ref[b], (form, b))


def test_stage_masks_apply_to_groups():
    n, nb = 96, 10
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    ref = _reference(LEAN, n, ins, [True] * nb, [True] * nb, n)
    p = _pipe(LEAN, n)
    p.set_lanes(2)
    p.set_stages(cov=True, evd=False, scan=False)
    outs = [Bufs(LEAN, n) for _ in range(nb)]
    _call(p, n, ins, outs, [True] * nb, [True] * nb, "detached")
    for b in range(nb):
        got = outs[b].host()
        assert np.array_equal(got[0].view(np.uint8), ref[b][0].view(np.uint8))
        assert all(np.all(a == SENTINEL) for a in got[1:])
    p.set_stages(cov=False, evd=True, scan=True)     # the covariances are in place: the rest of the chain completes the outputs
    _call(p, n, ins, outs, [True] * nb, [True] * nb, "detached")
    for b in range(nb):
        _same(outs[b].host(), ref[b], b)


@pytest.mark.parametrize("lanes,form", FORMS)
def test_injected_failure_in_the_middle_of_a_group(lanes, form):
    n, nb, bad = 96, 2 * K_MAX_GROUP + 3, K_MAX_GROUP + 3
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    ref = _reference(LEAN, n, ins, [True] * nb, [True] * nb, n)
    p = _pipe(LEAN, n)
    p.set_lanes(lanes)
    outs = [Bufs(LEAN, n) for _ in range(nb)]
    p.inject_failure(bad)
    with pytest.raises(doa.DoaError) as ei:
        _call(p, n, ins, outs, [True] * nb, [True] * nb, form)
    assert ei.value.status == -3 and "injected failure in batch %d" % bad in str(ei.value)
    assert p.lanes_idle()                            # an error return: nothing of the call still runs
    torch.cuda.synchronize()
    for b in range(nb):
        got = outs[b].host()
        if b < bad:
            _same(got, ref[b], b)                    # batches before the failure were launched ...
        else:
            assert all(np.all(a == SENTINEL) for a in got), b     # ... the others never
    outs = [Bufs(LEAN, n) for _ in range(nb)]
    assert _call(p, n, ins, outs, [True] * nb, [True] * nb, form) == nb * n       # one-shot: a clean call follows
    for b in range(nb):
        _same(outs[b].host(), ref[b], b)


def test_eigen_fall_back_items_inside_a_group_are_counted_once_each():
    """R = c I (every antenna one unit impulse at a time of its own): the signal-subspace iteration cannot certify such an item
    and hands it to the Jacobi, which the counter records -- per item, whatever launch the item is part of"""
    n, nb = 100, K_MAX_GROUP + 2
    N, K = LEAN["N"], LEAN["K"]
    ins = [_inputs(LEAN, n, seed=b) for b in range(nb)]
    flat = [(2, 0), (2, 63), (2, 64), (2, 99), (3, 0), (7, 17), (8, 5), (9, 99)]         # (batch, item)
    for b in sorted({b for b, _ in flat}):
        xs = [t.cpu().numpy().copy() for t in ins[b]]
        for bb, i in flat:
            if bb == b:
                for a in range(N):
                    xs[a][i * K:(i + 1) * K] = 0
                    xs[a][i * K + 3 * a + 1] = 1.0
        ins[b] = [torch.from_numpy(x).cuda() for x in xs]
    doa.evd_fallback_count(reset=True)
    ref = _reference(LEAN, n, ins, [True] * nb, [True] * nb, n)
    assert doa.evd_fallback_count(reset=True) == len(flat)
    for lanes, form in ((1, "attached"), (2, "detached")):
        p = _pipe(LEAN, n)
        p.set_lanes(lanes)
        outs = [Bufs(LEAN, n) for _ in range(nb)]
        _call(p, n, ins, outs, [True] * nb, [True] * nb, form)
        assert doa.evd_fallback_count(reset=True) == len(flat)
        for b in range(nb):
            _same(outs[b].host(), ref[b], b)
