"""GPU tests of root_pipeline.work_dev_auto (the source count estimated per snapshot inside the Root-MUSIC pipeline):
covariance, counts, eigenvalues, angles and status are BIT-IDENTICAL to the three blocks chained by hand -- autocorrelate ->
source_count -> rootMUSIC_linear_array.work_dev_counts --, the covariance is also work_dev's, and the counts equal the numpy
reference of the criterion (tests/source_count_ref.py)."""
import numpy as np
import pytest
import torch

import doa
import source_count_cases as cases
import source_count_ref as ref
from doa.sim import to_sc16

pytestmark = pytest.mark.gpu

S15 = 2.0 ** -15
# name: (covariance case, num_targets, sc16 input + fused antenna correction)
# n4_two_fb: overlap 64 with forward-backward averaging -- K1's read-once path; n5_two_s1: 67 items, a partial last wave
SHAPES = {
    "n4": ("n4_two_fb", 3, False),
    "n5": ("n5_two_s1", 4, False),
    "n16": ("n16_three_fb", 4, False),
    "n3_sc16_gains": ("n3_two", 2, True),
}
GAINS = np.array([1.0 + 0.0j, 0.8 - 0.3j, -0.2 + 1.1j], np.complex64)
METHODS = {"mdl": ref.MDL, "aic": ref.AIC}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _setup(shape, x=None):
    """(pipeline handle, autocorrelate block of the same front end, device streams (kept alive), their pointers, parameters)"""
    name, M, sc16 = SHAPES[shape]
    N, th, d, K, ovl, fb, snr, n, seed = cases.CASES[name]
    x = cases.streams(name) if x is None else x
    if sc16:
        q = to_sc16(x / np.abs(x).max() * 0.25, S15)
        dev = doa.sim.stream_slab_torch([_dev(a) for a in q])
        pipe = doa.root_music_pipeline_sc16(N, K, ovl, fb, d, M, max_batch=n)
        ac = doa.autocorrelate_sc16(N, K, ovl, fb)
        for b in (pipe, ac):
            b.fuse_antenna_correction(GAINS)
    else:
        dev = doa.sim.stream_slab_torch([_dev(a) for a in x])
        pipe = doa.root_pipeline(N, K, ovl, fb, d, M, max_batch=n)
        ac = doa.autocorrelate(N, K, ovl, fb)
    return pipe, ac, dev, [t.data_ptr() for t in dev], (N, d, K, n, M)


def _auto(pipe, ptrs, prm, method="mdl", cov=True, eig=True, status=True):
    N, d, K, n, M = prm
    t = dict(cov=torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda") if cov else None,
             ang=torch.full((n, M), -7.0, dtype=torch.float32, device="cuda"),
             cnt=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
             eig=torch.full((n, N), -7.0, dtype=torch.float32, device="cuda") if eig else None,
             st=torch.full((n,), -7, dtype=torch.int32, device="cuda") if status else None)
    ptr = lambda k: t[k].data_ptr() if t[k] is not None else None
    assert pipe.work_dev_auto(n, ptrs, ptr("ang"), ptr("cnt"), method, ptr("cov"), ptr("eig"), ptr("st"),
                              torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in t.items()}


def _work_dev(pipe, ptrs, prm):
    N, d, K, n, M = prm
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    ang = torch.empty((n, M), dtype=torch.float32, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    assert pipe.work_dev(n, ptrs, cov.data_ptr(), ang.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in (cov, ang, st)]


def _chain(ac, ptrs, prm, method):
    """autocorrelate -> source_count -> rootMUSIC_linear_array.work_dev_counts, three block handles."""
    N, d, K, n, M = prm
    s = torch.cuda.current_stream()
    cov = torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    eig = torch.full((n, N), -7.0, dtype=torch.float32, device="cuda")
    ang = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert ac.work_dev(n, ptrs, cov.data_ptr(), s) == n
    doa.source_count(N, K, method, M).work_dev(n, cov.data_ptr(), cnt.data_ptr(), eig.data_ptr(), s)
    doa.rootMUSIC_linear_array(d, M, N).work_dev_counts(n, cov.data_ptr(), cnt.data_ptr(), ang.data_ptr(), st.data_ptr(), s)
    torch.cuda.synchronize()
    return dict(cov=cov.cpu().numpy(), cnt=cnt.cpu().numpy(), eig=eig.cpu().numpy(), ang=ang.cpu().numpy(), st=st.cpu().numpy())


@pytest.mark.parametrize("method", ["mdl", "aic"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_auto_equals_the_chain_of_blocks(shape, method):
    pipe, ac, dev, ptrs, prm = _setup(shape)
    N, d, K, n, M = prm
    fresh = _work_dev(_setup(shape)[0], ptrs, prm)                  # a handle that never saw an auto call
    got = _auto(pipe, ptrs, prm, method)
    assert _same(got["cov"], fresh[0])                               # K1 exactly as work_dev runs it
    want = _chain(ac, ptrs, prm, method)
    for key in ("cov", "cnt", "eig", "ang", "st"):
        assert _same(got[key], want[key]), (shape, method, key)
    counts = got["cnt"]
    assert counts.min() >= 0 and counts.max() <= M and not got["st"].any()
    # NaN padding: exactly the slots from the item's count on
    pad = np.arange(M)[None, :] >= counts[:, None]
    assert np.array_equal(np.isnan(got["ang"]), pad), (shape, method)
    assert pad.any() or shape == "n3_sc16_gains"                     # (there num_targets is the number of sources)
    # the numpy reference of the criterion (the fc32 shapes: its covariances are those of these streams)
    if not SHAPES[shape][2]:
        c_ref, _, decided = cases.reference(SHAPES[shape][0], METHODS[method], M)
        assert decided.all() and np.array_equal(counts, c_ref), (shape, method, counts, c_ref)
    # optional outputs: the same angles and counts without them
    lean = _auto(pipe, ptrs, prm, method, cov=False, eig=False, status=False)
    for key in ("ang", "cnt"):
        assert _same(lean[key], got[key]), (shape, method, key)
    # the ordinary entry after auto calls: bit-identical to the fresh handle's
    again = _work_dev(pipe, ptrs, prm)
    for a, b in zip(again, fresh):
        assert _same(a, b)


def test_end_to_end_two_sources():
    """First shape: MDL finds two sources in every snapshot; both angles agree with the fixed num_targets = 2 handle's to the
    1e-3 degrees of the parity bar (the eigen routes differ) and lie at the sources."""
    pipe, ac, dev, ptrs, prm = _setup("n4")
    N, d, K, n, M = prm
    got = _auto(pipe, ptrs, prm, "mdl")
    assert np.all(got["cnt"] == 2), got["cnt"]
    c = cases.CASES[SHAPES["n4"][0]]
    fixed = doa.root_pipeline(N, K, c[4], c[5], d, 2, max_batch=n)
    _, ang2, st2 = _work_dev(fixed, ptrs, (N, d, K, n, 2))
    assert not st2.any()
    assert np.abs(got["ang"][:, :2].astype(np.float64) - ang2).max() <= 1e-3
    assert np.all(np.isnan(got["ang"][:, 2]))
    assert np.all(np.abs(got["ang"][:, :2] - np.array([30.0, 123.0])) <= 3.0)


def test_zero_and_nan_snapshots_have_no_usable_count():
    """n5 (no overlap: a snapshot's samples belong to it alone): an all-zero snapshot and one holding a NaN get count -1, status 2
    and NaN angles; every other snapshot is bit-identical to the clean run."""
    shape = "n5"
    N, th, d, K, ovl, fb, snr, n, seed = cases.CASES[SHAPES[shape][0]]
    assert ovl == 0
    clean_pipe, _, dev0, ptrs0, prm = _setup(shape)
    clean = _auto(clean_pipe, ptrs0, prm)
    x = np.array(cases.streams(SHAPES[shape][0]))
    zero, nan = 5, 9
    x[:, zero * K:(zero + 1) * K] = 0
    x[2, nan * K + 17] = complex(np.nan, 1.0)
    pipe, _, dev, ptrs, prm = _setup(shape, x)
    got = _auto(pipe, ptrs, prm)
    for i in (zero, nan):
        assert got["cnt"][i] == -1 and got["st"][i] == 2 and np.all(np.isnan(got["ang"][i])), (i, got["cnt"][i], got["st"][i])
    keep = np.ones(n, bool)
    keep[[zero, nan]] = False
    for key in ("cov", "cnt", "eig", "ang", "st"):
        assert _same(got[key][keep], clean[key][keep]), key


def test_rejections():
    pipe, ac, dev, ptrs, prm = _setup("n4")
    N, d, K, n, M = prm
    out = torch.zeros(n * M, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:                             # the count output is required
        pipe.work_dev_auto(n, ptrs, out.data_ptr(), None)
    assert ei.value.status == -1
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_auto(n, ptrs, out.data_ptr(), cnt.data_ptr(), method=2)
    assert ei.value.status == -1
    with pytest.raises(doa.DoaError) as ei:                             # one batch of at most max_batch items
        pipe.work_dev_auto(n + 1, ptrs, out.data_ptr(), cnt.data_ptr())
    assert ei.value.status == -1 and "max_batch" in str(ei.value)
    pipe.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_auto(n, ptrs, out.data_ptr(), cnt.data_ptr())
    assert ei.value.status == -4                                        # DOA_ERR_UNSUPPORTED
