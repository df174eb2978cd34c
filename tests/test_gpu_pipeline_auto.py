"""GPU tests of music_pipeline.work_dev_auto (the source count estimated per snapshot inside the pipeline): counts,
eigenvalues, spectrum, maxima and arg-maxima are BIT-IDENTICAL to the chain source_count -> MUSIC_lin_array.work_dev_counts
-> find_local_max.work_dev_counts fed the covariance work_dev_auto itself wrote, and that covariance is bit-identical to
work_dev's."""
import numpy as np
import pytest
import torch

import doa
import source_count_cases as cases
from doa.sim import to_sc16

pytestmark = pytest.mark.gpu

S15 = 2.0 ** -15
# name: (covariance case, pspectrum_len, num_targets, sc16 input + fused antenna correction)
SHAPES = {
    "n4": ("n4_two_fb", 256, 3, False),
    "n3_sc16_gains": ("n3_two", 512, 2, True),
    "n8": ("n8_three", 1000, 5, False),
    "n16": ("n16_three_fb", 2048, 4, False),
}
GAINS = np.array([1.0 + 0.0j, 0.8 - 0.3j, -0.2 + 1.1j], np.complex64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _setup(shape):
    """(pipeline handle, device streams (kept alive), their pointers, case parameters)"""
    name, P, M, sc16 = SHAPES[shape]
    N, th, d, K, ovl, fb, snr, n, seed = cases.CASES[name]
    x = cases.streams(name)
    if sc16:
        q = to_sc16(x / np.abs(x).max() * 0.25, S15)
        dev = doa.sim.stream_slab_torch([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in q])
        pipe = doa.music_pipeline_sc16(N, K, ovl, fb, d, M, P, max_batch=n)
        pipe.fuse_antenna_correction(GAINS)
    else:
        dev = doa.sim.stream_slab_torch([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in x])
        pipe = doa.music_pipeline(N, K, ovl, fb, d, M, P, max_batch=n)
    return pipe, dev, [t.data_ptr() for t in dev], (N, d, K, n, P, M)


def _auto(pipe, ptrs, prm, method="mdl", cov=True, spec=True, eig=True):
    N, d, K, n, P, M = prm
    t = dict(cov=torch.full((n, N * N), -7.0, dtype=torch.complex64, device="cuda") if cov else None,
             spec=torch.full((n, P), -7.0, dtype=torch.float32, device="cuda") if spec else None,
             mx=torch.full((n, M), -7.0, dtype=torch.float32, device="cuda"),
             am=torch.full((n, M), -7.0, dtype=torch.float32, device="cuda"),
             cnt=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
             eig=torch.full((n, N), -7.0, dtype=torch.float32, device="cuda") if eig else None)
    ptr = lambda k: t[k].data_ptr() if t[k] is not None else None
    assert pipe.work_dev_auto(n, ptrs, ptr("mx"), ptr("am"), ptr("cnt"), method, ptr("cov"), ptr("spec"), ptr("eig"),
                              torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in t.items()}


def _work_dev(pipe, ptrs, prm):
    N, d, K, n, P, M = prm
    cov = torch.empty((n, N * N), dtype=torch.complex64, device="cuda")
    spec = torch.empty((n, P), dtype=torch.float32, device="cuda")
    mx = torch.empty((n, M), dtype=torch.float32, device="cuda")
    am = torch.empty((n, M), dtype=torch.float32, device="cuda")
    pipe.work_dev(n, ptrs, cov.data_ptr(), spec.data_ptr(), mx.data_ptr(), am.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in (cov, spec, mx, am)]


@pytest.mark.parametrize("method", ["mdl", "aic"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_auto_equals_the_chain_of_blocks(shape, method):
    pipe, dev, ptrs, prm = _setup(shape)
    N, d, K, n, P, M = prm
    fresh = _work_dev(_setup(shape)[0], ptrs, prm)                  # a handle that never saw an auto call
    got = _auto(pipe, ptrs, prm, method)
    assert _same(got["cov"], fresh[0])                               # K1 exactly as work_dev runs it
    # the chain, on the covariance the auto call wrote
    dR = torch.from_numpy(got["cov"]).cuda()
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    eig = torch.full((n, N), -7.0, dtype=torch.float32, device="cuda")
    spec = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    mx = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    am = torch.full((n, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    doa.source_count(N, K, method, M).work_dev(n, dR.data_ptr(), cnt.data_ptr(), eig.data_ptr(), st)
    doa.MUSIC_lin_array(d, 1, N, P).work_dev_counts(n, dR.data_ptr(), cnt.data_ptr(), spec.data_ptr(), st)
    doa.find_local_max(M, P, 0.0, 180.0).work_dev_counts(n, spec.data_ptr(), cnt.data_ptr(), mx.data_ptr(), am.data_ptr(), st)
    torch.cuda.synchronize()
    for key, want in (("cnt", cnt), ("eig", eig), ("spec", spec), ("mx", mx), ("am", am)):
        assert _same(got[key], want.cpu().numpy()), (shape, method, key)
    counts = got["cnt"]
    assert counts.min() >= 0 and counts.max() <= M
    # NaN padding: exactly the slots from the item's count on
    pad = np.arange(M)[None, :] >= counts[:, None]
    assert np.array_equal(np.isnan(got["mx"]), pad) and np.array_equal(np.isnan(got["am"]), pad)
    assert pad.any() or shape != "n4"                                # (the first shape has counts below num_targets)
    # optional outputs: the same peaks and counts without them
    lean = _auto(pipe, ptrs, prm, method, cov=False, spec=False, eig=False)
    for key in ("mx", "am", "cnt"):
        assert _same(lean[key], got[key]), (shape, method, key)
    # the ordinary entry after auto calls: bit-identical to the fresh handle's
    again = _work_dev(pipe, ptrs, prm)
    for a, b in zip(again, fresh):
        assert _same(a, b)


def test_end_to_end_two_sources():
    """First shape: MDL finds two sources in every snapshot, and both angles are within one bin of the fixed-M = 2 handle's."""
    pipe, dev, ptrs, prm = _setup("n4")
    N, d, K, n, P, M = prm
    got = _auto(pipe, ptrs, prm, "mdl")
    assert np.all(got["cnt"] == 2), got["cnt"]
    name = SHAPES["n4"][0]
    c = cases.CASES[name]
    fixed = doa.music_pipeline(N, K, c[4], c[5], d, 2, P, max_batch=n)
    _, _, mx2, am2 = _work_dev(fixed, ptrs, (N, d, K, n, P, 2))
    assert np.all(np.abs(got["am"][:, :2] - am2) <= 180.0 / P + 1e-4), np.abs(got["am"][:, :2] - am2).max()
    assert np.all(np.isnan(got["am"][:, 2]))
    assert np.all(np.abs(got["am"][:, :2] - np.array([123.0, 30.0])) <= 3.0)


def test_rejections():
    pipe, dev, ptrs, prm = _setup("n4")
    N, d, K, n, P, M = prm
    out = torch.zeros(n * M, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    with pytest.raises(doa.DoaError) as ei:                             # the count output is required
        pipe.work_dev_auto(n, ptrs, out.data_ptr(), out.data_ptr(), None)
    assert ei.value.status == -1
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_auto(n, ptrs, out.data_ptr(), out.data_ptr(), cnt.data_ptr(), method=2)
    assert ei.value.status == -1
    pipe.set_internal_precision(32)
    with pytest.raises(doa.DoaError) as ei:
        pipe.work_dev_auto(n, ptrs, out.data_ptr(), out.data_ptr(), cnt.data_ptr())
    assert ei.value.status == -4                                        # DOA_ERR_UNSUPPORTED
