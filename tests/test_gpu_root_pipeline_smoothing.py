"""GPU tests of root_pipeline.set_spatial_smoothing on the coherent scenarios of tests/spatial_smooth_ref.py: work_dev,
work_dev_batches, work and work_dev_auto of a smoothed handle are BIT-IDENTICAL to the chain autocorrelate ->
spatial_smooth(N, S, fb) -> rootMUSIC_linear_array(d, M, S) made by hand, the covariance output is the unsmoothed handle's,
and the product does what the feature is for: it finds coherent sources the unsmoothed Root-MUSIC misses by tens of degrees.

Scenarios A, C and A_forward.  Scenario B (N = 4, S = 3, M = 2) is left out on purpose: with forward-backward smoothing and
num_targets = S - 1 there is ONE noise vector, it is conjugate-symmetric, and the polynomial's roots lie ON the unit circle
(the fp64 reference roots of B are 3e-10 from it), so Root-MUSIC's "strictly inside" rule flips a coin per root and no
reference decides the angles (choose S >= num_targets + 2)."""
import functools

import numpy as np
import pytest
import torch

import doa
import doa_oracle as oracle
import spatial_smooth_ref as ref

pytestmark = pytest.mark.gpu

K, D, NS = ref.K, ref.D, ref.N_SNAP
NAMES = ["A", "A_forward", "C"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _dev_streams(name):
    return tuple(doa.sim.stream_slab_torch([_dev(a) for a in ref.streams(name)]))


def _pipe(name, smoothed=True):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    p = doa.root_pipeline(N, K, 0, 0, D, len(th), max_batch=NS)
    if smoothed:
        p.set_spatial_smoothing(S, fb)
    return p


def _work_dev(pipe, name):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    cov = torch.full((NS, N * N), -7.0, dtype=torch.complex64, device="cuda")
    ang = torch.full((NS, len(th)), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in _dev_streams(name)]
    assert pipe.work_dev(NS, ptrs, cov.data_ptr(), ang.data_ptr(), st.data_ptr(), torch.cuda.current_stream()) == NS
    torch.cuda.synchronize()
    return dict(cov=cov.cpu().numpy(), ang=ang.cpu().numpy(), st=st.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _smoothed_run(name):
    return _work_dev(_pipe(name), name)


@functools.lru_cache(maxsize=None)
def _plain_run(name):
    return _work_dev(_pipe(name, smoothed=False), name)


@functools.lru_cache(maxsize=None)
def _chain(name):
    """autocorrelate -> spatial_smooth -> rootMUSIC_linear_array(d, M, S): three block handles on the device."""
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    s = torch.cuda.current_stream()
    cov = torch.full((NS, N * N), -7.0, dtype=torch.complex64, device="cuda")
    sm = torch.full((NS, S * S), -7.0, dtype=torch.complex64, device="cuda")
    ang = torch.full((NS, M), -7.0, dtype=torch.float32, device="cuda")
    assert doa.autocorrelate(N, K, 0, 0).work_dev(NS, [t.data_ptr() for t in _dev_streams(name)], cov.data_ptr(), s) == NS
    doa.spatial_smooth(N, S, fb).work_dev(NS, cov.data_ptr(), sm.data_ptr(), s)
    doa.rootMUSIC_linear_array(D, M, S).work_dev(NS, sm.data_ptr(), ang.data_ptr(), s)
    torch.cuda.synchronize()
    return dict(cov=cov.cpu().numpy(), sm=sm.cpu().numpy(), ang=ang.cpu().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_equals_the_chain_of_blocks(name):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    want, plain, got = _chain(name), _plain_run(name), _smoothed_run(name)
    assert _same(want["sm"], ref.smooth(want["cov"], N, S, fb))
    assert _same(got["cov"], plain["cov"]) and _same(got["cov"], want["cov"])      # d_cov_out: the N x N covariance, unchanged
    assert _same(got["ang"], want["ang"]) and not got["st"].any()
    assert not _same(got["ang"], plain["ang"])
    pipe = _pipe(name)
    x = ref.streams(name)
    # host entry
    h_ang, h_cov = np.full((NS, M), -7.0, np.float32), np.full((NS, N * N), -7.0, np.complex64)
    assert pipe.work(NS, [x[k] for k in range(N)], h_ang, cov_out=h_cov) == NS
    assert _same(h_ang, want["ang"]) and _same(h_cov, want["cov"])
    # three batches of eight, on the caller's stream alone and over four lanes
    nb, n = 3, NS // 3
    ins = [[t.data_ptr() + b * n * K * 8 for t in _dev_streams(name)] for b in range(nb)]
    for lanes in (1, 4):
        pipe.set_lanes(lanes)
        cov = torch.full((NS, N * N), -7.0, dtype=torch.complex64, device="cuda")
        ang = torch.full((NS, M), -7.0, dtype=torch.float32, device="cuda")
        st = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
        rows = lambda t, per: [t.data_ptr() + b * n * per * t.element_size() for b in range(nb)]
        assert pipe.work_dev_batches(n, ins, rows(cov, N * N), rows(ang, M), rows(st, 1), torch.cuda.current_stream()) == NS
        torch.cuda.synchronize()
        assert _same(cov.cpu().numpy(), want["cov"]) and _same(ang.cpu().numpy(), want["ang"]), (name, lanes)
        assert not st.cpu().numpy().any()
    # switched off again: a fresh unsmoothed handle's outputs
    pipe.set_spatial_smoothing(0, 0)
    off = _work_dev(pipe, name)
    for key in ("cov", "ang", "st"):
        assert _same(off[key], plain[key]), (name, "off", key)


def _auto(pipe, name, n_eig, method="mdl"):
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    t = dict(cov=torch.full((NS, N * N), -7.0, dtype=torch.complex64, device="cuda"),
             ang=torch.full((NS, M), -7.0, dtype=torch.float32, device="cuda"),
             cnt=torch.full((NS,), -7, dtype=torch.int32, device="cuda"),
             eig=torch.full((NS, n_eig), -7.0, dtype=torch.float32, device="cuda"),
             st=torch.full((NS,), -7, dtype=torch.int32, device="cuda"))
    ptrs = [v.data_ptr() for v in _dev_streams(name)]
    assert pipe.work_dev_auto(NS, ptrs, t["ang"].data_ptr(), t["cnt"].data_ptr(), method, t["cov"].data_ptr(), t["eig"].data_ptr(),
                              t["st"].data_ptr(), torch.cuda.current_stream()) == NS
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


@pytest.mark.parametrize("method", ["mdl", "aic"])
@pytest.mark.parametrize("name", NAMES)
def test_auto_on_a_smoothed_handle_equals_the_chain(name, method):
    """K in the criterion stays snapshot_size; the eigenvalues are S per item."""
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    got = _auto(_pipe(name), name, S, method)
    chain = _chain(name)
    assert _same(got["cov"], chain["cov"])
    s = torch.cuda.current_stream()
    sm = _dev(chain["sm"])
    cnt = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
    eig = torch.full((NS, S), -7.0, dtype=torch.float32, device="cuda")
    ang = torch.full((NS, M), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
    doa.source_count(S, K, method, M).work_dev(NS, sm.data_ptr(), cnt.data_ptr(), eig.data_ptr(), s)
    doa.rootMUSIC_linear_array(D, M, S).work_dev_counts(NS, sm.data_ptr(), cnt.data_ptr(), ang.data_ptr(), st.data_ptr(), s)
    torch.cuda.synchronize()
    for key, want in (("cnt", cnt), ("eig", eig), ("ang", ang), ("st", st)):
        assert _same(got[key], want.cpu().numpy()), (name, method, key)


def test_rejections_leave_the_handle_as_it_was():
    name = "A"
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    for smoothed in (False, True):
        pipe = _pipe(name, smoothed)
        want = _smoothed_run(name) if smoothed else _plain_run(name)
        for bad in ((1, 1), (N + 1, 1), (M, 1), (S, 2)):
            with pytest.raises(doa.DoaError) as ei:
                pipe.set_spatial_smoothing(*bad)
            assert ei.value.status == -1, bad
            got = _work_dev(pipe, name)
            for key in ("cov", "ang", "st"):
                assert _same(got[key], want[key]), (smoothed, bad, key)


@pytest.mark.parametrize("name", ["A", "C"])
def test_end_to_end_coherent_sources(name):
    """Without smoothing Root-MUSIC misses a true direction by more than 10 degrees (the fp64 oracle on the CPU: 59.6 and 62.7);
    smoothed, work_dev_auto reports the true count on all 24 snapshots and every angle is within 0.2 degrees of the truth (the
    fp64 oracle: 0.034 and 0.016), and within 1e-3 degrees of oracle.root_music on the smoothed items."""
    N, S, fb, th, rho = ref.SCENARIOS[name]
    M = len(th)
    e_raw = ref.angle_error(_plain_run(name)["ang"], th)
    auto = _auto(_pipe(name), name, S)
    e_auto = ref.angle_error(auto["ang"], th)
    a64 = oracle.root_music(_chain(name)["sm"], D, M, S, "f64")
    e_64 = float(np.abs(auto["ang"].astype(np.float64) - a64).max())
    print(name, "unsmoothed: max angle error %.3f deg; smoothed auto: counts %s, max angle error %.4f deg, against the fp64 "
          "oracle %.3g deg" % (e_raw, np.unique(auto["cnt"]), e_auto, e_64))
    assert e_raw > 10.0
    assert np.all(auto["cnt"] == M), auto["cnt"]
    assert not auto["st"].any()
    assert e_auto <= 0.2
    assert e_64 <= 1e-3
