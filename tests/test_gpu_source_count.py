"""GPU tests of doa.source_count against the fp64 reference of the criterion (tests/source_count_ref.py) on the shared
covariance cases (tests/source_count_cases.py).

Eigenvalues: |eig - ref| <= 2^-23 l_max(ref) per item -- the float rounding of the output is at most 2^-24 l_max, the double
Jacobi about 1e-13 l_max, so a factor two is in hand.  Counts: equal to the reference on every item whose reference margin
(best against runner-up criterion value) exceeds 1e-6 max(1, |best|), a thousand times what double rounding of the
eigenvalues can move the criterion by; at most 1 % of a case's items may fall under that margin (none does: the smallest
relative margin of these cases is 5e-4)."""
import numpy as np
import pytest
import torch

import doa
import source_count_cases as cases
import source_count_ref as ref

pytestmark = pytest.mark.gpu

METHODS = {"mdl": ref.MDL, "aic": ref.AIC}


def _run(name, method, kmax=None, R=None):
    N, K = cases.CASES[name][0], cases.CASES[name][3]
    R = cases.covariance(name) if R is None else R
    n = R.shape[0]
    blk = doa.source_count(N, K, method, kmax)
    cnt = np.full(n, -7, np.int32)
    eig = np.full((n, N), -7.0, np.float32)
    assert blk.work(n, [R], [cnt, eig]) == n
    return cnt, eig


def _check(name, method, cnt, eig, kmax=None):
    c_ref, e_ref, decided = cases.reference(name, METHODS[method], kmax)
    n = len(c_ref)
    lmax = e_ref[:, -1:]
    err = np.abs(eig.astype(np.float64) - e_ref)
    print(name, method, "max |eig - ref| / l_max = %.3g (bound %.3g); undecided %d of %d"
          % ((err / lmax).max(), 2.0 ** -23, (~decided).sum(), n))
    assert np.all(err <= 2.0 ** -23 * lmax), (name, (err / lmax).max())
    assert np.all(np.diff(eig, axis=1) >= 0), name
    assert (~decided).sum() <= 0.01 * n, (name, method, int((~decided).sum()))
    assert np.array_equal(cnt[decided], c_ref[decided]), (name, method, cnt, c_ref)


@pytest.mark.parametrize("method", ["mdl", "aic"])
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_counts_and_eigenvalues_match_the_reference(name, method):
    cnt, eig = _run(name, method)
    _check(name, method, cnt, eig)
    if name in cases.TABLE1 and method == "mdl":
        assert np.all(cnt == len(cases.CASES[name][1])), (name, cnt)        # MDL finds the true number on these


@pytest.mark.parametrize("name,kmax", [("n8_three", 1), ("n12_four_s0", 2), ("n4_two_fb", 1)])
def test_capped_count(name, kmax):
    cnt, eig = _run(name, "mdl", kmax)
    _check(name, "mdl", cnt, eig, kmax)
    assert cnt.max() <= kmax


@pytest.mark.parametrize("name", ["n4_two_fb", "n3_two", "n5_two_s0", "n12_four_s0", "n16_three_fb"])
def test_only_the_upper_triangle_is_read(name):
    N = cases.CASES[name][0]
    R = cases.covariance(name)
    Rg = R.copy().reshape(-1, N, N)               # [item][col][row]
    for col in range(N):
        for row in range(col + 1, N):
            Rg[:, col, row] = 1e3 + 7j
    a = _run(name, "mdl")
    b = _run(name, "mdl", R=Rg.reshape(R.shape))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["n4_one", "n2_one_s0", "n5_two_s1", "n9_two_s0", "n16_three_fb"])
def test_non_finite_and_zero_items(name):
    """A non-finite item: count -1, NaN eigenvalues, its wave neighbours untouched; an all-zero item: -1."""
    N = cases.CASES[name][0]
    R = cases.covariance(name)
    clean = _run(name, "aic")
    Rb = R.copy()
    Rb[3, 0 + 1 * N] = np.nan                      # (row 0, col 1): upper triangle
    Rb[6, (N - 1) + (N - 1) * N] = np.inf          # last diagonal entry
    Rb[9, :] = 0
    Rb[10, :] = -Rb[10, :]                         # negative definite: l_max < 0
    cnt, eig = _run(name, "aic", R=Rb)
    for i in (3, 6):
        assert cnt[i] == -1 and np.all(np.isnan(eig[i])), (name, i, cnt[i], eig[i])
    assert cnt[9] == -1 and np.all(eig[9] == 0.0)
    assert cnt[10] == -1 and np.all(eig[10] < 0.0)
    keep = np.ones(len(cnt), bool)
    keep[[3, 6, 9, 10]] = False
    assert np.array_equal(cnt[keep], clean[0][keep]) and np.array_equal(eig[keep], clean[1][keep])


@pytest.mark.parametrize("name", ["n4_two_fb", "n8_three", "n16_three_fb", "n2_one_s1"])
def test_host_entry_equals_device_entry(name):
    N, K = cases.CASES[name][0], cases.CASES[name][3]
    R = cases.covariance(name)
    n = R.shape[0]
    cnt, eig = _run(name, "mdl")
    blk = doa.source_count(N, K, "mdl")
    dR = torch.from_numpy(R.copy()).cuda()
    dc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    de = torch.full((n, N), -7.0, dtype=torch.float32, device="cuda")
    assert blk.work_dev(n, dR.data_ptr(), dc.data_ptr(), de.data_ptr(), torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy(), cnt) and np.array_equal(de.cpu().numpy(), eig)
    # the eigenvalue output is optional
    dc2 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert blk.work_dev(n, dR.data_ptr(), dc2.data_ptr(), None, torch.cuda.current_stream()) == n
    torch.cuda.synchronize()
    assert np.array_equal(dc2.cpu().numpy(), cnt)
    cnt3 = np.full(n, -7, np.int32)
    assert blk.work(n, [R], [cnt3]) == n and np.array_equal(cnt3, cnt)


def test_precision_32_is_unsupported():
    doa.set_internal_precision(32)
    try:
        blk = doa.source_count(4, 64, "mdl")
    finally:
        doa.set_internal_precision(64)
    R = cases.covariance("n4_one")
    with pytest.raises(doa.DoaError) as ei:
        blk.work(4, [R], [np.empty(4, np.int32)])
    assert ei.value.status == -4
