"""The records a grid-free estimator keeps between its eigen launch and its solver kernel (gr-doa_amd/csrc/gridfree_chain.hpp:
gridfree_plan) through doa_hip_gridfree_plan_debug: which records exist and how many bytes each takes per item, for Root-MUSIC
or ESPRIT.  rootMUSIC_linear_array, esprit_linear_array and root_pipeline size their buffers from this one function.  No device
is needed.  The expected sizes are written here from the definitions in gr-doa_amd/csrc/kernels.hpp (coef_stride,
subspace_record_len) and the refusals of the entries (include/doa_hip.h), not taken from the library."""
import ctypes as C
import itertools

import pytest

from doa import _lib

ROOT_MUSIC, ESPRIT = 0, 1               # DOA_GRIDFREE_ROOT_MUSIC / _ESPRIT
DOA_OK, DOA_ERR_INVALID_ARG, DOA_ERR_UNSUPPORTED = 0, -1, -4
DOA_MAX_ANT_ELE = 16
SIZES = range(2, DOA_MAX_ANT_ELE + 1)


def plan(estimator, N, bits, counted):
    """-> (status, {coef, rec, status} in bytes per item)"""
    out = (C.c_longlong * 3)(*[-1] * 3)
    rc = _lib.lib.doa_hip_gridfree_plan_debug(estimator, N, bits, int(counted), out)
    return rc, dict(zip(("coef", "rec", "status"), out))


def refused(estimator, bits, counted):
    """what the entries refuse: ESPRIT at 32 bits, counts at 32 bits"""
    return bits == 32 and (estimator == ESPRIT or counted)


COMBOS = list(itertools.product((ROOT_MUSIC, ESPRIT), (64, 32), (False, True)))


@pytest.mark.parametrize("estimator,bits,counted", [c for c in COMBOS if not refused(*c)])
def test_record_sizes_at_every_array_size(estimator, bits, counted):
    for N in SIZES:
        rc, p = plan(estimator, N, bits, counted)
        assert rc == DOA_OK, (N, _lib.last_error())
        # coefficient record: [u0, Re u1, Im u1, ..., pad] = 2 N doubles whatever the precision is (the root finder reads doubles)
        assert p["coef"] == (2 * N * 8 if estimator == ROOT_MUSIC else 0), N
        # signal-subspace record: N eigenvectors of N complex doubles
        assert p["rec"] == (2 * N * N * 8 if estimator == ESPRIT else 0), N
        # status: one int32 per item for either estimator
        assert p["status"] == 4, N


@pytest.mark.parametrize("estimator,bits,counted", [c for c in COMBOS if refused(*c)])
def test_refused_combinations_are_not_runnable(estimator, bits, counted):
    for N in SIZES:
        rc, p = plan(estimator, N, bits, counted)
        assert rc == DOA_ERR_UNSUPPORTED and not any(p.values()), (N, p)
        assert "hip_gridfree_plan_debug" in _lib.last_error()


def test_the_two_lists_cover_every_combination():
    ok = [c for c in COMBOS if not refused(*c)]
    # Root-MUSIC at 64 and 32 bits and counted at 64; ESPRIT at 64 bits, fixed and counted
    assert len(COMBOS) == 8 and len(ok) == 5
    assert sorted(ok) == sorted([(ROOT_MUSIC, 64, False), (ROOT_MUSIC, 32, False), (ROOT_MUSIC, 64, True), (ESPRIT, 64, False),
                                 (ESPRIT, 64, True)])


@pytest.mark.parametrize("estimator,N,bits", [(2, 4, 64), (-1, 4, 64), (ROOT_MUSIC, 1, 64), (ESPRIT, 1, 64),
                                              (ROOT_MUSIC, DOA_MAX_ANT_ELE + 1, 64), (ESPRIT, DOA_MAX_ANT_ELE + 1, 64),
                                              (ROOT_MUSIC, 4, 16), (ESPRIT, 4, 0)])
def test_unknown_estimators_sizes_and_precisions_are_not_runnable(estimator, N, bits):
    rc, p = plan(estimator, N, bits, False)
    assert rc == DOA_ERR_UNSUPPORTED and not any(p.values())


def test_bad_arguments():
    out = (C.c_longlong * 3)()
    f = _lib.lib.doa_hip_gridfree_plan_debug
    for args in [(ROOT_MUSIC, 4, 64, 0, None), (ROOT_MUSIC, 4, 64, 2, out), (ESPRIT, 4, 64, -1, out)]:
        assert f(*args) == DOA_ERR_INVALID_ARG, args
        assert "hip_gridfree_plan_debug" in _lib.last_error()
