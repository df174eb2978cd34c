"""The records a spectrum estimator keeps between its front and its scan (gr-doa_amd/csrc/spectrum_chain.hpp: spectrum_plan)
through doa_hip_spectrum_plan_debug: which records exist and how many bytes each takes per item, for MUSIC or Capon on a
uniform linear array or a steering table.  The four spectrum blocks and music_pipeline size their buffers from this one
function.  No device is needed.  The expected sizes are written here from the definitions in gr-doa_amd/csrc/kernels.hpp
(coef_stride, kChebRecord and music_uses_cheb, full_record_len) and include/doa_hip.h, not taken from the library."""
import ctypes as C
import itertools

import pytest

from doa import _lib

MUSIC, CAPON = 0, 1                     # DOA_ESTIMATOR_MUSIC / _CAPON
DOA_OK, DOA_ERR_INVALID_ARG, DOA_ERR_UNSUPPORTED = 0, -1, -4
DOA_MAX_ANT_ELE = 16
SIZES = range(2, DOA_MAX_ANT_ELE + 1)


def plan(estimator, table, N, bits, counted):
    """-> (status, {coef, cheb, full, status, coef_slot} in bytes per item)"""
    out = (C.c_longlong * 5)(*[-1] * 5)
    rc = _lib.lib.doa_hip_spectrum_plan_debug(estimator, int(table), N, bits, int(counted), out)
    return rc, dict(zip(("coef", "cheb", "full", "status", "coef_slot"), out))


def refused(estimator, table, bits, counted):
    """what the entries refuse: Capon, a table or counts at 32 bits; counts with a table or with Capon"""
    capon = estimator == CAPON
    return (bits == 32 and (capon or table or counted)) or (counted and (capon or table))


COMBOS = list(itertools.product((MUSIC, CAPON), (False, True), (64, 32), (False, True)))


@pytest.mark.parametrize("estimator,table,bits,counted", [c for c in COMBOS if not refused(*c)])
def test_record_sizes_at_every_array_size(estimator, table, bits, counted):
    for N in SIZES:
        rc, p = plan(estimator, table, N, bits, counted)
        assert rc == DOA_OK, (N, _lib.last_error())
        # coefficient record: [u0, Re u1, Im u1, ..., pad] = 2 N values, floats at 32 bits; a ULA's scan reads it, a table's does not
        assert p["coef"] == (0 if table else 2 * N * (8 if bits == 64 else 4)), N
        # its slot is sized as doubles whatever the precision is
        assert p["coef_slot"] == (0 if table else 2 * N * 8), N
        # Chebyshev record: 8 doubles, exactly for the lean scan kernel's shapes: a ULA of up to 4 elements in double
        assert p["cheb"] == (64 if (N <= 4 and bits == 64 and not table) else 0), N
        # full record: N^2 doubles, exactly for a table
        assert p["full"] == (8 * N * N if table else 0), N
        # status: one int32, exactly for Capon
        assert p["status"] == (4 if estimator == CAPON else 0), N


@pytest.mark.parametrize("estimator,table,bits,counted", [c for c in COMBOS if refused(*c)])
def test_refused_combinations_are_not_runnable(estimator, table, bits, counted):
    for N in SIZES:
        rc, p = plan(estimator, table, N, bits, counted)
        assert rc == DOA_ERR_UNSUPPORTED and not any(p.values()), (N, p)
        assert "hip_spectrum_plan_debug" in _lib.last_error()


def test_the_two_lists_cover_every_combination():
    ok = [c for c in COMBOS if not refused(*c)]
    # MUSIC on a ULA at 64 and 32 bits and counted at 64; Capon on a ULA, MUSIC and Capon on a table, at 64 bits
    assert len(COMBOS) == 16 and len(ok) == 6


@pytest.mark.parametrize("estimator,N,bits", [(2, 4, 64), (-1, 4, 64), (MUSIC, 1, 64), (MUSIC, DOA_MAX_ANT_ELE + 1, 64), (MUSIC, 4, 16)])
def test_unknown_estimators_sizes_and_precisions_are_not_runnable(estimator, N, bits):
    rc, p = plan(estimator, False, N, bits, False)
    assert rc == DOA_ERR_UNSUPPORTED and not any(p.values())


def test_bad_arguments():
    out = (C.c_longlong * 5)()
    f = _lib.lib.doa_hip_spectrum_plan_debug
    for args in [(MUSIC, 0, 4, 64, 0, None), (MUSIC, 2, 4, 64, 0, out), (MUSIC, 0, 4, 64, -1, out)]:
        assert f(*args) == DOA_ERR_INVALID_ARG, args
        assert "hip_spectrum_plan_debug" in _lib.last_error()
