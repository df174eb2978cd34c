"""CPU tests of music_pipeline's grid mode: the two entries it adds (doa_pipeline_set_steering_grid, the hook
doa_hip_array_grid_debug) are bound and exported, refuse bad arguments before they look for a device and name themselves,
the count of doa_music_pipeline_* entries is what test_cpu_pipeline_entries.py pins, and the numpy side of the contract the
GPU test demands of the pipeline: MUSIC on a steering grid followed by the two-dimensional peak pick finds every source of
the three circular scenarios within one cell.  No device needed."""
import ctypes as C

import numpy as np
import pytest

import array_ref as ref
import peaks2d_ref as p2
from doa import _lib

DOA_ERR_INVALID_ARG = -1
NEW = ("doa_pipeline_set_steering_grid", "doa_hip_array_grid_debug")


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_both_entries_are_bound_and_exported():
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.SIGNATURES[NEW[0]][0] is C.c_int and len(_lib.SIGNATURES[NEW[0]][1]) == 9
    assert _lib.SIGNATURES[NEW[1]][0] is C.c_int and len(_lib.SIGNATURES[NEW[1]][1]) == 17


def test_the_music_pipeline_prefix_still_counts_sixteen_entries():
    prefix = "doa_music_pipeline_"
    names = [n for n in _lib.SIGNATURES if n.startswith(prefix) and n[len(prefix):] not in ("create", "destroy")]
    assert len(names) == 16 and not NEW[0].startswith(prefix)


def test_the_setter_refuses_a_null_handle_and_names_itself():
    table = np.ones((8, 4), np.complex128)
    assert _lib.lib.doa_pipeline_set_steering_grid(None, _vp(table), 4, 2, 0.0, 360.0, 0.0, 90.0, 1) == DOA_ERR_INVALID_ARG
    assert "pipeline_set_steering_grid" in _lib.last_error()


def test_the_hook_refuses_bad_arguments_before_the_device():
    N, n_az, n_el, M, n = 4, 4, 2, 2, 3
    table = np.exp(1j * np.arange(n_az * n_el * N, dtype=np.float64)).reshape(n_az * n_el, N)
    nan_table = table.copy(); nan_table[5, 2] = np.nan
    rec = np.zeros((n, N * N), np.float64)
    spec = np.empty((n, n_az * n_el), np.float32)
    val, az, el = (np.empty((n, M), np.float32) for _ in range(3))
    # (num_ant_ele, steering, n_az, n_el, az_min, az_max, el_min, el_max, wrap, M, n_items, records, fused, spec, val, az, el)
    good = [N, table, n_az, n_el, 0.0, 360.0, 0.0, 90.0, 1, M, n, rec, 1, spec, val, az, el]
    bad = {"N = 1": (0, 1), "N = 17": (0, 17), "a NULL table": (1, None), "a NaN in the table": (1, nan_table), "n_az = 0": (2, 0),
           "az_max = az_min": (5, 0.0), "az_max < az_min": (5, -10.0), "M = 0": (9, 0), "M = 17": (9, 17), "NULL records": (11, None),
           "NULL values": (14, None), "NULL azimuths": (15, None), "NULL elevations": (16, None)}
    for what, (i, value) in bad.items():
        args = list(good)
        args[i] = value
        if what.startswith("N = "):                     # a table of the matching width, so that only N is at fault
            args[1] = np.ones((n_az * n_el, value), np.complex128)
            args[11] = np.zeros((n, value * value), np.float64)
        call = [_vp(a) if isinstance(a, np.ndarray) else a for a in args]
        assert _lib.lib.doa_hip_array_grid_debug(*call) == DOA_ERR_INVALID_ARG, what
        err = _lib.last_error()
        assert "hip_array_grid_debug" in err and "no HIP device" not in err and "no CPU fallback" not in err, (what, err)


@pytest.mark.parametrize("name", sorted(p2.CIRCULAR))
def test_the_numpy_chain_finds_every_source_within_one_cell(name):
    """array_ref.music then peaks2d_ref.find_local_max_2d on 72 x 18: what test_gpu_pipeline_grid.py asks of the pipeline."""
    assert NEW[0] in _lib.SIGNATURES                     # the entry this is the statement for
    N, radius, sources = p2.CIRCULAR[name]
    n, M = 15, len(sources)
    table = p2.grid_table(p2.circular_positions(N, radius))
    R = p2.covariances(p2.streams(name, n), n)
    spec, _, _ = ref.music(R, table, M)
    val, az, el = p2.find_local_max_2d(spec.astype(np.float32), M, p2.N_AZ, p2.N_EL)
    for d in range(n):
        assert val[d, 0] == 0.0 and p2.sources_found(az[d], el[d], sources), (name, d, val[d], az[d], el[d])
