"""CPU tests of the C entries of the two fused handles (doa_music_pipeline_*, doa_root_pipeline_*), through doa._lib.lib
directly, in the style of test_cpu_block_entries.py: every entry other than create and destroy refuses a NULL handle with
DOA_ERR_INVALID_ARG and names itself in doa_last_error(), both creates refuse bad arguments before they look for a device,
destroy(NULL) is a no-op, and without a device a valid create fails loudly.  No compute is attempted."""
import ctypes as C

import numpy as np
import pytest

import doa
from doa import _lib

DOA_ERR_INVALID_ARG = -1

# handle -> (bad create argument tuples, one valid tuple)
#   music: (inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets, pspectrum_len, max_batch)
#   root:  (inputs, snapshot_size, overlap_size, avg_method, norm_spacing, num_targets, max_batch)
HANDLES = {
    "music_pipeline": ([(0, 64, 0, 0, 0.5, 1, 64, 8), (17, 64, 0, 0, 0.5, 1, 64, 8), (4, 64, 64, 0, 0.5, 1, 64, 8),
                        (4, 64, 0, 0, 0.5, 4, 64, 8), (4, 64, 0, 0, 0.6, 1, 64, 8), (4, 64, 0, 0, 0.5, 1, 64, 0),
                        (4, 64, 0, 0, 0.5, 1, 0, 8)], (4, 64, 0, 0, 0.5, 1, 64, 8)),
    "root_pipeline": ([(0, 64, 0, 0, 0.5, 1, 8), (17, 64, 0, 0, 0.5, 1, 8), (4, 64, 64, 0, 0.5, 1, 8),
                       (4, 64, 0, 0, 0.5, 4, 8), (4, 64, 0, 0, 0.6, 1, 8), (4, 64, 0, 0, 0.5, 1, 0)], (4, 64, 0, 0, 0.5, 1, 8)),
}
# the one entry that sets no message for a NULL handle (it may gain one that names it)
UNNAMED = ("fuse_antenna_correction",)


def _entries(handle):
    prefix = f"doa_{handle}_"
    names = [n for n in _lib.SIGNATURES if n.startswith(prefix) and n[len(prefix):] not in ("create", "destroy")]
    for suffix in ("work", "work_dev", "work_dev_auto", "work_dev_batches", "fuse_antenna_correction", "set_input_format",
                   "set_spatial_smoothing", "set_estimator", "set_lanes", "set_lane_streams", "synchronize", "inject_failure",
                   "lanes_idle", "set_internal_precision"):
        assert prefix + suffix in names
    return sorted(names)


def test_the_two_handles_have_the_entries_this_file_expects():
    # the fourteen shared ones; music adds set_stages and set_steering_table
    assert len(_entries("music_pipeline")) == 16 and len(_entries("root_pipeline")) == 14


@pytest.mark.parametrize("handle", sorted(HANDLES))
def test_every_entry_refuses_a_null_handle_and_names_itself(handle):
    buf = np.zeros(4096, np.uint8)                      # never read: the NULL handle is refused first
    by_type = {C.c_int: 1, C.c_float: 1.0, _lib._vp: buf.ctypes.data,
               _lib._vpp: C.cast(buf.ctypes.data, _lib._vpp)}
    for name in _entries(handle):
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and argtypes[0] is _lib._vp
        assert getattr(_lib.lib, name)(None, *[by_type[t] for t in argtypes[1:]]) == DOA_ERR_INVALID_ARG, name
        err = _lib.last_error()
        if name.endswith(UNNAMED):
            assert err == "" or name[len("doa_"):] in err, (name, err)
        else:
            assert name[len("doa_"):] in err, (name, err)
    getattr(_lib.lib, f"doa_{handle}_destroy")(None)    # a no-op


@pytest.mark.parametrize("handle", sorted(HANDLES))
def test_create_refuses_bad_arguments_before_the_device(handle):
    create = getattr(_lib.lib, f"doa_{handle}_create")
    for args in HANDLES[handle][0]:
        assert not create(*args), (handle, args)
        err = _lib.last_error()
        assert err.startswith(handle + ": bad ") and "no HIP device" not in err, (handle, args, err)


@pytest.mark.parametrize("handle", sorted(HANDLES))
def test_without_a_device_create_fails_loudly(handle):
    if doa.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert not getattr(_lib.lib, f"doa_{handle}_create")(*HANDLES[handle][1])
    assert "no CPU fallback" in _lib.last_error()


def test_the_batch_plan_entry_refuses_bad_arguments():
    """doa_hip_batch_plan_debug (the plan both handles' work_dev_batches run; no handle, so neither count above includes it)"""
    nb = 3
    outs = (C.c_void_p * (4 * nb))(*[0x1000 + 16 * i for i in range(4 * nb)])
    flags, caps = (C.c_ubyte * nb)(3, 3, 0), (C.c_int * nb)(4, 4, 1)
    grp, lane, sync, rot = (C.c_int * nb)(), (C.c_int * nb)(), (C.c_int * nb)(), C.c_int(0)
    good = [nb, outs, flags, caps, 2, 1, grp, lane, sync, C.byref(rot)]
    f = _lib.lib.doa_hip_batch_plan_debug
    assert f(*good) == 2 and list(grp) == [0, 0, 1] and _lib.last_error() == ""
    bad = [(0, -1), (4, 0), (4, 9), (5, -1), (5, 2), (2, (C.c_ubyte * nb)(1, 8, 0)), (3, (C.c_int * nb)(4, 0, 1))]
    bad += [(i, None) for i in (1, 2, 3, 6, 7, 8, 9)]
    for i, value in bad:
        args = list(good)
        args[i] = value
        assert f(*args) == DOA_ERR_INVALID_ARG, (i, value)
        assert "hip_batch_plan_debug" in _lib.last_error()
