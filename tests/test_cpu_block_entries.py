"""CPU tests of the C entries of the ten blocks that take one item stream (covariance items or spectra), through
doa._lib.lib directly: create refuses bad arguments before it looks for a device, every work* / *_debug entry refuses a NULL
handle with DOA_ERR_INVALID_ARG and names itself in doa_last_error(), and without a device a valid create fails loudly.
Extends what test_cpu_abi.py asserts for four blocks to all ten.  No compute is attempted."""
import ctypes as C

import numpy as np
import pytest

import doa
from doa import _lib

DOA_ERR_INVALID_ARG = -1

_TABLE = np.ones((8, 4, 2), np.float64)                 # a finite steering table: 8 bins, 4 elements, (re, im)
_TABLE[..., 1] = 0.0
_TABLE_PTR = _TABLE.ctypes.data

# block -> (bad create argument tuples, one valid tuple)
BLOCKS = {
    "MUSIC_lin_array": ([(0.5, 4, 4, 64), (0.6, 1, 4, 64), (0.5, 1, 4, 0), (0.5, 1, 17, 64)], (0.5, 1, 4, 64)),
    "capon_lin_array": ([(0.5, 1, 64, 0.0), (0.6, 4, 64, 0.0), (0.5, 4, 0, 0.0), (0.5, 4, 64, -1.0)], (0.5, 4, 64, 0.0)),
    "MUSIC_array": ([(1, 1, 8, _TABLE_PTR), (4, 4, 8, _TABLE_PTR), (1, 4, 0, _TABLE_PTR), (1, 4, 8, None)], (1, 4, 8, _TABLE_PTR)),
    "capon_array": ([(1, 8, _TABLE_PTR, 0.0), (4, 0, _TABLE_PTR, 0.0), (4, 8, None, 0.0), (4, 8, _TABLE_PTR, -1.0)],
                    (4, 8, _TABLE_PTR, 0.0)),
    "rootMUSIC_linear_array": ([(0.5, 4, 4), (0.7, 1, 4), (0.5, 0, 4), (0.5, 1, 17)], (0.5, 1, 4)),
    "esprit_linear_array": ([(0.5, 1, 1), (0.5, 4, 4), (0.7, 1, 4), (0.5, 1, 17)], (0.5, 1, 4)),
    "source_count": ([(1, 64, 0, 1), (4, 1, 0, 1), (4, 64, 2, 1), (4, 64, 0, 4), (17, 64, 0, 1)], (4, 64, 0, 3)),
    "spatial_smooth": ([(4, 1, 0), (4, 5, 0), (4, 3, 2), (17, 3, 0)], (4, 3, 0)),
    "calibrate_lin_array": ([(0.5, 1, 45.0), (0.5, 17, 45.0), (0.6, 4, 45.0), (0.0, 4, 45.0)], (0.5, 4, 45.0)),
    "find_local_max": ([(0, 64, 0.0, 1.0), (2, 0, 0.0, 1.0), (2, 64, 1.0, 1.0), (17, 64, 0.0, 1.0)], (1, 64, 0.0, 180.0)),
}


def _entries(block):
    """Every exported work* / *_debug entry of the block (the binding mirrors the headers one to one)."""
    prefix = f"doa_{block}_"
    names = [n for n in _lib.SIGNATURES
             if n.startswith(prefix) and (n[len(prefix):].startswith("work") or n.endswith("_debug"))]
    assert f"{prefix}work" in names and f"{prefix}work_dev" in names
    return sorted(names)


def test_the_table_covers_the_ten_item_blocks():
    assert len(BLOCKS) == 10
    for block in BLOCKS:
        for suffix in ("create", "destroy", "work", "work_dev"):
            assert f"doa_{block}_{suffix}" in _lib.SIGNATURES
    # 10 work + 10 work_dev, the counts pairs of MUSIC_lin_array / rootMUSIC / esprit / find_local_max, 8 debug entries
    assert sum(len(_entries(b)) for b in BLOCKS) == 36


@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_create_refuses_bad_arguments_before_the_device(block):
    create = getattr(_lib.lib, f"doa_{block}_create")
    for args in BLOCKS[block][0]:
        assert not create(*args), (block, args)
        err = _lib.last_error()
        assert err and "no HIP device" not in err, (block, args, err)


@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_every_entry_refuses_a_null_handle_and_names_itself(block):
    buf = np.zeros(4096, np.uint8)                      # never read: the NULL handle is refused first
    p = buf.ctypes.data
    for name in _entries(block):
        fn = getattr(_lib.lib, name)
        argtypes = _lib.SIGNATURES[name][1]
        assert argtypes[0] is C.c_void_p and argtypes[1] is C.c_int
        rest = [p] * (len(argtypes) - 2)
        for n in (1, 0):
            assert fn(None, n, *rest) == DOA_ERR_INVALID_ARG, (name, n)
            assert name[len("doa_"):] in _lib.last_error(), (name, _lib.last_error())
    # destroy(NULL) is a no-op
    getattr(_lib.lib, f"doa_{block}_destroy")(None)


@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_without_a_device_create_fails_loudly(block):
    if doa.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert not getattr(_lib.lib, f"doa_{block}_create")(*BLOCKS[block][1])
    assert "no CPU fallback" in _lib.last_error()
