"""CPU tests of the Root-MUSIC per-item-count and spatial-smoothing entries: the boundary headers declare them, the library
exports them, the binding maps them, and the Python wrappers exist with the documented signatures."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "doa_hip.h")
TEST_HEADER = os.path.join(ROOT, "include", "doa_hip_test.h")

_vp, _vpp, _i = C.c_void_p, C.POINTER(C.c_void_p), C.c_int
# name: (header, C parameter list with the names dropped, ctypes argument list)
ENTRIES = {
    "doa_rootMUSIC_linear_array_work_counts": (
        HEADER, "doa_rootMUSIC_linear_array_t *, int, const void *, const void *, void *", [_vp, _i, _vp, _vp, _vp]),
    "doa_rootMUSIC_linear_array_work_dev_counts": (
        HEADER, "doa_rootMUSIC_linear_array_t *, int, const void *, const void *, void *, int *, void *",
        [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "doa_rootMUSIC_linear_array_select_counts_debug": (
        TEST_HEADER, "doa_rootMUSIC_linear_array_t *, int, const void *, const void *, void *, int *",
        [_vp, _i, _vp, _vp, _vp, _vp]),
    "doa_root_pipeline_work_dev_auto": (
        HEADER, "doa_root_pipeline_t *, int, const void *const *, int, void *, void *, void *, void *, int *, void *",
        [_vp, _i, _vpp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "doa_root_pipeline_set_spatial_smoothing": (HEADER, "doa_root_pipeline_t *, int, int", [_vp, _i, _i]),
}


def _declared_types(path, name):
    """The parameter types of `DOA_HIP_API int name(...)` in the header, names dropped, blanks normalised."""
    code = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"DOA_HIP_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, name + " is not declared in " + os.path.basename(path)
    out = []
    for prm in m.group(1).split(","):
        prm = " ".join(prm.split())
        prm = re.sub(r"\b\w+$", "", prm).strip()              # the parameter's name
        out.append(re.sub(r"\s*\*\s*", " *", prm).replace("* *", "**").strip())
    return ", ".join(out)


def test_headers_declare_the_entries():
    for name, (path, types, _) in ENTRIES.items():
        want = ", ".join(re.sub(r"\s*\*\s*", " *", " ".join(t.split())).strip() for t in types.split(","))
        assert _declared_types(path, name) == want, name
    # the one test hook lives in the test header only
    public = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "select_counts_debug" not in public
    # the contracts are written down: status 2 and the smoothing caution
    src = open(HEADER).read()
    assert "status 2" in src and "no usable count" in src


def test_library_exports_the_entries_and_the_binding_maps_them():
    from doa import _lib
    for name, (_, _, args) in ENTRIES.items():
        assert hasattr(_lib.lib, name), name
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == args, name
    assert _lib.lib.doa_hip_abi_version() == 1


def test_python_wrappers_and_signatures():
    import doa
    sig = lambda f: list(inspect.signature(f).parameters)
    blk = doa.rootMUSIC_linear_array
    assert sig(blk.work_counts) == sig(doa.MUSIC_lin_array.work_counts) == ["self", "noutput_items", "input_items", "counts",
                                                                            "output_items"]
    assert sig(blk.work_dev_counts) == ["self", "noutput_items", "d_in_ptr", "d_counts_ptr", "d_out_ptr", "d_status_ptr", "stream"]
    assert sig(blk.select_counts_debug) == ["self", "roots", "counts"]
    pipe = doa.root_pipeline
    assert sig(pipe.set_spatial_smoothing) == sig(doa.music_pipeline.set_spatial_smoothing) == ["self", "subarray_size",
                                                                                               "forward_backward"]
    assert inspect.signature(pipe.set_spatial_smoothing).parameters["forward_backward"].default is True
    p = inspect.signature(pipe.work_dev_auto).parameters
    assert list(p) == ["self", "noutput_items", "d_input_ptrs", "d_angles_ptr", "d_count_ptr", "method", "d_cov_ptr", "d_eig_ptr",
                       "d_status_ptr", "stream"]
    assert p["method"].default == "mdl" and all(p[k].default is None for k in ("d_cov_ptr", "d_eig_ptr", "d_status_ptr", "stream"))
    # the sc16 class inherits both
    assert doa.root_music_pipeline_sc16.work_dev_auto is pipe.work_dev_auto
    assert doa.root_music_pipeline_sc16.set_spatial_smoothing is pipe.set_spatial_smoothing
