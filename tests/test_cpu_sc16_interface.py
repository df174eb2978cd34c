"""CPU tests of the sc16 (complex int16) input format: the boundary header declares the three
doa_*_set_input_format entries and the DOA_SAMPLE_* macros, the library exports them and the binding maps them;
the three sc16 GRC descriptors are their complex counterparts plus a scale and an sc16 sink; the Python blocks
exist with the documented signatures; doa.sim.to_sc16 / from_sc16 round, saturate and widen as specified."""
import inspect
import os
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "doa_hip.h")
GRC = os.path.join(ROOT, "gr-doa_amd", "grc")
SETTERS = ("doa_autocorrelate_set_input_format", "doa_music_pipeline_set_input_format",
           "doa_root_pipeline_set_input_format")


def test_header_declares_the_format_and_the_setters():
    src = open(HEADER).read()
    assert re.search(r"#define\s+DOA_SAMPLE_FC32\s+0\b", src)
    assert re.search(r"#define\s+DOA_SAMPLE_SC16\s+1\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for blk, name in zip(("autocorrelate", "music_pipeline", "root_pipeline"), SETTERS):
        assert re.search(r"DOA_HIP_API\s+int\s+%s\s*\(\s*doa_%s_t\s*\*\s*h\s*,\s*int\s+format\s*,\s*float\s+scale\s*\)\s*;"
                         % (name, blk), code), name


def test_library_exports_the_setters_and_the_binding_maps_them():
    import ctypes as C
    from doa import _lib
    for name in SETTERS:
        assert hasattr(_lib.lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_float]
    assert _lib.lib.doa_hip_abi_version() == 1


def test_python_blocks_and_signatures():
    import doa
    for cls in (doa.autocorrelate, doa.music_pipeline, doa.root_pipeline):
        assert list(inspect.signature(cls.set_input_format).parameters) == ["self", "fmt", "scale"]
        assert inspect.signature(cls.set_input_format).parameters["scale"].default is None
    p = inspect.signature(doa.autocorrelate_sc16).parameters
    assert list(p) == ["inputs", "snapshot_size", "overlap_size", "avg_method", "scale"] and p["scale"].default == 2.0 ** -15
    p = inspect.signature(doa.music_pipeline_sc16).parameters
    assert list(p) == ["inputs", "snapshot_size", "overlap_size", "avg_method", "norm_spacing", "num_targets",
                       "pspectrum_len", "scale", "max_batch"]
    assert p["scale"].default == 2.0 ** -15 and p["max_batch"].default == 4096
    p = inspect.signature(doa.root_music_pipeline_sc16).parameters
    assert list(p) == ["inputs", "snapshot_size", "overlap_size", "avg_method", "norm_spacing", "num_targets", "scale",
                       "max_batch"]
    assert issubclass(doa.autocorrelate_sc16, doa.autocorrelate)
    assert issubclass(doa.music_pipeline_sc16, doa.music_pipeline)
    assert issubclass(doa.root_music_pipeline_sc16, doa.root_pipeline)


def test_sc16_constructors_validate_arguments_before_the_device():
    import doa
    for cls, args in [(doa.autocorrelate_sc16, (0, 16, 0, 0)), (doa.music_pipeline_sc16, (4, 16, 16, 0, 0.5, 1, 64)),
                      (doa.root_music_pipeline_sc16, (4, 16, 0, 0, 0.5, 4))]:
        with pytest.raises(doa.DoaError) as ei:
            cls(*args)
        assert "no HIP device" not in str(ei.value)


def _ports(root, tag):
    return [(p.findtext("type"), p.findtext("vlen"), p.findtext("nports")) for p in root.findall(tag)]


@pytest.mark.parametrize("key,base,make", [
    ("doa_autocorrelate_sc16", "doa_autocorrelate",
     "doa.autocorrelate_sc16($inputs, $snapshot_size, $overlap_size, $avg_method, $scale)"),
    ("doa_music_pipeline_sc16", "doa_music_pipeline",
     "doa.music_pipeline_sc16($inputs, $snapshot_size, $overlap_size, $avg_method, $norm_spacing, $num_targets, "
     "$pspectrum_len, $scale)"),
    ("doa_root_music_pipeline_sc16", "doa_root_music_pipeline",
     "doa.root_music_pipeline_sc16($inputs, $snapshot_size, $overlap_size, $avg_method, $norm_spacing, $num_targets, $scale)"),
])
def test_sc16_grc_descriptors(key, base, make):
    root = ET.parse(os.path.join(GRC, key + ".xml")).getroot()
    ref = ET.parse(os.path.join(GRC, base + ".xml")).getroot()
    assert root.findtext("key") == key
    assert root.findtext("import") == "import doa"
    assert root.findtext("make").strip() == make
    params = {p.findtext("key"): p.findtext("value") for p in root.findall("param")}
    ref_params = {p.findtext("key"): p.findtext("value") for p in ref.findall("param")}
    assert params == dict(ref_params, scale="1.0/32768")
    assert [c.text for c in root.findall("check")] == [c.text for c in ref.findall("check")] + ["$scale > 0"]
    assert _ports(root, "sink") == [("sc16", None, "$inputs")]
    assert _ports(root, "source") == _ports(ref, "source")
    assert set(re.findall(r"\$(\w+)", make)) == set(params)


def test_to_sc16_rounds_half_to_even_and_saturates():
    from doa.sim import to_sc16
    s = 2.0 ** -15
    x = np.array([0.5 * s, 1.5 * s, 2.5 * s, -0.5 * s, -1.5 * s, -2.5 * s, 3.49 * s, -3.51 * s], np.float64)
    q = to_sc16(x.astype(np.complex128) + 1j * x[::-1], s)
    assert q.dtype == np.int16 and q.shape == (8, 2)
    assert q[:, 0].tolist() == [0, 2, 2, 0, -2, -2, 3, -4]
    assert q[:, 1].tolist() == [-4, 3, -2, -2, 0, 2, 2, 0]
    big = np.array([1.0, -1.0, 5.0, -5.0, 0.999969482421875, -1.0000305], np.float32)
    q = to_sc16(big + 0j, s)
    assert q[:, 0].tolist() == [32767, -32768, 32767, -32768, 32767, -32768]
    assert np.all(q[:, 1] == 0)
    q = to_sc16(np.array([100.0 + 0j]), 1.0 / 32767)                       # a driver's own factor
    assert q.tolist() == [[32767, 0]]


def test_from_sc16_is_the_float32_product_and_round_trips():
    from doa.sim import from_sc16, to_sc16
    rng = np.random.default_rng(3)
    q = rng.integers(-32768, 32768, size=(3, 257, 2)).astype(np.int16)
    q[0, :4] = [[32767, -32768], [-32768, 32767], [0, 0], [-1, 1]]
    for s in (2.0 ** -15, 1.0 / 32767, 1.0, 3.0e-5):
        x = from_sc16(q, s)
        assert x.dtype == np.complex64 and x.shape == (3, 257)
        assert np.array_equal(x.real, q[..., 0].astype(np.float32) * np.float32(s))
        assert np.array_equal(x.imag, q[..., 1].astype(np.float32) * np.float32(s))
        # flat 2n layout: the same samples
        assert np.array_equal(from_sc16(q[1].reshape(-1), s), x[1])
    # exact round trip: every int16 value is representable after a power-of-two scale
    for s in (2.0 ** -15, 1.0, 2.0 ** -10):
        assert np.array_equal(to_sc16(from_sc16(q, s), s), q)
    # full scale maps to [-1, 1) with the default scale
    x = from_sc16(np.array([[32767, -32768]], np.int16))
    assert x[0].real == np.float32(32767 / 32768) and x[0].imag == -1.0


def test_torch_forms_match_numpy():
    torch = pytest.importorskip("torch")
    from doa.sim import from_sc16, to_sc16
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 300)) + 1j * rng.standard_normal((2, 300))).astype(np.complex64) * 0.3
    x[0, 0] = 3.0 + 0.5j * 2.0 ** -15                                     # saturates / ties to even
    for s in (2.0 ** -15, 1.0 / 32767):
        qn = to_sc16(x, s)
        qt = to_sc16(torch.from_numpy(x), s)
        assert qt.dtype == torch.int16 and np.array_equal(qt.numpy(), qn)
        xt = from_sc16(qt, s)
        assert xt.dtype == torch.complex64 and np.array_equal(xt.numpy(), from_sc16(qn, s))
