"""The GRC descriptors of the four calibration blocks keep the reference's interface: block keys, parameter keys and
defaults, make strings and port types (reference grc/doa_twinrx_phase_offset_est.xml:4-33, doa_findmax_and_save.xml:4-30,
doa_average_and_save.xml:4-30, doa_save_antenna_calib.xml:4-37; restated here as data, the XML text itself is this
repository's own).  Checked the way test_cpu_grc.py checks the hot-path blocks."""
import os
import re
import xml.etree.ElementTree as ET

import pytest

GRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-doa_amd", "grc")

EXPECT = {
    "doa_twinrx_phase_offset_est": dict(
        make="doa.twinrx_phase_offset_est($num_inputs, $n_skip_ahead)",
        params={"num_inputs": ("4", "raw"), "n_skip_ahead": ("8192", "raw")},
        sinks=[("complex", None, "$num_inputs")], sources=[("float", None, "$num_inputs-1")]),
    "doa_findmax_and_save": dict(
        make="doa.findmax_and_save($samples_to_findmax, $num_inputs, $config_filename)",
        params={"num_inputs": (None, "int"), "samples_to_findmax": (None, "int"), "config_filename": ("/tmp/phases.cfg", "file_save")},
        sinks=[("float", None, "$num_inputs")], sources=[]),
    "doa_average_and_save": dict(
        make="doa.average_and_save($samples_to_average, $num_inputs, $config_filename)",
        params={"num_inputs": (None, "int"), "samples_to_average": (None, "int"), "config_filename": ("/tmp/phases.cfg", "file_save")},
        sinks=[("float", None, "$num_inputs")], sources=[]),
    "doa_save_antenna_calib": dict(
        make="doa.save_antenna_calib($num_inputs, $config_filename, $samples_to_average)",
        params={"num_inputs": (None, "int"), "samples_to_average": (None, "int"), "config_filename": ("/tmp/antenna.cfg", "file_save")},
        sinks=[("float", "$num_inputs", None), ("float", "$num_inputs", None)], sources=[]),
}


def _ports(root, tag):
    return [(p.findtext("type"), p.findtext("vlen"), p.findtext("nports")) for p in root.findall(tag)]


@pytest.mark.parametrize("key", sorted(EXPECT))
def test_grc_descriptor_keeps_the_reference_interface(key):
    root = ET.parse(os.path.join(GRC, key + ".xml")).getroot()
    e = EXPECT[key]
    assert root.findtext("key") == key
    assert root.findtext("category") == "DoA"
    assert root.findtext("import") == "import doa"
    assert root.findtext("make").strip() == e["make"]
    params = {p.findtext("key"): (p.findtext("value"), p.findtext("type")) for p in root.findall("param")}
    assert params == e["params"]
    assert _ports(root, "sink") == e["sinks"] and _ports(root, "source") == e["sources"]
    assert set(re.findall(r"\$(\w+)", e["make"])) == set(params)      # every $variable of the make string is a parameter


def test_make_strings_name_constructors_the_package_has():
    import doa
    for key, e in EXPECT.items():
        name = re.match(r"doa\.(\w+)\(", e["make"]).group(1)
        assert callable(getattr(doa, name)), name
