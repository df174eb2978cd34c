"""CPU tests of the steering-table estimators: the numpy statement (tests/array_ref.py) has the properties the feature is
for -- on every scenario both spectra peak at the true azimuths, a linear array cannot tell an azimuth from its mirror image
and a circular one can -- and the parts of the product that need no device: doa.planar_steering_table, argument validation
in create, the GRC descriptors.  The figures are printed before they are asserted (run with -s)."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import doa_oracle as oracle
import array_ref as ref
import capon_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(ref.SCENARIOS))
def test_reference_properties(name):
    pos, src, snr_db, K = ref.SCENARIOS[name]
    N, M = pos.shape[0], len(src)
    table = ref.planar_table(pos, ref.P)
    R = ref.covariance(name)
    cond = capon_ref.condition_numbers(R, N, 0.0)
    s_m, q_m, _ = ref.music(R, table, M)
    s_c, q_c, _, st = ref.capon(R, table, 0.0)
    _, loc_m = oracle.find_local_max(s_m, M, ref.P, 0.0, 360.0)
    _, loc_c = oracle.find_local_max(s_c, M, ref.P, 0.0, 360.0)
    e_m, e_c = ref.angle_error(loc_m, src), ref.angle_error(loc_c, src)
    print("%s (N=%d K=%d): min Q / max Q (MUSIC) %.2g, angle error MUSIC %.3f / Capon %.3f deg, cond <= %.3g"
          % (name, N, K, (q_m.min(axis=1) / q_m.max(axis=1)).min(), e_m, e_c, cond.max()))
    assert np.all(st == 0)
    assert cond.max() <= 1e5
    assert e_m <= ref.angle_cap(ref.P) and e_c <= ref.angle_cap(ref.P)


def test_a_linear_array_cannot_tell_an_azimuth_from_its_mirror_image():
    """One source at 70.3 degrees, 20 dB, K = 256, scanned over 0..360: a 5-element ULA gives two peaks, at 70 and 290
    degrees; the 5-element circular array of scenario uca5 gives one."""
    step = 360.0 / ref.P
    for pos, mirrored in ((ref.ula(5, 0.5), True), (ref.uca(5), False)):
        x = ref.make_streams(pos, (70.3,), 20.0, ref.N_ITEMS * 256)
        R = oracle.autocorrelate(x, 256, 0, 0, ref.N_ITEMS)
        spec, _, _ = ref.music(R, ref.planar_table(pos, ref.P), 1)
        val, loc = oracle.find_local_max(spec, 2, ref.P, 0.0, 360.0)
        val, loc = np.asarray(val, np.float64), np.asarray(loc, np.float64)
        print("linear" if mirrored else "circular", "array: two largest peaks of item 0 at", loc[0], "deg,", val[0], "dB")
        if mirrored:
            loc = np.sort(loc, axis=1)
            assert np.all(np.abs(loc[:, 0] - 70.3) <= step) and np.all(np.abs(loc[:, 1] - (360.0 - 70.3)) <= step)
        else:
            _, top = oracle.find_local_max(spec, 1, ref.P, 0.0, 360.0)     # (the two ports are sorted independently)
            assert np.all(np.abs(np.asarray(top, np.float64) - 70.3) <= step)
            assert np.all(np.abs(loc - (360.0 - 70.3)) > 5.0)          # nothing at the mirror image


def test_planar_steering_table_matches_its_formula():
    import doa
    rand11 = ref.SCENARIOS["rand11"][0]
    for pos, kw in ((ref.uca(5), {}), (rand11, {}), (ref.ula(6, 0.45), {}), (ref.uca(5), dict(elevation=60.0)),
                    (rand11, dict(az_min=-30.0, az_max=150.0, elevation=60.0))):
        got = doa.planar_steering_table(pos, 181, **kw)
        want = ref.planar_table(pos, 181, **kw)
        assert got.shape == (181, pos.shape[0]) and got.dtype == np.complex128
        err = float(np.abs(got - want).max())
        print("planar_steering_table N=%d %s: max abs error %.3g" % (pos.shape[0], kw, err))
        assert err <= 1e-14
    # the ULA form is doa.sim.manifold's
    got = doa.planar_steering_table(ref.ula(4, 0.5), 90, 0.0, 180.0)
    assert np.abs(got.T - doa.sim.manifold(0.5, 4, ref.grid(90, 0.0, 180.0))).max() <= 1e-14
    assert np.array_equal(doa.uca_positions(5, 0.425), 0.425 * np.stack(
        [np.cos(2 * np.pi * np.arange(5) / 5), np.sin(2 * np.pi * np.arange(5) / 5)], axis=1))


def test_planar_steering_table_rejects_bad_arguments():
    import doa
    good = ref.uca(4)
    nan_pos = good.copy(); nan_pos[2, 1] = np.nan
    bad = [(good[:1], 8, {}), (np.zeros((17, 2)), 8, {}), (good, 0, {}), (nan_pos, 8, {}),
           (good, 8, dict(az_min=10.0, az_max=10.0)), (good, 8, dict(az_min=10.0, az_max=5.0)),
           (good, 8, dict(elevation=float("inf"))), (good, 8, dict(az_max=float("nan")))]
    for pos, p, kw in bad:
        with pytest.raises(doa.DoaError) as ei:
            doa.planar_steering_table(pos, p, **kw)
        assert ei.value.status == -1, (pos.shape, p, kw)
    with pytest.raises(ValueError):
        doa.planar_steering_table(np.zeros((4, 3)), 8)


def test_create_validates_before_the_device():
    import doa
    from doa import _lib
    t = ref.planar_table(ref.uca(4), 16)
    t_nan = t.copy(); t_nan[3, 1] = np.nan
    t_inf = t.copy(); t_inf[0, 0] = np.inf * 1j
    music_bad = [(1, t[:, :1]), (1, np.ones((16, 17), complex)), (0, t), (4, t), (5, t), (1, t[:0]), (1, t_nan), (1, t_inf)]
    for m, tab in music_bad:
        with pytest.raises(doa.DoaError) as ei:
            doa.MUSIC_array(m, tab)
        assert ei.value.status == -1 and "no HIP device" not in str(ei.value), (m, tab.shape)
    capon_bad = [(t[:, :1], 0.0), (np.ones((16, 17), complex), 0.0), (t[:0], 0.0), (t_nan, 0.0), (t_inf, 0.0), (t, -1.0),
                 (t, float("nan")), (t, float("inf"))]
    for tab, delta in capon_bad:
        with pytest.raises(doa.DoaError) as ei:
            doa.capon_array(tab, delta)
        assert ei.value.status == -1 and "no HIP device" not in str(ei.value), (tab.shape, delta)
    # a NULL table
    assert not _lib.lib.doa_MUSIC_array_create(1, 4, 16, None) and "NULL" in _lib.last_error()
    assert not _lib.lib.doa_capon_array_create(4, 16, None, 0.0) and "NULL" in _lib.last_error()
    with pytest.raises(ValueError):
        doa.MUSIC_array(1, np.ones(16, complex))


DESCRIPTORS = {
    "MUSIC_array": (["num_targets", "positions", "pspectrum_len", "az_min", "az_max", "elevation"],
                    "doa.MUSIC_array($num_targets, doa.planar_steering_table($positions, $pspectrum_len, $az_min, $az_max, $elevation))",
                    ["len($positions) > 1", "len($positions) > $num_targets", "$num_targets > 0", "$az_max > $az_min"]),
    "capon_array": (["positions", "pspectrum_len", "az_min", "az_max", "elevation", "diagonal_loading"],
                    "doa.capon_array(doa.planar_steering_table($positions, $pspectrum_len, $az_min, $az_max, $elevation), $diagonal_loading)",
                    ["len($positions) > 1", "$diagonal_loading >= 0", "$az_max > $az_min"]),
}


@pytest.mark.parametrize("cls", sorted(DESCRIPTORS))
def test_grc_descriptor(cls):
    keys, make, checks = DESCRIPTORS[cls]
    root = ET.parse(os.path.join(ROOT, "gr-doa_amd", "grc", "doa_%s.xml" % cls)).getroot()
    assert root.findtext("key") == "doa_" + cls
    assert root.findtext("import") == "import doa"
    assert [p.findtext("key") for p in root.findall("param")] == keys
    assert root.findtext("make") == make
    assert [c.text for c in root.findall("check")] == checks
    sink, source = root.find("sink"), root.find("source")
    assert sink.findtext("type") == "complex" and sink.findtext("vlen") == "len($positions)*len($positions)"
    assert source.findtext("type") == "float" and source.findtext("vlen") == "$pspectrum_len"
    # the make string and the defaults construct what they say (no device needed up to the table)
    import doa
    defaults = {p.findtext("key"): p.findtext("value") for p in root.findall("param")}
    table = doa.planar_steering_table(eval(defaults["positions"], {"doa": doa}), int(defaults["pspectrum_len"]),
                                      float(defaults["az_min"]), float(defaults["az_max"]), float(defaults["elevation"]))
    assert table.shape == (720, 5)
