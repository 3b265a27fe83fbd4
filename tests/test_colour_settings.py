"""CPU: the Dense.Colour* settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: read only
with Dense.VoxelSize; Dense.Colour 0 by default, 0 or 1; Dense.Colour.Band Dense.Truncation / 2 by default, positive and at most Dense.Truncation;
Dense.Colour.MaxWeight Dense.MaxWeight by default, Dense.Colour.MinWeight 1 by default, both 1..255.  Any other value is a settings error - which
ends a C++ caller's process with every sensor."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.system import write_settings

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    for name in ("host_settings_check_dense_colour", "host_settings_check_dense", "host_settings_check_dense_mesh"):
        getattr(L, name).argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(5, -7.0)
    return host.host_settings_check_dense_colour(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), tuple(out)


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, 387.5744, 256.0, 40.0, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


NONE = (0, -7.0, -7.0, -7.0, -7.0)


def test_read_only_with_the_voxel_size(host, tmp_path):
    assert _check(host, _with(tmp_path, "plain.yaml", [])) == (0, "", NONE)
    assert _check(host, _with(tmp_path, "alone.yaml", ["Dense.Colour: 1", "Dense.Colour.Band: 0.1"])) == (0, "", NONE)
    assert _check(host, _with(tmp_path, "alone_bad.yaml", ["Dense.Colour: 7", "Dense.Colour.Band: -1", "Dense.Colour.MaxWeight: 0", "Dense.Colour.MinWeight: 999"])) == (0, "", NONE)
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_defaults_and_values(host, tmp_path):
    f = lambda v: float(np.float32(v))
    assert _check(host, _with(tmp_path, "default.yaml", ["Dense.VoxelSize: 0.1"])) == (0, "", (1, 0, f(np.float32(0.4) / np.float32(2)), 64, 1))
    assert _check(host, _with(tmp_path, "off.yaml", ["Dense.VoxelSize: 0.1", "Dense.Colour: 0"]))[2][:2] == (1, 0)
    on = _with(tmp_path, "on.yaml", ["Dense.VoxelSize: 0.1", "Dense.Colour: 1"])
    assert _check(host, on) == (0, "", (1, 1, f(np.float32(0.4) / np.float32(2)), 64, 1))
    # the defaults follow Dense.Truncation and Dense.MaxWeight
    assert _check(host, _with(tmp_path, "follow.yaml", ["Dense.VoxelSize: 0.1", "Dense.Truncation: 0.3", "Dense.MaxWeight: 20", "Dense.Colour: 1"])) == \
        (0, "", (1, 1, f(np.float32(0.3) / np.float32(2)), 20, 1))
    given = _with(tmp_path, "given.yaml", ["Dense.VoxelSize: 0.1", "Dense.Colour: 1", "Dense.Colour.Band: 0.4", "Dense.Colour.MaxWeight: 255", "Dense.Colour.MinWeight: 3"])
    assert _check(host, given) == (0, "", (1, 1, f(0.4), 255, 3))                 # Band == Truncation is in range
    assert _check(host, _with(tmp_path, "low.yaml", ["Dense.VoxelSize: 0.1", "Dense.Colour.MaxWeight: 1", "Dense.Colour.MinWeight: 255"]))[2][3:] == (1, 255)
    # the keys change none of the other Dense.* values
    a, b = np.full(14, -7.0), np.full(14, -7.0)
    msg = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(given).encode(), msg, 256, a.ctypes.data) == 0
    assert host.host_settings_check_dense(str(_with(tmp_path, "default2.yaml", ["Dense.VoxelSize: 0.1"])).encode(), msg, 256, b.ctypes.data) == 0
    assert np.array_equal(a, b) and a[0] == 1
    m = np.full(2, -7.0)
    assert host.host_settings_check_dense_mesh(str(given).encode(), msg, 256, m.ctypes.data) == 0 and tuple(m) == (1, 0)


BAD = [("Dense.Colour", v, "Dense.Colour must be 0 or 1") for v in ("2", "-1", "0.5", "nan", "inf", "1e12", "[1]")] + \
      [("Dense.Colour.Band", v, "Dense.Colour.Band must be positive") for v in ("0", "-0.1", "nan", "inf", "1e-60", "[0.1]")] + \
      [("Dense.Colour.Band", v, "Dense.Colour.Band must not exceed Dense.Truncation") for v in ("0.41", "100")] + \
      [("Dense.Colour.MaxWeight", v, "Dense.Colour.MaxWeight must be a whole number") for v in ("1.5", "nan", "[3]")] + \
      [("Dense.Colour.MaxWeight", v, "Dense.Colour.MaxWeight outside 1..255") for v in ("0", "256", "-3")] + \
      [("Dense.Colour.MinWeight", v, "Dense.Colour.MinWeight must be a whole number") for v in ("2.5", "inf", "[1]")] + \
      [("Dense.Colour.MinWeight", v, "Dense.Colour.MinWeight outside 1..255") for v in ("0", "256", "-1")]


@pytest.mark.parametrize("key,value,text", BAD, ids=[f"{k}={v}" for k, v, _ in BAD])
def test_bad_values_are_settings_errors(host, tmp_path, key, value, text):
    """with and without Dense.Colour: 1 - the keys are checked whenever Dense.VoxelSize is there"""
    for extra in ([], ["Dense.Colour: 1"] if key != "Dense.Colour" else []):
        rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1"] + extra + [f"{key}: {value}"]))
        assert rc == 1 and msg == "settings: " + text, msg
        assert v == (-7.0,) * 5                                   # nothing is reported beside an error
    # the error is the same through the probe of the other Dense.* keys
    msg = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(_with(tmp_path, "bad2.yaml", ["Dense.VoxelSize: 0.1", f"{key}: {value}"])).encode(), msg, 256, None) == 1
    assert msg.value.decode() == "settings: " + text


@pytest.mark.parametrize("sensor", [0, 1, 2])
def test_a_bad_value_ends_the_process_with_every_sensor(tmp_path, sensor):
    """System(settings, sensor) as a C++ caller gets it: the settings error exits with -1 and its message before any device is touched.  In a child
    process, since it ends the process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.Colour: 1", "Dense.Colour.Band: 0.5"])
    code = ("import ctypes, sys; from vdo_slam_amd import _capi as K; L = K.load_host_lib(); L.host_system_create_unchecked.restype = ctypes.c_void_p; "
            "L.host_system_create_unchecked.argtypes = [ctypes.c_char_p, ctypes.c_int]; L.host_system_create_unchecked(sys.argv[1].encode(), int(sys.argv[2])); print('survived')")
    r = subprocess.run([sys.executable, "-c", code, str(bad), str(sensor)], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Dense.Colour.Band must not exceed Dense.Truncation" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr)
