"""CPU: the Dense.Distance settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: read only
with Dense.VoxelSize; Dense.Distance 0 by default, 0 or 1; Dense.Distance.Radius 2.0 metres, positive, finite and 1..8191 voxels of Dense.VoxelSize;
Dense.Distance.MinWeight Dense.MinWeight by default, 1..255 - and any other value a settings error, which ends a C++ caller's process with every sensor."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.system import write_settings

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)
NONE = (-7.0,) * 5


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_settings_check_dense_distance.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_check_dense.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(5, -7.0)
    return host.host_settings_check_dense_distance(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), tuple(float(v) for v in out)


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, 387.5744, 256.0, 40.0, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def test_read_only_with_the_voxel_size(host, tmp_path):
    nothing = (0.0,) + NONE[1:]
    assert _check(host, _with(tmp_path, "plain.yaml", [])) == (0, "", nothing)
    assert _check(host, _with(tmp_path, "alone.yaml", ["Dense.Distance: 1", "Dense.Distance.Radius: 1.0"])) == (0, "", nothing)
    assert _check(host, _with(tmp_path, "alone_bad.yaml", ["Dense.Distance: 7", "Dense.Distance.Radius: -1", "Dense.Distance.MinWeight: 0"])) == (0, "", nothing)   # not even read
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_defaults_and_values(host, tmp_path):
    v = ["Dense.VoxelSize: 0.1"]
    assert _check(host, _with(tmp_path, "default.yaml", v)) == (0, "", (1, 0, 2.0, 20, 2))                      # Radius 2.0 m = 20 voxels, MinWeight Dense.MinWeight = 2
    assert _check(host, _with(tmp_path, "off.yaml", v + ["Dense.Distance: 0"])) == (0, "", (1, 0, 2.0, 20, 2))
    on = _with(tmp_path, "on.yaml", v + ["Dense.Distance: 1"])
    assert _check(host, on) == (0, "", (1, 1, 2.0, 20, 2))
    assert _check(host, _with(tmp_path, "mw.yaml", v + ["Dense.Distance: 1", "Dense.MinWeight: 5"])) == (0, "", (1, 1, 2.0, 20, 5))      # follows Dense.MinWeight
    assert _check(host, _with(tmp_path, "own.yaml", v + ["Dense.Distance: 1", "Dense.MinWeight: 5", "Dense.Distance.MinWeight: 1", "Dense.Distance.Radius: 0.75"])) == \
        (0, "", (1, 1, 0.75, 8, 1))                                                                              # ceil(0.75 / 0.1) = 8
    # the keys change none of the other Dense.* values
    a, b = np.full(14, -7.0), np.full(14, -7.0)
    msg = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(on).encode(), msg, 256, a.ctypes.data) == 0
    assert host.host_settings_check_dense(str(_with(tmp_path, "default2.yaml", v)).encode(), msg, 256, b.ctypes.data) == 0
    assert np.array_equal(a, b) and a[0] == 1


def test_range_edges(host, tmp_path):
    v = ["Dense.VoxelSize: 0.5", "Dense.Distance: 1"]
    for lines, want in ((["Dense.Distance.Radius: 0.0001"], (1, 1, np.float32(0.0001), 1, 2)),                 # a fraction of a voxel is one voxel
                        (["Dense.Distance.Radius: 0.5"], (1, 1, 0.5, 1, 2)),
                        (["Dense.Distance.Radius: 4095.5"], (1, 1, 4095.5, 8191, 2)),                             # the largest radius
                        (["Dense.Distance.MinWeight: 1"], (1, 1, 2.0, 4, 1)),
                        (["Dense.Distance.MinWeight: 255"], (1, 1, 2.0, 4, 255))):
        assert _check(host, _with(tmp_path, "edge.yaml", v + lines)) == (0, "", tuple(float(x) for x in want)), lines
    rc, msg, out = _check(host, _with(tmp_path, "over.yaml", v + ["Dense.Distance.Radius: 4095.75"]))             # 8192 voxels
    assert rc == 1 and "Dense.Distance.Radius" in msg and "8191" in msg and out == NONE
    # the default radius against a voxel it is 8191 voxels too long for: an error only where the field is asked for
    tiny = ["Dense.VoxelSize: 0.000244140625", "Dense.Size: [8, 8, 8]", "Dense.MaxDepth: 0.02"]                  # 2^-12 m: 2.0 m are 8192 voxels
    assert _check(host, _with(tmp_path, "tiny_off.yaml", tiny))[0] == 0
    rc, msg, out = _check(host, _with(tmp_path, "tiny_on.yaml", tiny + ["Dense.Distance: 1"]))
    assert rc == 1 and "Dense.Distance.Radius" in msg
    assert _check(host, _with(tmp_path, "tiny_fit.yaml", tiny + ["Dense.Distance: 1", "Dense.Distance.Radius: 1.5"]))[2][3] == 6144


@pytest.mark.parametrize("key,value", [("Dense.Distance", "2"), ("Dense.Distance", "-1"), ("Dense.Distance", "0.5"), ("Dense.Distance", "nan"), ("Dense.Distance", "[1]"),
                                       ("Dense.Distance.Radius", "0"), ("Dense.Distance.Radius", "-2"), ("Dense.Distance.Radius", "nan"), ("Dense.Distance.Radius", "inf"),
                                       ("Dense.Distance.Radius", "1e39"), ("Dense.Distance.Radius", "[2.0]"), ("Dense.Distance.Radius", "900"),
                                       ("Dense.Distance.MinWeight", "0"), ("Dense.Distance.MinWeight", "256"), ("Dense.Distance.MinWeight", "1.5"),
                                       ("Dense.Distance.MinWeight", "nan"), ("Dense.Distance.MinWeight", "[2]")])
def test_bad_values_are_settings_errors(host, tmp_path, key, value):
    """also with Dense.Distance: 0 - a bad value of a key that is present is an error whether the field is on or not"""
    for on in ("1", "0"):
        lines = ["Dense.VoxelSize: 0.1"] + ([f"Dense.Distance: {on}"] if key != "Dense.Distance" else []) + [f"{key}: {value}"]
        rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", lines))
        assert rc == 1 and msg.startswith("settings: ") and key in msg, (on, msg)
        assert v == NONE                                          # nothing is reported beside an error


@pytest.mark.parametrize("sensor", [0, 1, 2])
def test_a_bad_value_ends_the_process_with_every_sensor(tmp_path, sensor):
    """System(settings, sensor) as a C++ caller gets it: the settings error exits with -1 and its message before any device is touched.  In a child
    process, since it ends the process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.Distance: 2"])
    code = ("import ctypes, sys; from vdo_slam_amd import _capi as K; L = K.load_host_lib(); L.host_system_create_unchecked.restype = ctypes.c_void_p; "
            "L.host_system_create_unchecked.argtypes = [ctypes.c_char_p, ctypes.c_int]; L.host_system_create_unchecked(sys.argv[1].encode(), int(sys.argv[2])); print('survived')")
    r = subprocess.run([sys.executable, "-c", code, str(bad), str(sensor)], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Dense.Distance must be 0 or 1" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr)
