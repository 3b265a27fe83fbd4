"""CPU: the Dense.* settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: absent without
Dense.VoxelSize, the defaults, every key read back, and every value outside its range as a settings error - which ends a C++ caller's process,
like the reference's, with either sensor."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.system import write_settings

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)
BF, THBG = 387.5744, 40.0
NAMES = ["present", "VoxelSize", "nx", "ny", "nz", "Truncation", "MinDepth", "MaxDepth", "MaxWeight", "MinWeight", "ax", "ay", "az", "RecenterMargin"]


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_settings_check_dense.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_read.argtypes = [C.c_char_p, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(14, -7.0)
    return host.host_settings_check_dense(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), dict(zip(NAMES, out))


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, BF, 256.0, THBG, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def test_absent_without_the_voxel_size(host, tmp_path):
    plain = _with(tmp_path, "plain.yaml", [])
    rc, msg, v = _check(host, plain)
    assert (rc, msg) == (0, "") and v["present"] == 0 and all(x == -7.0 for k, x in v.items() if k != "present")
    # the other keys alone make no mapper and are not even read: a bad value among them is no error
    others = _with(tmp_path, "others.yaml", ["Dense.Size: [8, 8, 8]", "Dense.MaxWeight: 999", "Dense.Anchor: [2, 2, 2]"])
    rc, msg, v = _check(host, others)
    assert (rc, msg) == (0, "") and v["present"] == 0
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_defaults_and_every_key(host, tmp_path):
    only = _with(tmp_path, "only.yaml", ["Dense.VoxelSize: 0.05"])
    rc, msg, v = _check(host, only)
    assert (rc, msg) == (0, "")
    vox = float(np.float32(0.05))
    want = dict(present=1, VoxelSize=vox, nx=256, ny=128, nz=256, Truncation=float(np.float32(4) * np.float32(0.05)), MinDepth=0, MaxDepth=THBG, MaxWeight=64, MinWeight=2, ax=0.5,
                ay=0.5, az=0.25, RecenterMargin=16)
    assert v == want
    lines = ["Dense.VoxelSize: 0.25", "Dense.Size: [96, 32, 160]", "Dense.Truncation: 0.75", "Dense.MinDepth: 0.5", "Dense.MaxDepth: 30", "Dense.MaxWeight: 255", "Dense.MinWeight: 1",
             "Dense.Anchor: [0.25, 0.75, 0.125]", "Dense.RecenterMargin: 0"]
    keyed = _with(tmp_path, "keyed.yaml", lines)
    rc, msg, v = _check(host, keyed)
    assert (rc, msg) == (0, "")
    assert v == dict(present=1, VoxelSize=0.25, nx=96, ny=32, nz=160, Truncation=0.75, MinDepth=0.5, MaxDepth=30, MaxWeight=255, MinWeight=1, ax=0.25, ay=0.75, az=0.125, RecenterMargin=0)
    sized = _with(tmp_path, "sized.yaml", ["Dense.VoxelSize: 0.1", "Dense.Size: [40, 24, 80]"])
    assert _check(host, sized)[2]["RecenterMargin"] == 3                       # min(n) / 8
    plain = _with(tmp_path, "plain.yaml", [])
    a, b = np.zeros(31), np.zeros(31)                             # the Dense.* lines change none of the 31 flat values
    assert host.host_settings_read(str(plain).encode(), a.ctypes.data) == 0 and host.host_settings_read(str(keyed).encode(), b.ctypes.data) == 0
    assert np.array_equal(a, b)


BAD = [("VoxelSize", "0"), ("VoxelSize", "-0.1"), ("VoxelSize", "nan"), ("VoxelSize", "inf"), ("VoxelSize", "1e-60"), ("Size", "[0, 8, 8]"), ("Size", "[8, 8]"), ("Size", "[8, 8, 8, 8]"),
       ("Size", "[8, 4097, 8]"), ("Size", "[8.5, 8, 8]"), ("Size", "[2048, 2048, 1024]"), ("Size", "64"), ("Size", "[8, 8, 8"), ("Truncation", "0"), ("Truncation", "-1"), ("Truncation", "nan"),
       ("MinDepth", "-0.5"), ("MaxDepth", "0"), ("MaxDepth", "inf"), ("MaxWeight", "0"), ("MaxWeight", "256"), ("MaxWeight", "2.5"), ("MinWeight", "0"), ("MinWeight", "256"),
       ("MinWeight", "1.5"), ("Anchor", "[0, 0.5, 0.5]"), ("Anchor", "[0.5, 1, 0.5]"), ("Anchor", "[0.5, 0.5]"), ("Anchor", "0.5"), ("Anchor", "[0.5, nan, 0.5]"),
       ("RecenterMargin", "-1"), ("RecenterMargin", "1.5"), ("RecenterMargin", "1e12")]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_are_settings_errors(host, tmp_path, key, value):
    lines = ([] if key == "VoxelSize" else ["Dense.VoxelSize: 0.1"]) + [f"Dense.{key}: {value}"]
    rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", lines))
    assert rc == 1 and msg.startswith("settings: ") and f"Dense.{key}" in msg, msg
    assert all(x == -7.0 for x in v.values())                     # nothing is reported beside an error


def test_min_depth_at_or_above_max_depth(host, tmp_path):
    rc, msg, _ = _check(host, _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.MinDepth: 40"]))
    assert rc == 1 and "Dense.MaxDepth" in msg


@pytest.mark.parametrize("sensor", [0, 1])
def test_a_bad_value_ends_the_process_with_either_sensor(tmp_path, sensor):
    """System(settings, sensor) as a C++ caller gets it: a Dense.* settings error exits with -1 and its message before any device is touched.  In a
    child process, since it ends the process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.MaxWeight: 300"])
    code = ("import ctypes, sys; from vdo_slam_amd import _capi as K; L = K.load_host_lib(); L.host_system_create_unchecked.restype = ctypes.c_void_p; "
            "L.host_system_create_unchecked.argtypes = [ctypes.c_char_p, ctypes.c_int]; L.host_system_create_unchecked(sys.argv[1].encode(), int(sys.argv[2])); print('survived')")
    r = subprocess.run([sys.executable, "-c", code, str(bad), str(sensor)], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Dense.MaxWeight outside 1..255" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr)
