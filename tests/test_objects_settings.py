"""CPU: the Dense.Objects.* settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: absent
without Dense.VoxelSize or Dense.Objects.VoxelSize, the defaults, every key read back, each range edge and every value outside its range as a
settings error; without the keys the other Dense.* results are unchanged."""
import ctypes as C

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.system import write_settings

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)
BF, THBG, THOBJ = 387.5744, 40.0, 25.0
NAMES = ["present", "VoxelSize", "nx", "ny", "nz", "Truncation", "MinDepth", "MaxDepth", "MaxWeight", "MaxObjects", "MinPixels", "MinFrames", "MinWeight"]


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_settings_check_dense_objects.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_check_dense.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(13, -7.0)
    return host.host_settings_check_dense_objects(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), dict(zip(NAMES, out))


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, BF, 256.0, THBG, THOBJ)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def test_absent_without_either_voxel_size(host, tmp_path):
    rc, msg, v = _check(host, _with(tmp_path, "plain.yaml", []))
    assert (rc, msg) == (0, "") and v["present"] == 0 and all(x == -7.0 for k, x in v.items() if k != "present")
    rc, msg, v = _check(host, _with(tmp_path, "dense.yaml", ["Dense.VoxelSize: 0.1", "Dense.Objects.MaxObjects: 999", "Dense.Objects.Size: [0, 0]"]))
    assert (rc, msg) == (0, "") and v["present"] == 0                    # without Dense.Objects.VoxelSize the other object keys are not read
    rc, msg, v = _check(host, _with(tmp_path, "objects.yaml", ["Dense.Objects.VoxelSize: 0.05", "Dense.Objects.MaxObjects: 999"]))
    assert (rc, msg) == (0, "") and v["present"] == 0                    # the keys are read only with Dense.VoxelSize
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_defaults_and_every_key(host, tmp_path):
    rc, msg, v = _check(host, _with(tmp_path, "only.yaml", ["Dense.VoxelSize: 0.25", "Dense.Objects.VoxelSize: 0.05"]))
    assert (rc, msg) == (0, "")
    assert v == dict(present=1, VoxelSize=float(np.float32(0.05)), nx=96, ny=64, nz=96, Truncation=float(np.float32(4) * np.float32(0.05)), MinDepth=0, MaxDepth=THOBJ, MaxWeight=64,
                     MaxObjects=16, MinPixels=200, MinFrames=3, MinWeight=2)
    lines = ["Dense.VoxelSize: 0.25", "Dense.MinDepth: 0.5", "Dense.MaxWeight: 200", "Dense.MinWeight: 5", "Dense.Objects.VoxelSize: 0.125", "Dense.Objects.Size: [40, 24, 72]",
             "Dense.Objects.Truncation: 0.75", "Dense.Objects.MaxDepth: 30", "Dense.Objects.MaxObjects: 64", "Dense.Objects.MinPixels: 1", "Dense.Objects.MinFrames: 1"]
    rc, msg, v = _check(host, _with(tmp_path, "keyed.yaml", lines))
    assert (rc, msg) == (0, "")
    assert v == dict(present=1, VoxelSize=0.125, nx=40, ny=24, nz=72, Truncation=0.75, MinDepth=0.5, MaxDepth=30, MaxWeight=200, MaxObjects=64, MinPixels=1, MinFrames=1, MinWeight=5)
    # each range edge that is still in order
    for line in ("Dense.Objects.MaxObjects: 1", "Dense.Objects.MinWeight: 1", "Dense.Objects.MinWeight: 255", "Dense.Objects.Size: [1, 1, 1]", "Dense.Objects.Size: [4096, 4096, 128]",
                 "Dense.Objects.MaxDepth: 0.001"):
        rc, msg, v = _check(host, _with(tmp_path, "edge.yaml", ["Dense.VoxelSize: 0.25", "Dense.Objects.VoxelSize: 0.05", line]))
        assert (rc, msg) == (0, "") and v["present"] == 1, line


def test_without_the_keys_the_other_dense_results_are_unchanged(host, tmp_path):
    lines = ["Dense.VoxelSize: 0.25", "Dense.Size: [96, 32, 160]", "Dense.MaxWeight: 32"]
    obj = ["Dense.Objects.VoxelSize: 0.05", "Dense.Objects.Size: [8, 8, 8]", "Dense.Objects.MinWeight: 9", "Dense.Objects.MaxDepth: 7"]
    a, b = np.full(14, -7.0), np.full(14, -7.0)
    msg = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(_with(tmp_path, "a.yaml", lines)).encode(), msg, 256, a.ctypes.data) == 0
    assert host.host_settings_check_dense(str(_with(tmp_path, "b.yaml", lines + obj)).encode(), msg, 256, b.ctypes.data) == 0
    assert np.array_equal(a, b) and a[0] == 1


BAD = [("VoxelSize", "0"), ("VoxelSize", "-0.1"), ("VoxelSize", "nan"), ("VoxelSize", "inf"), ("VoxelSize", "1e-60"), ("Size", "[0, 8, 8]"), ("Size", "[8, 8]"), ("Size", "[8, 4097, 8]"),
       ("Size", "[8.5, 8, 8]"), ("Size", "[2048, 2048, 1024]"), ("Size", "64"), ("Truncation", "0"), ("Truncation", "-1"), ("Truncation", "nan"), ("MaxDepth", "0"), ("MaxDepth", "inf"),
       ("MaxObjects", "0"), ("MaxObjects", "65"), ("MaxObjects", "2.5"), ("MinPixels", "0"), ("MinPixels", "1.5"), ("MinFrames", "0"), ("MinFrames", "0.5"), ("MinWeight", "0"),
       ("MinWeight", "256"), ("MinWeight", "1.5")]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_are_settings_errors(host, tmp_path, key, value):
    lines = ["Dense.VoxelSize: 0.1"] + ([] if key == "VoxelSize" else ["Dense.Objects.VoxelSize: 0.05"]) + [f"Dense.Objects.{key}: {value}"]
    path = _with(tmp_path, "bad.yaml", lines)
    rc, msg, v = _check(host, path)
    assert rc == 1 and msg.startswith("settings: ") and f"Dense.Objects.{key}" in msg, msg
    assert all(x == -7.0 for x in v.values())                     # nothing is reported beside an error
    out = np.full(14, -7.0)
    buf = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(path).encode(), buf, 256, out.ctypes.data) == 1       # the same error wherever the Dense.* keys are read


def test_max_depth_at_or_below_the_dense_min_depth(host, tmp_path):
    rc, msg, _ = _check(host, _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.MinDepth: 26", "Dense.Objects.VoxelSize: 0.05"]))
    assert rc == 1 and "Dense.Objects.MaxDepth" in msg


def test_a_bad_value_ends_a_cpp_callers_process(tmp_path):
    """System(settings, sensor) as a C++ caller gets it: a Dense.Objects.* settings error exits with -1 and its message before any device is touched.
    In a child process, since it ends the process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.Objects.VoxelSize: 0.05", "Dense.Objects.MaxObjects: 65"])
    code = ("import ctypes, sys; from vdo_slam_amd import _capi as K; L = K.load_host_lib(); L.host_system_create_unchecked.restype = ctypes.c_void_p; "
            "L.host_system_create_unchecked.argtypes = [ctypes.c_char_p, ctypes.c_int]; L.host_system_create_unchecked(sys.argv[1].encode(), 0); print('survived')")
    r = subprocess.run([sys.executable, "-c", code, str(bad)], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Dense.Objects.MaxObjects outside 1..64" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr)
