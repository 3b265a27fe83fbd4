"""CPU: the Dense.Align.* settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: read only with
Dense.VoxelSize, absent keys mean off, their defaults, every range edge, and every bad value as a settings error."""
import ctypes as C

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.system import write_settings

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)
BF, THBG = 387.5744, 40.0
W, H = 1242, 375
NAMES = ["present", "Iterations", "MaxDist", "Subsample", "MinPixels", "Apply"]


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_settings_check_dense_align.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_check_dense.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_check_dense_view.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(6, -7.0)
    return host.host_settings_check_dense_align(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), dict(zip(NAMES, out))


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", W, H, KITTI_K, BF, 256.0, THBG, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def _grid16(s):
    return (-(-W // s)) * (-(-H // s)) // 16


def test_not_read_without_the_voxel_size(host, tmp_path):
    rc, msg, v = _check(host, _with(tmp_path, "plain.yaml", []))
    assert (rc, msg) == (0, "") and v["present"] == 0 and all(x == -7.0 for k, x in v.items() if k != "present")
    rc, msg, v = _check(host, _with(tmp_path, "others.yaml", ["Dense.Align.Iterations: -1", "Dense.Align.MaxDist: nan", "Dense.Align.Subsample: 99", "Dense.Align.Apply: 7"]))
    assert (rc, msg) == (0, "") and v["present"] == 0
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_absent_keys_mean_off_and_the_defaults(host, tmp_path):
    f32 = lambda v: float(np.float32(v))
    # off; MaxDist Truncation (4 x voxel); Subsample 1; MinPixels a sixteenth of the sample grid; Apply 0
    rc, msg, v = _check(host, _with(tmp_path, "only.yaml", ["Dense.VoxelSize: 0.05"]))
    assert (rc, msg) == (0, "") and v == dict(present=1, Iterations=0, MaxDist=float(np.float32(4) * np.float32(0.05)), Subsample=1, MinPixels=_grid16(1), Apply=0)
    rc, msg, v = _check(host, _with(tmp_path, "zero.yaml", ["Dense.VoxelSize: 0.05", "Dense.Align.Iterations: 0", "Dense.Align.Apply: 1"]))
    assert (rc, msg) == (0, "") and v["Iterations"] == 0 and v["Apply"] == 1
    rc, msg, v = _check(host, _with(tmp_path, "trunc.yaml", ["Dense.VoxelSize: 0.25", "Dense.Truncation: 0.75", "Dense.Align.Iterations: 5", "Dense.Align.Subsample: 4"]))
    assert (rc, msg) == (0, "") and v == dict(present=1, Iterations=5, MaxDist=0.75, Subsample=4, MinPixels=_grid16(4), Apply=0)
    rc, msg, v = _check(host, _with(tmp_path, "keyed.yaml", ["Dense.VoxelSize: 0.25", "Dense.Align.Iterations: 7", "Dense.Align.MaxDist: 0.3", "Dense.Align.Subsample: 3",
                                                              "Dense.Align.MinPixels: 1234", "Dense.Align.Apply: 1"]))
    assert (rc, msg) == (0, "") and v == dict(present=1, Iterations=7, MaxDist=f32(0.3), Subsample=3, MinPixels=1234, Apply=1)
    # the alignment keys change none of the mapper's or the view's own values
    for hook, n in ((host.host_settings_check_dense, 14), (host.host_settings_check_dense_view, 5)):
        a, b = np.full(n, -7.0), np.full(n, -7.0)
        m = C.create_string_buffer(256)
        assert hook(str(_with(tmp_path, "a.yaml", ["Dense.VoxelSize: 0.25"])).encode(), m, 256, a.ctypes.data) == 0
        assert hook(str(tmp_path / "keyed.yaml").encode(), m, 256, b.ctypes.data) == 0
        assert np.array_equal(a, b)


@pytest.mark.parametrize("key,value", [("Iterations", "1"), ("Iterations", "64"), ("Subsample", "1"), ("Subsample", "8"), ("MinPixels", "6"), ("MinPixels", "1000000000"), ("Apply", "0"),
                                       ("Apply", "1"), ("MaxDist", "1e-30"), ("MaxDist", "3e38")])
def test_every_range_edge_is_taken(host, tmp_path, key, value):
    rc, msg, v = _check(host, _with(tmp_path, "edge.yaml", ["Dense.VoxelSize: 0.1", f"Dense.Align.{key}: {value}"]))
    assert (rc, msg) == (0, "") and v[key] == (float(np.float32(float(value))) if key == "MaxDist" else float(value))


BAD = [("Iterations", "-1"), ("Iterations", "65"), ("Iterations", "2.5"), ("Iterations", "nan"), ("MaxDist", "0"), ("MaxDist", "-0.1"), ("MaxDist", "nan"), ("MaxDist", "inf"),
       ("MaxDist", "1e-60"), ("MaxDist", "1e39"), ("Subsample", "0"), ("Subsample", "9"), ("Subsample", "1.5"), ("Subsample", "nan"), ("MinPixels", "5"), ("MinPixels", "0"),
       ("MinPixels", "-3"), ("MinPixels", "6.5"), ("MinPixels", "inf"), ("Apply", "2"), ("Apply", "-1"), ("Apply", "0.5"), ("Apply", "nan")]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_are_settings_errors(host, tmp_path, key, value):
    """Iterations outside 0..64 or not whole; MaxDist not positive, not finite or not a positive float; Subsample outside 1..8; MinPixels below 6; Apply not 0 or 1"""
    rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", f"Dense.Align.{key}: {value}"]))
    assert rc == 1 and msg.startswith("settings: ") and f"Dense.Align.{key}" in msg, msg
    assert all(x == -7.0 for x in v.values())
    m = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(tmp_path / "bad.yaml").encode(), m, 256, None) == 1 and f"Dense.Align.{key}" in m.value.decode()      # the same error wherever the keys are read
