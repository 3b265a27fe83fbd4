"""CPU: the Dense.View.* settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: read only with
Dense.VoxelSize, their defaults, every key read back, and every bad value as a settings error."""
import ctypes as C

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.system import write_settings

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)
BF, THBG = 387.5744, 40.0
NAMES = ["present", "Near", "Step", "MinWeight", "n_steps"]


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_settings_check_dense_view.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_check_dense.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(5, -7.0)
    return host.host_settings_check_dense_view(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), dict(zip(NAMES, out))


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, BF, 256.0, THBG, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def test_not_read_without_the_voxel_size(host, tmp_path):
    rc, msg, v = _check(host, _with(tmp_path, "plain.yaml", []))
    assert (rc, msg) == (0, "") and v["present"] == 0 and all(x == -7.0 for k, x in v.items() if k != "present")
    rc, msg, v = _check(host, _with(tmp_path, "others.yaml", ["Dense.View.Step: -1", "Dense.View.Near: nan", "Dense.View.MinWeight: 999"]))
    assert (rc, msg) == (0, "") and v["present"] == 0
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_defaults_and_every_key(host, tmp_path):
    f32 = lambda v: float(np.float32(v))
    # Near max(MinDepth, VoxelSize); Step Truncation / 2 with Truncation 4 x voxel; MinWeight Dense.MinWeight; n_steps ceil((MaxDepth - Near) / Step) + 1
    rc, msg, v = _check(host, _with(tmp_path, "only.yaml", ["Dense.VoxelSize: 0.05"]))
    near, step = f32(0.05), float(np.float32(4) * np.float32(0.05) / np.float32(2))
    assert (rc, msg) == (0, "") and v == dict(present=1, Near=near, Step=step, MinWeight=2, n_steps=int(np.ceil((THBG - near) / step)) + 1)
    rc, msg, v = _check(host, _with(tmp_path, "dense.yaml", ["Dense.VoxelSize: 0.25", "Dense.MinDepth: 0.5", "Dense.Truncation: 0.75", "Dense.MaxDepth: 30", "Dense.MinWeight: 5"]))
    assert (rc, msg) == (0, "") and v == dict(present=1, Near=0.5, Step=0.375, MinWeight=5, n_steps=int(np.ceil(29.5 / 0.375)) + 1)
    rc, msg, v = _check(host, _with(tmp_path, "keyed.yaml", ["Dense.VoxelSize: 0.25", "Dense.MaxDepth: 30", "Dense.View.Near: 0", "Dense.View.Step: 0.125", "Dense.View.MinWeight: 255"]))
    assert (rc, msg) == (0, "") and v == dict(present=1, Near=0, Step=0.125, MinWeight=255, n_steps=241)
    # 65536 samples are the most: (32 - 2^-11) / 2^-11 = 65535 intervals, all exact in fp32; one more is an error
    rc, msg, v = _check(host, _with(tmp_path, "most.yaml", ["Dense.VoxelSize: 0.25", "Dense.MaxDepth: 31.99951171875", "Dense.View.Near: 0", "Dense.View.Step: 0.00048828125"]))
    assert (rc, msg) == (0, "") and v["n_steps"] == 65536
    rc, msg, v = _check(host, _with(tmp_path, "more.yaml", ["Dense.VoxelSize: 0.25", "Dense.MaxDepth: 32", "Dense.View.Near: 0", "Dense.View.Step: 0.00048828125"]))
    assert rc == 1 and "Dense.View.Step" in msg
    # the view keys change none of the mapper's own values
    a, b = np.full(14, -7.0), np.full(14, -7.0)
    m = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(_with(tmp_path, "a.yaml", ["Dense.VoxelSize: 0.25"])).encode(), m, 256, a.ctypes.data) == 0
    assert host.host_settings_check_dense(str(_with(tmp_path, "b.yaml", ["Dense.VoxelSize: 0.25", "Dense.View.Near: 3", "Dense.View.Step: 0.3", "Dense.View.MinWeight: 9"])).encode(), m, 256,
                                          b.ctypes.data) == 0
    assert np.array_equal(a, b)


BAD = [("Near", "-0.5"), ("Near", "nan"), ("Near", "inf"), ("Near", "40"), ("Near", "41.5"), ("Step", "0"), ("Step", "-0.2"), ("Step", "nan"), ("Step", "inf"), ("Step", "1e-60"),
       ("Step", "0.0005"), ("MinWeight", "0"), ("MinWeight", "256"), ("MinWeight", "1.5"), ("MinWeight", "nan")]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_are_settings_errors(host, tmp_path, key, value):
    """Near < 0, not finite or >= Dense.MaxDepth (40, ThDepthBG); Step <= 0, not finite, or so small that a ray has more than 65536 samples (0.0005: 80 000);
    MinWeight outside 1..255 or not whole"""
    rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", f"Dense.View.{key}: {value}"]))
    assert rc == 1 and msg.startswith("settings: ") and f"Dense.View.{key}" in msg, msg
    assert all(x == -7.0 for x in v.values())
    m = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(tmp_path / "bad.yaml").encode(), m, 256, None) == 1 and f"Dense.View.{key}" in m.value.decode()      # the same error wherever the keys are read
