"""CPU: the Dense.Mesh settings key (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: read only with
Dense.VoxelSize, 0 by default, 0 or 1, and any other value a settings error - which ends a C++ caller's process with every sensor."""
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
    L.host_settings_check_dense_mesh.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_check_dense.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(2, -7.0)
    return host.host_settings_check_dense_mesh(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), (out[0], out[1])


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, 387.5744, 256.0, 40.0, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def test_read_only_with_the_voxel_size(host, tmp_path):
    assert _check(host, _with(tmp_path, "plain.yaml", [])) == (0, "", (0, -7.0))
    assert _check(host, _with(tmp_path, "alone.yaml", ["Dense.Mesh: 1"])) == (0, "", (0, -7.0))
    assert _check(host, _with(tmp_path, "alone_bad.yaml", ["Dense.Mesh: 7"])) == (0, "", (0, -7.0))        # not even read: no error
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


def test_default_and_both_values(host, tmp_path):
    assert _check(host, _with(tmp_path, "default.yaml", ["Dense.VoxelSize: 0.1"])) == (0, "", (1, 0))
    assert _check(host, _with(tmp_path, "off.yaml", ["Dense.VoxelSize: 0.1", "Dense.Mesh: 0"])) == (0, "", (1, 0))
    on = _with(tmp_path, "on.yaml", ["Dense.VoxelSize: 0.1", "Dense.Mesh: 1"])
    assert _check(host, on) == (0, "", (1, 1))
    # the key changes none of the other Dense.* values
    a, b = np.full(14, -7.0), np.full(14, -7.0)
    msg = C.create_string_buffer(256)
    assert host.host_settings_check_dense(str(on).encode(), msg, 256, a.ctypes.data) == 0
    assert host.host_settings_check_dense(str(_with(tmp_path, "default2.yaml", ["Dense.VoxelSize: 0.1"])).encode(), msg, 256, b.ctypes.data) == 0
    assert np.array_equal(a, b) and a[0] == 1


@pytest.mark.parametrize("value", ["2", "-1", "0.5", "nan", "inf", "1e12", "[1]"])
def test_bad_values_are_settings_errors(host, tmp_path, value):
    rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", f"Dense.Mesh: {value}"]))
    assert rc == 1 and msg.startswith("settings: ") and "Dense.Mesh" in msg, msg
    assert v == (-7.0, -7.0)                                      # nothing is reported beside an error


@pytest.mark.parametrize("sensor", [0, 1, 2])
def test_a_bad_value_ends_the_process_with_every_sensor(tmp_path, sensor):
    """System(settings, sensor) as a C++ caller gets it: the settings error exits with -1 and its message before any device is touched.  In a child
    process, since it ends the process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = _with(tmp_path, "bad.yaml", ["Dense.VoxelSize: 0.1", "Dense.Mesh: 2"])
    code = ("import ctypes, sys; from vdo_slam_amd import _capi as K; L = K.load_host_lib(); L.host_system_create_unchecked.restype = ctypes.c_void_p; "
            "L.host_system_create_unchecked.argtypes = [ctypes.c_char_p, ctypes.c_int]; L.host_system_create_unchecked(sys.argv[1].encode(), int(sys.argv[2])); print('survived')")
    r = subprocess.run([sys.executable, "-c", code, str(bad), str(sensor)], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Dense.Mesh must be 0 or 1" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr)
