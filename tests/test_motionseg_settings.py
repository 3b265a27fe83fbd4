"""CPU: the Motion.* settings keys (vdo_slam_amd/host/System.cc) through a flat hook of libvdo_host.so, which loads without a GPU: the defaults,
every key read back, and every value outside its range as a settings error - which ends a C++ caller's process, like the reference's."""
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
NAMES = ["SigmaFlow", "SigmaDisp", "Chi2", "VoteRadius", "VoteNum", "VoteDen", "MinKnown", "MinDisparity", "Class", "EgoStep", "EgoThreshold", "EgoIterations",
         "EgoConfidence", "EgoMinInliers"]


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_settings_check_motion.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    L.host_settings_read.argtypes = [C.c_char_p, C.c_void_p]
    return L


def _check(host, path):
    msg = C.create_string_buffer(256)
    out = np.full(14, -7.0)
    return host.host_settings_check_motion(str(path).encode(), msg, 256, out.ctypes.data), msg.value.decode(), dict(zip(NAMES, out))


def _with(tmp_path, name, lines):
    base = write_settings(tmp_path / "base.yaml", 1242, 375, KITTI_K, BF, 256.0, THBG, 25.0)
    p = tmp_path / name
    p.write_text(open(base).read() + "\n".join(lines) + "\n")
    return p


def test_defaults_and_every_key(host, tmp_path):
    plain = _with(tmp_path, "plain.yaml", [])
    rc, msg, v = _check(host, plain)
    assert (rc, msg) == (0, "")
    want = dict(SigmaFlow=0.5, SigmaDisp=0.5, Chi2=9, VoteRadius=2, VoteNum=1, VoteDen=2, MinKnown=6, MinDisparity=float(np.float32(BF) / np.float32(THBG)), Class=1, EgoStep=16,
                EgoThreshold=1.0, EgoIterations=500, EgoConfidence=0.98, EgoMinInliers=50)
    assert v == want
    mine = dict(SigmaFlow=0.25, SigmaDisp=2.0, Chi2=0, VoteRadius=7, VoteNum=2, VoteDen=3, MinKnown=225, MinDisparity=0.0, Class=255, EgoStep=1, EgoThreshold=0.5,
                EgoIterations=0, EgoConfidence=0.5, EgoMinInliers=0)
    keyed = _with(tmp_path, "keyed.yaml", [f"Motion.{k}: {val}" for k, val in mine.items()])
    rc, msg, v = _check(host, keyed)
    assert (rc, msg) == (0, "") and v == mine
    a, b = np.zeros(31), np.zeros(31)                             # the Motion.* lines change none of the 31 flat values
    assert host.host_settings_read(str(plain).encode(), a.ctypes.data) == 0 and host.host_settings_read(str(keyed).encode(), b.ctypes.data) == 0
    assert np.array_equal(a, b)
    assert _check(host, tmp_path / "absent.yaml")[0] == -2


BAD = [("SigmaFlow", "0"), ("SigmaFlow", "-1"), ("SigmaDisp", "0"), ("Chi2", "-0.5"), ("MinDisparity", "-1"), ("VoteRadius", "8"), ("VoteRadius", "-1"), ("VoteRadius", "1.5"),
       ("VoteDen", "0"), ("VoteDen", "65536"), ("VoteNum", "2"), ("VoteNum", "-1"), ("VoteNum", "7"), ("MinKnown", "0"), ("Class", "0"), ("Class", "256"), ("EgoStep", "0"),
       ("EgoStep", "2.5"), ("EgoThreshold", "0"), ("EgoIterations", "-1"), ("EgoConfidence", "0"), ("EgoConfidence", "1"), ("EgoMinInliers", "-1"), ("Chi2", "nan"),
       ("SigmaDisp", "inf"), ("EgoIterations", "1e12")]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_are_settings_errors(host, tmp_path, key, value):
    lines = [f"Motion.{key}: {value}"]
    rc, msg, v = _check(host, _with(tmp_path, "bad.yaml", lines))
    word = "Motion.VoteDen" if (key, value) == ("VoteNum", "2") else f"Motion.{key}"
    assert rc == 1 and msg.startswith("settings: ") and word in msg, msg
    assert all(x == -7.0 for x in v.values())                     # nothing is reported beside an error


def test_a_bad_value_ends_the_process_with_the_stereo_sensor_only(tmp_path):
    """System(settings, sensor) as a C++ caller gets it: a Motion.* settings error exits with -1 and its message before any device is touched, with
    the STEREO sensor; an RGBD system never reads the keys.  In a child process, since it ends the process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = _with(tmp_path, "bad.yaml", ["Motion.VoteRadius: 9"])
    code = ("import ctypes, sys; from vdo_slam_amd import _capi as K; L = K.load_host_lib(); L.host_system_create_unchecked.restype = ctypes.c_void_p; "
            "L.host_system_create_unchecked.argtypes = [ctypes.c_char_p, ctypes.c_int]; L.host_system_create_unchecked(sys.argv[1].encode(), int(sys.argv[2])); print('survived')")
    r = subprocess.run([sys.executable, "-c", code, str(bad), "1"], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Motion.VoteRadius outside 0..7" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr)
    r = subprocess.run([sys.executable, "-c", code, str(bad), "0"], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Motion." not in r.stderr and "survived" in r.stdout, (r.returncode, r.stderr)
