"""vdo_slam_amd/csrc/dense_plan.hpp - the two integer decisions every handle on a TSDF volume shares: what a move of the origin makes stale (dn_move)
and what a box leaves of the volume (dn_clip) - against brute force, in a stand-alone C++ program (tests/helpers/dense_plan_check.cpp): no GPU, no
library, nothing loaded into Python.

The cases.  Both functions decide per axis; what couples the axes is one flag (`all`, `empty`).  So every size 1..5, every origin -7..7 and every move
-12..12 (for the box: every lo and hi of -9..9, INT32_MIN, INT32_MAX) are crossed exhaustively ON each axis, with every size on the other two; the
axes together take every size and every move at once over three origin triples (for the box: 4 x 4 bounds per axis); then origins at +-(2^22 - 1).
The full product over three axes at once would be 6.6e9 moves and 3.6e13 boxes: it adds no case of either rule and does not run in seconds.
The brute force: a slot keeps its word iff its global voxel is the same before and after; a voxel of the volume is in the box iff lo <= g < hi."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "dense_plan_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", *FLAGS, *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("dense_plan ok:"), r.stdout


def test_move_and_box_equal_brute_force(tmp_path):
    _build_and_run(tmp_path, "dense_plan_check", ["-O2"])


def test_move_and_box_under_address_and_undefined_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link -fsanitize=address,undefined here: the sanitizer runtime (libasan / libubsan) is not installed")
    _build_and_run(tmp_path, "dense_plan_check_san", ["-O1", "-g", *san])
