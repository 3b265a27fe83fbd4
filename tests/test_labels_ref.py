"""CPU: the NumPy restatement of the instance labeller's contract (tests/labels_ref.py) checked on its own - against a plain Python flood fill, on
the properties the contract states, on the threshold rule with ties and on the disparity gate.  tests/test_labels_gpu.py compares the device with
this restatement array_equal, so the device inherits what is shown here."""
import os
import re
from collections import deque

import numpy as np
import pytest

from tests import labels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flood(member, linked, connectivity):
    """roots by breadth-first search over the full (symmetric) neighbourhood; linked(y0, x0, y1, x1) on scalars"""
    H, W = member.shape
    nb = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (-1, -1), (-1, 1), (1, -1)] if connectivity == 8 else [])
    roots = np.full((H, W), -1, np.int64)
    for y in range(H):
        for x in range(W):
            if not member[y, x] or roots[y, x] >= 0:
                continue
            seed = y * W + x                                     # raster scan: the first pixel met is the component's smallest index
            roots[y, x] = seed
            todo = deque([(y, x)])
            while todo:
                cy, cx = todo.popleft()
                for dx, dy in nb:
                    yy, xx = cy + dy, cx + dx
                    if 0 <= yy < H and 0 <= xx < W and member[yy, xx] and roots[yy, xx] < 0 and linked(cy, cx, yy, xx):
                        roots[yy, xx] = seed
                        todo.append((yy, xx))
    return roots


def _flood_instances(cls, disp, connectivity, tau):
    d = R.int_disparity(disp) if tau >= 0 else None

    def linked(y0, x0, y1, x1):
        if cls[y0, x0] != cls[y1, x1]:
            return False
        return tau < 0 or d[y0, x0] == 0 or d[y1, x1] == 0 or abs(int(d[y0, x0]) - int(d[y1, x1])) <= tau
    return _flood(cls != 0, linked, connectivity)


def _mask_from_roots(roots, min_area, max_labels):
    """labels by the definitions, in plain Python: areas, the threshold by trying every A upwards, numbers in order of first pixel"""
    flat = roots.ravel()
    area = {}
    for r in flat:
        if r >= 0:
            area[int(r)] = area.get(int(r), 0) + 1
    A = min_area
    while sum(1 for v in area.values() if v >= A) > max_labels:
        A += 1
    number = {r: k + 1 for k, r in enumerate(sorted(r for r, v in area.items() if v >= A))}
    if A > min_area and number:                                  # reported: the area of the smallest component kept
        A = min(area[r] for r in number)
    mask = np.array([number.get(int(r), 0) for r in flat], np.int32).reshape(roots.shape)
    areas = np.zeros(flat.size, np.int64)
    for r, v in area.items():
        areas[r] = v
    return mask, len(number), len(area), A, areas.reshape(roots.shape)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_the_flood_fill(connectivity, gate):
    for seed in range(20):
        rng = np.random.default_rng(seed)
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        cls = R.noise(H, W, float(rng.choice([0.4, 0.59, 0.8])), seed + 100, classes=int(rng.integers(1, 4)))
        disp = (rng.integers(0, 6, (H, W)) * rng.integers(0, 2, (H, W))).astype(np.float32) + np.float32(0.5)      # zeros (0.5 truncates to 0) among 1..5
        tau = int(rng.integers(0, 3)) if gate else -1
        min_area, max_labels = int(rng.integers(1, 5)), int(rng.integers(1, 12))
        got = R.stages(cls, disp, connectivity, tau, min_area, max_labels)
        roots = _flood_instances(cls, disp, connectivity, tau)
        mask, n, nc, A, areas = _mask_from_roots(roots, min_area, max_labels)
        what = f"seed {seed} {W}x{H}"
        assert np.array_equal(got["roots"], roots), what
        assert np.array_equal(got["areas"], areas), what
        assert np.array_equal(got["mask"], mask), what
        assert got["counts"] == (n, nc, A), what


@pytest.mark.parametrize("connectivity", [4, 8])
def test_properties(connectivity):
    cls = R.noise(24, 23, 0.59, 5, classes=2)
    s = R.stages(cls, None, connectivity, -1, 3, 7)
    roots, areas, mask = s["roots"], s["areas"], s["mask"]
    n, nc, A = s["counts"]
    idx = np.arange(cls.size).reshape(cls.shape)
    assert ((roots >= 0) == (cls != 0)).all()
    for r in np.unique(roots[roots >= 0]):
        assert idx[roots == r].min() == r                        # the root is the smallest index of its component
        assert areas.ravel()[r] == (roots == r).sum()
    assert areas.sum() == (cls != 0).sum()
    assert nc == (areas > 0).sum()
    labels = np.unique(mask[mask > 0])
    assert np.array_equal(labels, np.arange(1, n + 1))           # 1..n without gaps
    first = [idx[mask == k].min() for k in range(1, n + 1)]
    assert first == sorted(first)                                # in raster order of the first pixel
    assert n <= 7 and A >= 3
    assert (areas.ravel()[roots[mask > 0]] >= A).all() and (areas.ravel()[roots[(mask == 0) & (roots >= 0)]] < A).all()


FIVE = [3, 3, 2, 2, 1]                                           # squares of areas 9, 9, 4, 4, 1


@pytest.mark.parametrize("max_labels,A,n", [(3, 9, 2), (4, 4, 4), (1, 10, 0), (5, 1, 5), (1023, 1, 5)])
def test_threshold_rule_with_ties(max_labels, A, n):
    cls = R.blobs(8, 24, FIVE)
    s = R.stages(cls, None, 4, -1, 1, max_labels)
    assert s["counts"] == (n, 5, A)
    assert sorted(np.unique(s["mask"])) == list(range(0, n + 1))
    assert R.area_threshold([9, 9, 4, 4, 1], 5, 1023) == 5       # nothing overflows: min_area itself
    assert R.area_threshold([9, 9, 4, 4, 1], 5, 1) == 10


def test_gate_semantics():
    tau = 3
    cls = np.ones((6, 10), np.uint8)
    disp = np.full((6, 10), 20.0, np.float32)
    disp[:, 5:] = 20.0 + tau                                     # two rectangles of one class touching along an edge
    assert R.stages(cls, disp, 4, tau)["counts"][1] == 1
    disp[:, 5:] = 20.0 + tau + 1
    assert R.stages(cls, disp, 4, tau)["counts"][1] == 2
    assert R.stages(cls, disp, 4, -1)["counts"][1] == 1          # gate off
    wide = np.ones((6, 11), np.uint8)
    d3 = np.full((6, 11), 20.0, np.float32)
    d3[:, 6:] = 20.0 + tau + 1
    d3[:, 5] = 0.0                                               # a column of unknown disparity between them joins them
    assert R.stages(wide, d3, 4, tau)["counts"][1] == 1
    d3[:, 5] = np.nan
    assert R.stages(wide, d3, 4, tau)["counts"][1] == 1
    assert np.array_equal(R.int_disparity(np.array([np.nan, -1.0, 2.0 ** 24, 2.0 ** 24 - 1, 7.99, np.inf], np.float32)), [0, 0, 0, 2 ** 24 - 1, 7, 0])


def test_speckle_mode_equals_the_flood_fill():
    for seed in range(20):
        rng = np.random.default_rng(seed)
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        disp = (rng.integers(0, 8, (H, W)) * (rng.random((H, W)) < 0.7)).astype(np.float32) * np.float32(1.25)
        max_diff, max_size = int(rng.integers(0, 3)), int(rng.integers(0, 6))
        got = R.filter_speckles(disp, max_diff, max_size)
        d = R.int_disparity(disp)
        roots = _flood(d != 0, lambda y0, x0, y1, x1: abs(int(d[y0, x0]) - int(d[y1, x1])) <= max_diff, 4)
        _, _, _, _, areas = _mask_from_roots(roots, 1, 1 << 30)
        drop = (roots >= 0) & (areas.ravel()[np.maximum(roots, 0)] <= max_size)
        assert np.array_equal(got["roots"], roots) and np.array_equal(got["areas"], areas), seed
        assert got["n_removed"] == drop.sum(), seed
        assert (got["disp"][drop] == 0).all() and np.array_equal(got["disp"][~drop].view(np.uint32), disp[~drop].view(np.uint32)), seed


def test_patterns_are_what_they_say():
    for H, W in ((64, 96), (17, 65)):
        for a in (R.spiral(H, W), R.serpentine(H, W), R.comb(H, W, True), R.comb(H, W, False)):
            assert R.stages(a, None, 4)["counts"][1] == 1
        assert R.spiral(H, W).sum() > H * W // 3                 # arms one pixel wide, one free pixel between them: about half the image
        cb = R.checkerboard(H, W)
        assert R.stages(cb, None, 4)["counts"][1] == (cb != 0).sum() and R.stages(cb, None, 8)["counts"][1] == 1


SYMBOLS = ["vdo_labels_create", "vdo_labels_destroy", "vdo_labels_compute", "vdo_labels_filter_speckles", "vdo_labels_get_roots", "vdo_labels_get_areas",
           "vdo_labels_last_timing", "vdo_labels_device_images", "vdo_labels_stage_classes"]


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "vdo_slam_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/vdo_slam_hip.h"
    assert re.search(r"typedef struct vdo_labels_params \{[^}]*connectivity[^}]*max_disp_diff[^}]*min_area[^}]*max_labels[^}]*\}", header)
    from vdo_slam_amd import labels
    assert [f[0] for f in labels.LabelParamsC._fields_] == ["connectivity", "max_disp_diff", "min_area", "max_labels"]
    L = labels._lib()                                            # the library loads without a GPU; only calls need one
    for name in SYMBOLS:
        fn = getattr(L, name)                                    # AttributeError: the library does not export it
        assert fn.argtypes is not None, f"{name} is not bound in vdo_slam_amd/labels.py"
    assert callable(labels.compute) and callable(labels.filter_speckles) and hasattr(labels.InstanceLabeler, "compute")
    from vdo_slam_amd.system import System
    assert hasattr(System, "track_stereo_pair_semantic")
    host = open(os.path.join(ROOT, "vdo_slam_amd", "host", "host_capi.cc")).read()
    assert "host_labels_compute" in host and "host_system_track_stereo_pair_semantic" in host
