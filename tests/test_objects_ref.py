"""CPU: the NumPy restatement of the object mapper (tests/objects_ref.py) against a plain Python loop, against the ground truth of the project's own
renderer, and on hand-made cases of its lifecycle."""
import math

import numpy as np
import pytest

from tests import objects_ref as OR
from vdo_slam_amd import synth_seq as SQ
from vdo_slam_amd.synth import KITTI_H, KITTI_K, KITTI_W

F = np.float32


def test_stats_against_a_plain_loop():
    W, H, max_labels = 7, 5, 3
    K4 = (5.5, 4.25, 3.1, 2.2)
    rng = np.random.default_rng(4)
    depth = rng.uniform(0.5, 9.0, (H, W)).astype(F)
    depth[0, 0] = np.nan; depth[1, 2] = np.inf; depth[2, 3] = 0.0; depth[3, 4] = 8.0; depth[4, 5] = F(np.nextafter(F(8.0), F(np.inf))); depth[4, 6] = -1.0
    mask = rng.integers(-1, 5, (H, W)).astype(np.int32)
    mask[3, 4] = 2; mask[4, 5] = 2
    got = OR.stats(depth, mask, K4, 0.6, 8.0, max_labels)
    want = [[0, W, H, -1, -1, 0, 0, 0] for _ in range(max_labels + 1)]
    fx, fy, cx, cy = (F(v) for v in K4)
    for y in range(H):
        for x in range(W):
            d = depth[y, x]
            if not (math.isfinite(float(d)) and d > F(0.6) and d <= F(8.0)):
                continue
            l = int(mask[y, x])
            if l == 0:
                continue
            if l < 1 or l > max_labels:
                want[0][0] += 1
                continue
            r = want[l]
            r[0] += 1; r[1] = min(r[1], x); r[2] = min(r[2], y); r[3] = max(r[3], x); r[4] = max(r[4], y)
            t = F(F(F(x) - cx) * d); t = F(t / fx); t = F(t * F(1024)); r[5] += int(math.floor(float(F(t + F(0.5)))))
            t = F(F(F(y) - cy) * d); t = F(t / fy); t = F(t * F(1024)); r[6] += int(math.floor(float(F(t + F(0.5)))))
            r[7] += int(math.floor(float(F(F(d * F(1024)) + F(0.5)))))
    assert got.dtype == np.int64 and np.array_equal(got, np.array(want, np.int64))
    assert got[0, 0] > 0 and (got[1:, 0] > 0).all() and got[2, 3] >= 4                  # the depth == max_depth pixel counts, the float above it does not


# ---- the lifecycle on the project's renderer ---------------------------------------------------------------------------------------------------
VOXEL, SIZE, N_FRAMES, LEAVE, ENTER = 0.05, (80, 48, 80), 10, 7, 3


def _box_distance(ob, k, Xw):
    """Distance of world points to the surface of the box `ob` at frame k"""
    Ro, c = SQ.object_pose(ob, k)
    p = np.abs((Xw - c) @ Ro) - np.array([ob["hw"], ob["hh"], ob["hd"]])
    outside = np.linalg.norm(np.maximum(p, 0.0), axis=1)
    inside = np.minimum(p.max(axis=1), 0.0)
    return np.abs(outside + inside)


@pytest.fixture(scope="module")
def survey():
    objs = SQ.survey_objects(leave_at=LEAVE, enter_at=ENTER)
    Ts = SQ.camera_poses(N_FRAMES)
    maps = OR.RefMaps(KITTI_W, KITTI_H, KITTI_K, VOXEL, size=SIZE, max_depth=25.0, min_pixels=200, min_frames=3, min_weight=2, max_labels=16)
    started = {}
    for k in range(N_FRAMES):
        fr = SQ.render_frame(k, Ts, objs)
        depth = np.where(np.isfinite(fr["depth_true"]), fr["depth_true"], 0.0).astype(F)
        motions = [(100 + j, j + 1, SQ.object_motion(ob, k - 1) if k else np.eye(4)) for j, ob in enumerate(objs) if SQ.object_exists(ob, k)]
        maps.fuse(k, depth, fr["mask"], fr["Tcw"], motions)
        for m in maps.live:
            started.setdefault(m.mod_label, (k, m.Two.copy()))
    return objs, maps, started


def test_models_of_turning_boxes_lie_on_the_boxes(survey):
    """Every extracted point of every model, taken to the world through the model's last Two, lies within one voxel diagonal (sqrt(3) * voxel = 86.6 mm:
    a crossing lies between two adjacent voxel centres on each axis) of the box's surface at that frame.  Worst distance measured: 20.3 mm (per model 4.0 - 20.3 mm)."""
    objs, maps, _ = survey
    models = maps.models()
    assert len(models) >= 4 and any(not m["live"] for m in models) and maps.dropped == 0
    worst = 0.0
    for m in models:
        ob = objs[m["mod_label"] - 100]
        k, Two = m["trajectory"][-1]
        assert len(m["xyz"]) > 500 and m["frames"] >= 3, m["mod_label"]
        Xw = m["xyz"].astype(np.float64) @ Two[:3, :3].T + Two[:3, 3]
        d = _box_distance(ob, k, Xw)
        worst = max(worst, float(d.max()))
        print(f"object {m['mod_label']}: {len(d)} points, {m['frames']} frames, worst {d.max() * 1e3:.1f} mm, mean {d.mean() * 1e3:.1f} mm")
    assert worst <= math.sqrt(3.0) * VOXEL, worst


def test_the_chained_pose_is_the_composed_ground_truth(survey):
    objs, maps, started = survey
    for m in maps.finished + maps.live:
        ob = objs[m.mod_label - 100]
        k0, Two0 = started[m.mod_label]
        for k, Two in m.traj:
            R0, c0 = SQ.object_pose(ob, k0); Rk, ck = SQ.object_pose(ob, k)
            G = np.eye(4); G[:3, :3] = Rk @ R0.T; G[:3, 3] = ck - G[:3, :3] @ c0
            assert np.abs(Two - G @ Two0).max() <= 1e-9, (m.mod_label, k)
    gone = [m for m in maps.finished if m.mod_label == 101]
    assert len(gone) == 1 and gone[0].traj[-1][0] == LEAVE - 1 and gone[0].frames == LEAVE              # object 2 left: retired with its last pose
    assert any(m.mod_label == 104 and m.traj[0][0] == ENTER for m in maps.live)                         # object 5 entered at its frame


# ---- hand-made lifecycle cases: 48 x 32 images, a 24^3 volume ------------------------------------------------------------------------------------
W, H, K4 = 48, 32, (40.0, 40.0, 23.5, 15.5)


def _frame(blobs):
    """blobs: [(label, x0, y0, x1, y1, depth)] on a background at 4 m"""
    depth = np.full((H, W), 4.0, F); mask = np.zeros((H, W), np.int32)
    for l, x0, y0, x1, y1, d in blobs:
        depth[y0:y1, x0:x1] = d; mask[y0:y1, x0:x1] = l
    return depth, mask


def _maps(**kw):
    prm = dict(size=(24, 24, 24), max_depth=10.0, min_pixels=20, min_frames=2, min_weight=1, max_labels=7)
    prm.update(kw)
    return OR.RefMaps(W, H, K4, 0.05, **prm)


def _shift(dx):
    Hm = np.eye(4); Hm[0, 3] = dx
    return Hm


def test_a_walking_label_is_retired_as_a_model():
    m = _maps()
    for k in range(3):
        depth, mask = _frame([(3, 10 + 2 * k, 8, 20 + 2 * k, 20, 2.0)])
        m.fuse(k, depth, mask, np.eye(4), [(7, 3, _shift(0.1))])
    assert [(x.mod_label, x.frames) for x in m.live] == [(7, 3)] and np.allclose(m.live[0].Two[0, 3] - m.live[0].traj[0][1][0, 3], 0.2, atol=1e-12)
    depth, mask = _frame([])
    m.fuse(3, depth, mask, np.eye(4), [])
    assert not m.live and m.dropped == 0 and [(x["mod_label"], x["live"], x["frames"]) for x in m.models()] == [(7, False, 3)]
    fin = m.finished[0]
    assert len(fin.xyz) > 0 and [f for f, _ in fin.traj] == [0, 1, 2]
    # the centroid of the first frame is the middle of the volume: camera (x, y, z) of the blob's mean pixel at 2 m
    assert np.allclose(fin.traj[0][1][:3, 3], [((14.5 - 23.5) * 2.0) / 40.0, ((13.5 - 15.5) * 2.0) / 40.0, 2.0], atol=2e-3)


def test_a_short_lived_label_is_dropped():
    m = _maps(min_frames=3)
    for k in range(2):
        m.fuse(k, *_frame([(1, 4, 4, 14, 14, 3.0)]), np.eye(4), [(5, 1, np.eye(4))])
    m.fuse(2, *_frame([]), np.eye(4), [])
    assert not m.live and not m.finished and m.dropped == 1


def test_skips_by_max_objects_and_min_pixels():
    m = _maps(max_objects=1)
    depth, mask = _frame([(1, 4, 4, 14, 14, 3.0), (2, 30, 4, 40, 14, 3.0), (3, 20, 20, 23, 23, 3.0)])
    m.fuse(0, depth, mask, np.eye(4), [(5, 1, np.eye(4)), (6, 2, np.eye(4))])
    assert [x.mod_label for x in m.live] == [5] and m.skipped == 1                       # the second object finds no free model
    m2 = _maps()
    m2.fuse(0, depth, mask, np.eye(4), [(9, 3, np.eye(4)), (8, 6, np.eye(4)), (7, 99, np.eye(4))])
    assert not m2.live and m2.skipped == 3                                               # 9 pixels; a label without pixels; a label beyond max_labels
    # a live model whose label falls below MinPixels keeps its chained pose and is not fused
    m3 = _maps()
    m3.fuse(0, depth, mask, np.eye(4), [(5, 1, np.eye(4))])
    words = m3.live[0].V.words.copy()
    x0 = m3.live[0].Two[0, 3]
    m3.fuse(1, *_frame([(1, 4, 4, 6, 6, 3.0)]), np.eye(4), [(5, 1, _shift(0.25))])
    assert m3.live[0].frames == 1 and np.array_equal(m3.live[0].V.words, words) and m3.live[0].Two[0, 3] == x0 + 0.25 and len(m3.live[0].traj) == 2


def test_repeated_labels_are_ignored_after_their_first_use():
    m = _maps()
    depth, mask = _frame([(1, 4, 4, 14, 14, 3.0), (2, 30, 4, 40, 14, 3.0)])
    m.fuse(0, depth, mask, np.eye(4), [(5, 1, np.eye(4)), (5, 2, np.eye(4)), (6, 1, np.eye(4)), (7, 2, np.eye(4))])
    assert [(x.mod_label, x.sem_label) for x in m.live] == [(5, 1), (7, 2)] and m.skipped == 0
    x5 = m.live[0].Two[0, 3]
    m.fuse(1, depth, mask, np.eye(4), [(5, 1, _shift(0.5)), (5, 1, _shift(0.5)), (7, 2, np.eye(4))])
    assert m.live[0].Two[0, 3] == x5 + 0.5                                               # the motion is applied once
