"""GPU: the distance field through System (settings key Dense.Distance, System::DenseClearance, System::ObjectClearances).  A short synthetic walk:
after every frame the clearances System reports equal, bit for bit, what vdo_slam_amd/distance.py gives on the volumes of the Python flow
(dense.FollowingMap, objects.ObjectMaps) fed with the downloaded depth, mask and poses; the field is computed again after a frame and not between
two queries; and the trajectory, the saved map, mesh and object models are the same bytes with the key and without it."""
import os

import numpy as np
import pytest

from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ

pytestmark = pytest.mark.gpu

W, H = synth.KITTI_W, synth.KITTI_H
DENSE = dict(VoxelSize=0.25, Size=(96, 32, 160), MaxDepth=30.0, MaxWeight=32, MinWeight=1, Anchor=(0.5, 0.625, 0.05), RecenterMargin=4, Mesh=1)
OBJECTS = dict(VoxelSize=0.05, Size=(80, 48, 80), MinPixels=300, MinFrames=2)
RADIUS = 2.0                                                                     # metres: 8 voxels
N_FRAMES = 6


def _settings(tmp_path, name, distance):
    from vdo_slam_amd.system import write_settings
    p = write_settings(tmp_path / name, W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    with open(p, "a") as f:
        for k, v in DENSE.items():
            f.write(f"Dense.{k}: {list(v) if isinstance(v, tuple) else v}\n")
        for k, v in OBJECTS.items():
            f.write(f"Dense.Objects.{k}: {list(v) if isinstance(v, tuple) else v}\n")
        if distance:
            f.write(f"Dense.Distance: 1\nDense.Distance.Radius: {RADIUS}\n")
    return p


def _run(settings, frames, each=None):
    from vdo_slam_amd.system import System
    s = System(settings, sensor="rgbd")
    poses = []
    for k, fr in enumerate(frames):
        T = s.track_rgbd(fr["gray"], fr["depth_raw"].copy(), fr["flow"], fr["mask"].copy(), obj_rows=np.array([[k, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in (1, 2, 3)], np.float32))
        assert T is not None, k
        poses.append(T)
        if each:
            each(s, k, T)
    return s, np.stack(poses)


def _saved(s, tmp_path, tag):
    assert s.save_dense_map(tmp_path / f"{tag}_map.ply") and s.save_dense_mesh(tmp_path / f"{tag}_mesh.ply") and s.save_object_maps(tmp_path / f"{tag}_obj")
    return {n[len(tag):]: open(tmp_path / n, "rb").read() for n in sorted(os.listdir(tmp_path)) if n.startswith(tag + "_")}


def test_clearances_equal_the_python_flow_and_the_key_changes_nothing_else(tmp_path):
    from vdo_slam_amd import dense as DN, distance as DD, objects as O
    from vdo_slam_amd.ba import Context
    Ts = SQ.camera_poses(N_FRAMES); objs = SQ.default_objects(box_depth=0.9)
    frames = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]
    ctx = Context(0)
    fm = DN.FollowingMap(ctx, W, H, DENSE["Size"], DENSE["VoxelSize"], synth.KITTI_K, anchor=DENSE["Anchor"], margin=DENSE["RecenterMargin"], min_weight=DENSE["MinWeight"],
                         max_depth=DENSE["MaxDepth"], max_weight=DENSE["MaxWeight"])
    om = O.ObjectMaps(ctx, W, H, synth.KITTI_K, OBJECTS["VoxelSize"], size=OBJECTS["Size"], max_depth=SF.TH_DEPTH_OBJ, max_weight=DENSE["MaxWeight"], min_pixels=OBJECTS["MinPixels"],
                      min_frames=OBJECTS["MinFrames"], min_weight=DENSE["MinWeight"])
    field = DD.DistanceField(ctx, DENSE["Size"])
    radius = int(np.ceil(float(np.float32(RADIUS)) / float(np.float32(DENSE["VoxelSize"]))))
    rng = np.random.default_rng(4)
    seen = dict(finite=0, far=0, outside=0, states=set(), objects=0)

    def each(s, k, T):
        depth, mask = s.last_depth_mask(W, H)
        fm.fuse(depth, mask, T)
        om.fuse(k, depth, mask, T, [(mod, sem, Hm) for mod, sem, _, Hm in s.object_motions()])
        assert field.compute_all(fm.mapper, DENSE["MinWeight"], radius)[0] > 0, k                     # the map has sites
        c = np.array(DN.camera_voxel(T, DENSE["VoxelSize"]), np.float64) * DENSE["VoxelSize"]
        pts = (c + rng.uniform([-14, -5, -4], [14, 5, 44], (4000, 3))).astype(np.float32)
        pts[7] = [np.nan, 0, 0]; pts[8] = [0, np.inf, 0]
        words = field.sample(pts)
        metres, state = s.dense_clearance(pts)
        assert s.distance_computes == k + 1, (k, s.distance_computes)                                 # computed again after the frame
        assert metres.dtype == np.float32 and state.dtype == np.uint8
        assert np.array_equal(metres.view(np.uint32), DD.metres(words, DENSE["VoxelSize"]).view(np.uint32)) and np.array_equal(state, DD.state(words)), k
        again = s.dense_clearance(pts[:50])
        assert s.distance_computes == k + 1 and np.array_equal(again[0].view(np.uint32), metres[:50].view(np.uint32))     # and not between two queries
        seen["finite"] += int(np.isfinite(metres).sum()); seen["far"] += int(np.isinf(metres).sum()); seen["outside"] += int(np.isnan(metres).sum())
        seen["states"] |= set(int(v) for v in np.unique(state))
        rows = s.object_clearances()
        s.dense_clearance(pts[:1])
        assert s.distance_computes == k + 1                                                           # the objects' query computed nothing either
        assert [mod for mod, _ in rows] == [m.mod_label for m in om.live], k
        if om.live:
            at = np.array([m.Two[:3, 3] for m in om.live]).astype(np.float32)
            want = DD.metres(field.sample(at), DENSE["VoxelSize"])
            assert np.array_equal(np.array([v for _, v in rows], np.float32).view(np.uint32), want.view(np.uint32)), (k, rows, want)
            seen["objects"] += len(rows)

    s, poses = _run(_settings(tmp_path, "distance.yaml", True), frames, each)
    print("seen:", seen)
    assert seen["finite"] > 1000 and seen["far"] > 1000 and seen["outside"] > 100 and {0, 1, 255} <= seen["states"] and seen["objects"] > 0
    assert s.dense_clearance(np.zeros((0, 3), np.float32))[0].size == 0
    with_key = _saved(s, tmp_path, "with")
    s.close()

    # the same run without the key: no clearances, and the same trajectory and files byte for byte
    s0, poses0 = _run(_settings(tmp_path, "plain.yaml", False), frames)
    assert s0.dense_clearance(np.zeros((3, 3), np.float32)) is None and s0.object_clearances() is None
    assert np.array_equal(poses0.view(np.uint32), poses.view(np.uint32))
    without = _saved(s0, tmp_path, "plain")
    assert sorted(with_key) == sorted(without) and len(with_key) >= 3
    for name in with_key:
        assert with_key[name] == without[name], name
    s0.close(); field.close(); om.close(); fm.close(); ctx.close()


def test_no_clearance_without_a_mapper(tmp_path):
    from vdo_slam_amd.system import System, write_settings
    s = System(write_settings(tmp_path / "nodense.yaml", W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ), sensor="rgbd")
    assert s.dense_clearance(np.zeros((2, 3), np.float32)) is None and s.object_clearances() is None
    s.close()
