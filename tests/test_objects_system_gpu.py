"""GPU: the object mapper inside System (settings keys Dense.Objects.*, Tracking::FinishFrame, System::SaveObjectMaps): a short synthetic sequence
through System::TrackRGBD; after every frame the models equal what vdo_slam_amd/objects.py (ObjectMaps) makes from the downloaded depth and mask,
the fused pose and the tracker's own motions; the saved files are the same bytes; without the keys nothing changes.  The host class on its own
through host_objects_fuse."""
import ctypes as C
import os

import numpy as np
import pytest

from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ

pytestmark = pytest.mark.gpu
W, H = synth.KITTI_W, synth.KITTI_H
N_FRAMES = 8
DENSE = dict(VoxelSize=0.25, Size=(96, 32, 160), MaxDepth=30.0, MaxWeight=32, MinWeight=1, Anchor=(0.5, 0.625, 0.05), RecenterMargin=4)
OBJECTS = dict(VoxelSize=0.05, Size=(80, 48, 80), MinPixels=300, MinFrames=2)


@pytest.fixture(scope="module")
def frames():
    Ts = SQ.camera_poses(N_FRAMES)
    objs = SQ.default_objects(box_depth=0.9)
    return [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]


def _settings(tmp_path, name, objects):
    from vdo_slam_amd.system import write_settings
    p = write_settings(tmp_path / name, W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    with open(p, "a") as f:
        for k, v in DENSE.items():
            f.write(f"Dense.{k}: {list(v) if isinstance(v, tuple) else v}\n")
        if objects:
            for k, v in OBJECTS.items():
                f.write(f"Dense.Objects.{k}: {list(v) if isinstance(v, tuple) else v}\n")
    return p


def _run(settings, frames, each=None):
    from vdo_slam_amd.system import System
    s = System(settings, sensor="rgbd")
    poses = []
    for k, fr in enumerate(frames):
        depth = fr["depth_raw"].copy(); mask = fr["mask"].copy()
        rows = np.array([[k, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in (1, 2, 3)], np.float32)       # the ground-truth object rows of the frame: the tracker's gate
        T = s.track_rgbd(fr["gray"], depth, fr["flow"], mask, obj_rows=rows)
        assert T is not None, k
        poses.append(T)
        if each:
            each(s, k, T)
    return s, np.stack(poses)


def _same_files(a, b, names):
    for name in names:
        assert open(str(a) + name, "rb").read() == open(str(b) + name, "rb").read(), name


def test_the_models_equal_the_python_flow_on_the_same_frames(frames, tmp_path):
    from vdo_slam_amd import objects as O
    from vdo_slam_amd.ba import Context
    ctx = Context(0)
    om = O.ObjectMaps(ctx, W, H, synth.KITTI_K, OBJECTS["VoxelSize"], size=OBJECTS["Size"], max_depth=SF.TH_DEPTH_OBJ, max_weight=DENSE["MaxWeight"], min_pixels=OBJECTS["MinPixels"],
                      min_frames=OBJECTS["MinFrames"], min_weight=DENSE["MinWeight"])
    tracked = []

    def each(s, k, T):
        depth, mask = s.last_depth_mask(W, H)
        motions = s.object_motions()
        om.fuse(k, depth, mask, T, [(mod, sem, Hm) for mod, sem, _, Hm in motions])
        info = s.object_info()
        assert info is not None and info["models"] == om.info() and (info["dropped"], info["skipped"]) == (om.dropped, om.skipped), (k, info, om.info())
        tracked.append(len(motions))
        print(f"frame {k}: {len(motions)} motions, models {info['models']}, dropped {info['dropped']}, skipped {info['skipped']}")

    s, poses = _run(_settings(tmp_path, "objects.yaml", True), frames, each)
    # the tracker itself reports at least two objects over at least four consecutive frames
    runs = "".join("1" if n >= 2 else "0" for n in tracked)
    assert "1111" in runs, tracked
    live = [m for m in om.info() if m[1]]
    assert len(live) >= 2 and max(m[2] for m in live) >= 4 and all(m[3] > 200 for m in live if m[2] >= 2), om.info()
    a, b = tmp_path / "sys", tmp_path / "py"
    assert s.save_object_maps(a)
    om.save(b)
    names = sorted(n[len("sys"):] for n in os.listdir(tmp_path) if n.startswith("sys_"))
    assert names == sorted(n[len("py"):] for n in os.listdir(tmp_path) if n.startswith("py_")) and "_poses.txt" in names and len(names) == len(om.info()) + 1
    _same_files(a, b, names)
    assert s.save_object_maps(tmp_path / "again")
    _same_files(a, tmp_path / "again", names)                              # saving changes nothing
    assert s.object_info()["models"] == om.info()
    assert not s.save_object_maps(tmp_path / "no_such_dir" / "sys")
    best = max(live, key=lambda m: m[3])
    view = s.render_object_view(best[0], poses[-1], W, H)
    assert view is not None and (view[0] > 0).sum() > 200                  # a render of one object returns hits
    lens = np.linalg.norm(view[1].astype(np.float64), axis=2)
    assert ((np.abs(lens - 1) < 1e-6) | (lens == 0)).all()
    assert s.render_object_view(987654, poses[-1], W, H) is None
    static_ply = tmp_path / "static.ply"
    assert s.save_dense_map(static_ply)
    s.close(); om.close(); ctx.close()

    # without Dense.Objects.VoxelSize: no object mapper, and the trajectory and the static map are the same bytes
    s0, poses0 = _run(_settings(tmp_path, "plain.yaml", False), frames)
    assert s0.object_info() is None and not s0.save_object_maps(tmp_path / "none") and s0.render_object_view(best[0], poses[-1], W, H) is None
    assert not [n for n in os.listdir(tmp_path) if n.startswith("none")]
    assert np.array_equal(poses0.view(np.uint32), poses.view(np.uint32))
    plain_ply = tmp_path / "plain.ply"
    assert s0.save_dense_map(plain_ply) and plain_ply.read_bytes() == static_ply.read_bytes()
    s0.close()


def test_the_host_class_on_host_frames(tmp_path):
    """ObjectMapper::Fuse / SaveModels through host_objects_fuse against ObjectMaps: 48 x 32 images, a 24^3 volume, a label that walks and then
    disappears, a second label that stays, a label without pixels"""
    from vdo_slam_amd import _capi as K, dense as D, objects as O
    from vdo_slam_amd.ba import Context
    Wd, Hd, K4, n, voxel = 48, 32, (40.0, 40.0, 23.5, 15.5), (24, 24, 24), 0.05
    Tcw = np.eye(4); a = 0.1
    Tcw[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]; Tcw[:3, 3] = [0.05, -0.02, 0.1]
    Tcw = Tcw.astype(np.float32)
    ys, xs = np.mgrid[0:Hd, 0:Wd]
    Hm = np.eye(4, dtype=np.float32); Hm[:3, 3] = Tcw[:3, :3].T @ np.array([0.1, 0.0, 0.0], np.float32)
    depths, masks, motions = [], [], []
    for k in range(6):
        depth = np.full((Hd, Wd), 4.0, np.float32); mask = np.zeros((Hd, Wd), np.int32)
        if k < 4:
            sel = (xs >= 10 + 2 * k) & (xs < 24 + 2 * k) & (ys >= 8) & (ys < 22)
            depth[sel] = (2.0 + 0.01 * (xs - 17 - 2 * k))[sel]; mask[sel] = 3
        mask[2:6, 40:46] = 5
        depths.append(depth); masks.append(mask)
        motions.append(([(11, 3, Hm)] if k < 4 else []) + [(12, 5, np.eye(4, dtype=np.float32)), (13, 6, np.eye(4, dtype=np.float32))])
    L = K.load_host_lib()
    L.host_objects_fuse.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    prm = D.params(n, voxel, K4, max_depth=10.0, stage_points=512)
    life = np.array([2, 20, 2, 1, 7], np.int32)
    dd, mm, tt = np.stack(depths), np.stack(masks), np.stack([Tcw] * 6)
    n_mot = np.array([len(m) for m in motions], np.int32)
    mod = np.array([q[0] for m in motions for q in m], np.int32); sem = np.array([q[1] for m in motions for q in m], np.int32)
    HH = np.ascontiguousarray(np.stack([q[2] for m in motions for q in m]), np.float32)
    rows = np.zeros((8, 4), np.int64); counts = np.zeros(2, np.int64)
    got = L.host_objects_fuse(dd.ctypes.data, mm.ctypes.data, tt.ctypes.data, 6, Wd, Hd, C.byref(prm), life.ctypes.data, n_mot.ctypes.data, mod.ctypes.data, sem.ctypes.data,
                              HH.ctypes.data, str(tmp_path / "host").encode(), 8, rows.ctypes.data, counts.ctypes.data)
    ctx = Context(0)
    om = O.ObjectMaps(ctx, Wd, Hd, K4, voxel, size=n, max_depth=10.0, max_objects=2, min_pixels=20, min_frames=2, min_weight=1, max_labels=7, stage_points=512)
    for k in range(6):
        om.fuse(k, depths[k], masks[k], Tcw, motions[k])
    info = om.info()
    assert got == len(info) == 2 and [tuple(int(v) for v in r) for r in rows[:got]] == [(m[0], int(m[1]), m[2], m[3]) for m in info]
    assert info[0][:3] == (11, False, 4) and info[0][3] > 100 and info[1][:3] == (12, True, 6) and (int(counts[0]), int(counts[1])) == (om.dropped, om.skipped) == (0, 6)
    om.save(tmp_path / "py")
    _same_files(tmp_path / "host", tmp_path / "py", ["_11.ply", "_12.ply", "_poses.txt"])
    om.close(); ctx.close()
