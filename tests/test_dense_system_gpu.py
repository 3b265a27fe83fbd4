"""GPU: the dense mapper inside System (settings keys Dense.*, Tracking::FinishFrame, System::SaveDenseMap): a short synthetic sequence through
System::TrackRGBD; the saved points equal what vdo_slam_amd/dense.py (FollowingMap) makes from the downloaded depth, mask and poses of the same
frames; without the keys the trajectories are the same bytes and there is no mapper.  The host class on its own through host_dense_fuse."""
import ctypes as C

import numpy as np
import pytest

from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ

pytestmark = pytest.mark.gpu
W, H = synth.KITTI_W, synth.KITTI_H
N_FRAMES = 8
DENSE = dict(VoxelSize=0.25, Size=(96, 32, 160), MaxDepth=30.0, MaxWeight=32, MinWeight=1, Anchor=(0.5, 0.625, 0.05), RecenterMargin=4)


@pytest.fixture(scope="module")
def frames():
    Ts = SQ.camera_poses(N_FRAMES, step=1.6)               # 11 m in all: the ground first seen 6 m ahead leaves the volume, whose rear face follows 2 m behind the camera
    objs = SQ.default_objects()
    return [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]


def _settings(tmp_path, name, dense):
    from vdo_slam_amd.system import write_settings
    p = write_settings(tmp_path / name, W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    if dense:
        with open(p, "a") as f:
            for k, v in DENSE.items():
                f.write(f"Dense.{k}: {list(v) if isinstance(v, tuple) else v}\n")
    return p


def _run(settings, frames, each=None):
    from vdo_slam_amd.system import System
    s = System(settings, sensor="rgbd")
    poses = []
    for k, fr in enumerate(frames):
        depth = fr["depth_raw"].copy(); mask = fr["mask"].copy()
        T = s.track_rgbd(fr["gray"], depth, fr["flow"], mask)
        assert T is not None, k
        poses.append(T)
        if each:
            each(s, k, T)
    return s, np.stack(poses)


def test_the_saved_map_equals_the_python_flow_on_the_same_frames(frames, tmp_path):
    from vdo_slam_amd import dense as D
    from vdo_slam_amd.ba import Context
    ctx = Context(0)
    fm = D.FollowingMap(ctx, W, H, DENSE["Size"], DENSE["VoxelSize"], synth.KITTI_K, anchor=DENSE["Anchor"], margin=DENSE["RecenterMargin"], min_weight=DENSE["MinWeight"],
                        max_depth=DENSE["MaxDepth"], max_weight=DENSE["MaxWeight"])
    seen = []

    def each(s, k, T):
        depth, mask = s.last_depth_mask(W, H)
        counts = fm.fuse(depth, mask, T)
        info = s.dense_info()
        assert info is not None and info["counts"] == counts and info["origin"] == fm.mapper.origin() and info["recenters"] == fm.recenters, (k, info, counts)
        assert info["kept_points"] == sum(len(w) for w in fm.wgt)
        seen.append((counts, (mask != 0).sum()))

    s, poses = _run(_settings(tmp_path, "dense.yaml", True), frames, each)
    assert fm.recenters >= 1 and all(c[0] > 10000 for c, _ in seen) and any(c[1] > 0 for c, _ in seen)      # the volume moved; voxels were fused, some left out by the mask
    ply = tmp_path / "map.ply"
    assert s.save_dense_map(ply)
    xyz, nrm, wgt = D.read_ply(ply)
    X, N, Wt = fm.points()
    assert len(X) > 1000 and sum(len(w) for w in fm.wgt) > 0
    assert np.array_equal(xyz.view(np.uint32), X.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), N.view(np.uint32)) and np.array_equal(wgt, Wt)
    lens = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert ((np.abs(lens - 1) < 1e-6) | (lens == 0)).all() and (lens > 0).mean() > 0.5
    assert s.save_dense_map(ply) and np.array_equal(D.read_ply(ply)[0].view(np.uint32), X.view(np.uint32))       # saving changes nothing
    assert not s.save_dense_map(tmp_path / "no_such_dir" / "map.ply")
    s.close(); fm.close(); ctx.close()

    # without the keys: no mapper, and the same trajectory byte for byte (the mapper only reads what the tracker made)
    s0, poses0 = _run(_settings(tmp_path, "plain.yaml", False), frames)
    assert s0.dense_info() is None and not s0.save_dense_map(tmp_path / "none.ply") and not (tmp_path / "none.ply").exists()
    assert np.array_equal(poses0.view(np.uint32), poses.view(np.uint32))
    s0.close()


def test_the_host_class_on_host_frames(tmp_path):
    """DenseMapper::Fuse / SavePLY through host_dense_fuse against FollowingMap: a plane seen from a camera that walks out of a small volume"""
    from vdo_slam_amd import _capi as K, dense as D
    from vdo_slam_amd.ba import Context
    Wd, Hd, n, voxel, K4 = 48, 32, (24, 16, 20), 0.1, (40.0, 40.0, 23.5, 15.5)
    poses, depths, masks = [], [], []
    rng = np.random.default_rng(0)
    for k in range(7):
        T = np.eye(4, dtype=np.float32); T[0, 3] = -0.35 * k; T[2, 3] = -0.02 * k              # the camera moves along +x and a little towards the plane
        poses.append(T)
        depths.append((1.4 - 0.02 * k + rng.normal(0, 0.01, (Hd, Wd))).astype(np.float32))
        m = np.zeros((Hd, Wd), np.int32); m[4:9, 5 + k:12 + k] = 2
        masks.append(m)
    L = K.load_host_lib()
    L.host_dense_fuse.restype = C.c_longlong
    L.host_dense_fuse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_void_p]
    prm = D.params(n, voxel, K4, max_depth=10.0, stage_points=1000)
    anchor = np.array([0.5, 0.5, 0.25])
    info = np.zeros(2, np.int64)
    ply = tmp_path / "host.ply"
    dd, mm, tt = np.stack(depths), np.stack(masks), np.stack(poses)
    ctx = Context(0)
    for with_mask in (True, False):
        got = L.host_dense_fuse(dd.ctypes.data, mm.ctypes.data if with_mask else None, tt.ctypes.data, 7, Wd, Hd, C.byref(prm), anchor.ctypes.data, 2, 1, str(ply).encode(), info.ctypes.data)
        fm = D.FollowingMap(ctx, Wd, Hd, n, voxel, K4, anchor=anchor, margin=2, min_weight=1, max_depth=10.0)
        for k in range(7):
            fm.fuse(depths[k], masks[k] if with_mask else None, poses[k])
        X, N, Wt = fm.points()
        assert got == len(X) and got > 100 and info[0] == fm.recenters >= 2 and info[1] == sum(len(w) for w in fm.wgt) > 0
        xyz, nrm, wgt = D.read_ply(ply)
        assert np.array_equal(xyz.view(np.uint32), X.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), N.view(np.uint32)) and np.array_equal(wgt, Wt)
        fm.close()
    ctx.close()
