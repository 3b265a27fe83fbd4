"""GPU: the raycaster behind the host class and System (DenseMapper::Render, System::RenderDenseView, settings keys Dense.View.*): the host class on
host frames through host_dense_render, and a short synthetic sequence through System::TrackRGBD, both against vdo_slam_amd/raycast.py on the Python
flow (dense.FollowingMap) of the same frames, bit for bit; rendering changes nothing of the tracker; without the keys there is no view."""
import ctypes as C

import numpy as np
import pytest

from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ

pytestmark = pytest.mark.gpu
F = np.float32


def _n_steps(near, step, max_depth):
    """ceil((MaxDepth - Near) / Step) + 1 in double on the float32 values, as DenseMapper::CheckView"""
    return int(np.ceil((float(F(max_depth)) - float(F(near))) / float(F(step)))) + 1


def _same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), what


def test_the_host_class_renders_what_the_python_flow_renders():
    """The 48 x 32 plane sequence of test_dense_system_gpu.py::test_the_host_class_on_host_frames through host_dense_render"""
    from vdo_slam_amd import _capi as K, dense as D, raycast as RY
    from vdo_slam_amd.ba import Context
    Wd, Hd, n, voxel, K4 = 48, 32, (24, 16, 20), 0.1, (40.0, 40.0, 23.5, 15.5)
    poses, depths, masks = [], [], []
    rng = np.random.default_rng(0)
    for k in range(7):
        T = np.eye(4, dtype=F); T[0, 3] = -0.35 * k; T[2, 3] = -0.02 * k
        poses.append(T)
        depths.append((1.4 - 0.02 * k + rng.normal(0, 0.01, (Hd, Wd))).astype(F))
        m = np.zeros((Hd, Wd), np.int32); m[4:9, 5 + k:12 + k] = 2
        masks.append(m)
    L = K.load_host_lib()
    L.host_dense_render.restype = C.c_int
    L.host_dense_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    prm = D.params(n, voxel, K4, max_depth=10.0, stage_points=1000)
    anchor = np.array([0.5, 0.5, 0.25])
    dd, mm, tt = np.stack(depths), np.stack(masks), np.stack(poses)
    turned = poses[5].copy()
    a = np.deg2rad(12.0); turned[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F)
    ctx = Context(0)
    fm = D.FollowingMap(ctx, Wd, Hd, n, voxel, K4, anchor=anchor, margin=2, min_weight=1, max_depth=10.0)
    for k in range(7):
        fm.fuse(depths[k], masks[k], poses[k])
    assert fm.recenters >= 2
    # the defaults of the view: Near max(min_depth, voxel), Step trunc / 2, MinWeight the mapper's; then keys of our own
    d_near, d_step = float(max(F(0.0), F(voxel))), float(F(prm.trunc) / F(2))
    hits = 0
    for view3, (near, step, mw) in [(None, (d_near, d_step, 1)), (np.array([0.5, 0.07, 3.0]), (0.5, 0.07, 3))]:
        rc = RY.Raycaster(fm.mapper, Wd, Hd, K4, near, step, _n_steps(near, step, 10.0), mw)
        for Tv in (poses[6], turned):
            depth = np.full((Hd, Wd), -7.0, F); nrm = np.full((Hd, Wd, 3), -7.0, F); wgt = np.full((Hd, Wd), -7, np.int32); counts = np.full(3, -7, np.int64)
            Tc = np.ascontiguousarray(Tv.reshape(16))
            assert L.host_dense_render(dd.ctypes.data, mm.ctypes.data, tt.ctypes.data, 7, Wd, Hd, C.byref(prm), anchor.ctypes.data, 2, 1, view3.ctypes.data if view3 is not None else None,
                                       Tc.ctypes.data, depth.ctypes.data, nrm.ctypes.data, wgt.ctypes.data, counts.ctypes.data) == 0
            rd, rg, rw, rcounts = rc.render(Tv)
            _same_bits(depth, rd, "depth"); _same_bits(nrm, RY.normals(rg), "normals"); assert np.array_equal(wgt, rw) and tuple(counts) == tuple(rcounts)
            lens = np.linalg.norm(nrm.astype(np.float64), axis=-1)
            assert ((np.abs(lens - 1) < 1e-6) | (lens == 0)).all()
            hits += rcounts[0]
        rc.close()
    assert hits > 0
    fm.close(); ctx.close()


W, H = synth.KITTI_W, synth.KITTI_H
N_FRAMES = 4
DENSE = dict(VoxelSize=0.25, Size=(96, 32, 160), MaxDepth=30.0, MaxWeight=32, MinWeight=1, Anchor=(0.5, 0.625, 0.05), RecenterMargin=4)
VIEW = {"View.Near": 1.0, "View.Step": 0.4, "View.MinWeight": 1}


def _settings(tmp_path, name, keys):
    from vdo_slam_amd.system import write_settings
    p = write_settings(tmp_path / name, W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    with open(p, "a") as f:
        for k, v in keys.items():
            f.write(f"Dense.{k}: {list(v) if isinstance(v, tuple) else v}\n")
    return p


def _run(settings, frames, each=None):
    from vdo_slam_amd.system import System
    s = System(settings, sensor="rgbd")
    poses = []
    for k, fr in enumerate(frames):
        T = s.track_rgbd(fr["gray"], fr["depth_raw"].copy(), fr["flow"], fr["mask"].copy())
        assert T is not None, k
        poses.append(T)
        if each:
            each(s, k, T)
    return s, np.stack(poses)


def test_system_renders_what_the_python_flow_renders_and_rendering_changes_nothing(tmp_path):
    from vdo_slam_amd import dense as D, raycast as RY
    from vdo_slam_amd.ba import Context
    Ts = SQ.camera_poses(N_FRAMES, step=1.6)
    objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]
    ctx = Context(0)
    fm = D.FollowingMap(ctx, W, H, DENSE["Size"], DENSE["VoxelSize"], synth.KITTI_K, anchor=DENSE["Anchor"], margin=DENSE["RecenterMargin"], min_weight=DENSE["MinWeight"],
                        max_depth=DENSE["MaxDepth"], max_weight=DENSE["MaxWeight"])
    near, step, mw = VIEW["View.Near"], VIEW["View.Step"], VIEW["View.MinWeight"]
    rc = RY.Raycaster(fm.mapper, W, H, synth.KITTI_K, near, step, _n_steps(near, step, DENSE["MaxDepth"]), mw)
    hits = []

    def each(s, k, T):
        depth, mask = s.last_depth_mask(W, H)
        fm.fuse(depth, mask, T)
        got = s.render_dense_view(T)
        assert got is not None
        rd, rg, rw, counts = rc.render(T)
        _same_bits(got[0], rd, f"frame {k}: depth"); _same_bits(got[1], RY.normals(rg), f"frame {k}: normals")
        hits.append(counts[0])

    s, poses = _run(_settings(tmp_path, "view.yaml", {**DENSE, **VIEW}), frames, each)
    assert min(hits) > 1000, hits                                              # the ground and the walls of the scene are seen
    # from another place, after the last frame
    T2 = poses[-1].copy(); T2[0, 3] += 0.8; T2[1, 3] -= 0.3
    got = s.render_dense_view(T2)
    rd, rg, rw, counts = rc.render(T2)
    _same_bits(got[0], rd, "moved: depth"); _same_bits(got[1], RY.normals(rg), "moved: normals")
    s.close(); rc.close(); fm.close(); ctx.close()

    # the same keys without a render call, and no Dense.* keys at all: the same trajectory byte for byte; without a mapper there is no view
    s1, poses1 = _run(_settings(tmp_path, "quiet.yaml", {**DENSE, **VIEW}), frames)
    s1.close()
    seen = []
    s0, poses0 = _run(_settings(tmp_path, "plain.yaml", {}), frames, lambda s, k, T: seen.append(s.render_dense_view(T)))
    assert seen == [None] * N_FRAMES and s0.render_dense_view(np.eye(4)) is None
    s0.close()
    assert np.array_equal(poses1.view(np.uint32), poses.view(np.uint32)) and np.array_equal(poses0.view(np.uint32), poses.view(np.uint32))
