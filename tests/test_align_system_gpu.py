"""GPU: the aligner behind the host class and System (DenseMapper::Align, System::AlignDenseView, settings keys Dense.Align.*): the host class on host
frames through host_dense_align, and a short synthetic sequence through System::TrackRGBD, both against vdo_slam_amd/align.py on the Python flow
(dense.FollowingMap) of the same frames and against the NumPy restatement; the tracker's trajectory is the same bytes with and without the keys."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import align_ref as A
from tests.test_align_gpu import _walk
from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ

pytestmark = pytest.mark.gpu
F = np.float32


def _n_steps(near, step, max_depth):
    """ceil((MaxDepth - Near) / Step) + 1 in double on the float32 values, as DenseMapper::CheckView"""
    return int(np.ceil((float(F(max_depth)) - float(F(near))) / float(F(step)))) + 1


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_report(got, want, what):
    assert (got["iterations"], got["status"], got["used"]) == (want["iterations"], want["status"], want["used"]), (what, got, want)
    assert got["rms_first"] == want["rms_first"] and got["rms_last"] == want["rms_last"] and np.array_equal(got["xi"], want["xi"]), (what, got, want)


class Flow:
    """The Python flow of DenseMapper: a FollowingMap, its view with DenseMapper::ViewDefaults, and the aligner DenseMapper::Align makes"""

    def __init__(self, ctx, W, H, n, voxel, K4, anchor, margin, min_weight, max_depth, iterations, subsample, min_pixels, view=None, **prm):
        from vdo_slam_amd import align as AL, dense as D, raycast as RY
        self.fm = D.FollowingMap(ctx, W, H, n, voxel, K4, anchor=anchor, margin=margin, min_weight=min_weight, max_depth=max_depth, **prm)
        trunc = float(F(4.0) * F(voxel))
        near, step, mw = view or (float(max(F(0.0), F(voxel))), float(F(trunc) / F(2)), min_weight)
        self.rc = RY.Raycaster(self.fm.mapper, W, H, K4, near, step, _n_steps(near, step, max_depth), mw)
        self.prm = dict(min_depth=0.0, max_depth=max_depth, max_dist=trunc)
        self.K4, self.s, self.min_pixels, self.iterations = K4, subsample, min_pixels, iterations
        self.al = AL.Aligner(ctx, W, H, K4, subsample=subsample, min_pixels=min_pixels, max_iterations=iterations, eps=1e-5, **self.prm)

    def align(self, depth, mask, T, what, equilibrated=False):
        """-> (T_out, report) of the device flow, after walking its trace against the restatement"""
        self.al.set_model_from_view(self.rc, T)
        Tn, rep, trace = self.al.solve(depth, mask, T)
        Dm, Gm, _, _ = self.rc.render(T)
        _walk(trace, rep, Tn, depth, mask, self.K4, Dm, Gm, self.K4, np.asarray(T, F), self.prm, self.s, self.min_pixels, self.iterations, 1e-5, what, equilibrated)
        return Tn, rep

    def close(self):
        self.al.close(); self.rc.close(); self.fm.close()


def test_the_host_class_aligns_what_the_python_flow_aligns_and_changes_nothing_of_the_map():
    from vdo_slam_amd import _capi as K, dense as D
    from vdo_slam_amd.ba import Context
    c = A.CORNER
    Wd, Hd, K4, n, voxel = c["W"], c["H"], c["K4"], c["n"], c["voxel"]
    poses = [A.look_at(eye, target) for eye, target in A.CORNER_POSES]
    depths = [A.plane_depth(c["planes"], T, Wd, Hd, K4) for T in poses]
    masks = [np.zeros((Hd, Wd), np.int32) for _ in poses]
    masks[1][:, :5] = 3
    _, T_true = A.corner_volume()
    frame = A.plane_depth(c["planes"], T_true, Wd, Hd, K4)
    fmask = np.zeros((Hd, Wd), np.int32); fmask[40:, 50:] = 1
    L = K.load_host_lib()
    L.host_dense_align.restype = C.c_int
    L.host_dense_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    prm = D.params(n, voxel, K4, max_depth=c["max_depth"], stage_points=1000)
    anchor = np.array([0.45, 0.45, 0.1])
    dd, mm, tt = np.stack(depths), np.stack(masks), np.stack(poses)
    ctx = Context(0)
    used_any = 0
    for align5, (iters, sub, min_px) in [(np.array([0.0, 0.0, 1.0, 0.0, 0.0]), (10, 1, Wd * Hd // 16)), (np.array([3.0, 0.0, 2.0, 50.0, 0.0]), (3, 2, 50))]:
        fl = Flow(ctx, Wd, Hd, n, voxel, K4, anchor, 100, 1, c["max_depth"], iters, sub, min_px)
        for k in range(len(poses)):
            fl.fm.fuse(depths[k], masks[k], poses[k])
        before = fl.fm.mapper.volume()[0]
        for pert in (0, 3):
            T_init = A.perturbed(T_true, *A.PERTURBATIONS[pert])
            want_T, want = fl.align(frame, fmask, T_init, f"flow, perturbation {pert}")
            T_out = np.full(16, -7.0, F); rep = np.full(11, -7.0); words = np.zeros(before.shape, np.uint32)
            assert L.host_dense_align(dd.ctypes.data, mm.ctypes.data, tt.ctypes.data, len(poses), Wd, Hd, C.byref(prm), anchor.ctypes.data, 100, 1, align5.ctypes.data, frame.ctypes.data,
                                      fmask.ctypes.data, np.ascontiguousarray(T_init.reshape(16)).ctypes.data, T_out.ctypes.data, rep.ctypes.data, words.ctypes.data) == 0
            got = dict(iterations=int(rep[0]), status=int(rep[1]), used=int(rep[2]), rms_first=rep[3], rms_last=rep[4], xi=rep[5:11])
            _same_report(got, want, f"host class, perturbation {pert}")
            assert np.array_equal(_bits(T_out.reshape(4, 4)), _bits(want_T))
            assert np.array_equal(words, before) and np.array_equal(fl.fm.mapper.volume()[0], before)      # nothing of the map changes
            assert got["status"] == 0 and got["rms_last"] < got["rms_first"]
            dt, dr = A.pose_error(T_out.reshape(4, 4), T_true)
            assert dt < 0.025 and dr < 1.0, (dt, dr)                         # below half the perturbation
            used_any += got["used"]
        fl.close()
    assert used_any > 0
    gc.collect()
    ctx.close()


W, H = synth.KITTI_W, synth.KITTI_H
N_FRAMES = 4
DENSE = dict(VoxelSize=0.25, Size=(96, 32, 160), MaxDepth=30.0, MaxWeight=32, MinWeight=1, Anchor=(0.5, 0.625, 0.05), RecenterMargin=4)
ALIGN = {"Align.Iterations": 2, "Align.Subsample": 4, "Align.MinPixels": 200}


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
    try:
        for k, fr in enumerate(frames):
            T = s.track_rgbd(fr["gray"], fr["depth_raw"].copy(), fr["flow"], fr["mask"].copy())
            assert T is not None, k
            poses.append(T)
            if each:
                each(s, k, T)
    except BaseException:
        s.close()                                                               # a failing check must not leave a System behind for the tests after it
        raise
    return s, np.stack(poses)


def test_system_aligns_every_frame_and_the_tracker_sees_nothing_of_it(tmp_path):
    from vdo_slam_amd.ba import Context
    Ts = SQ.camera_poses(N_FRAMES, step=1.6)
    objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]
    ctx = Context(0)
    runs = {}
    for apply in (0, 1):
        fl = Flow(ctx, W, H, DENSE["Size"], DENSE["VoxelSize"], synth.KITTI_K, DENSE["Anchor"], DENSE["RecenterMargin"], DENSE["MinWeight"], DENSE["MaxDepth"],
                  ALIGN["Align.Iterations"], ALIGN["Align.Subsample"], ALIGN["Align.MinPixels"], max_weight=DENSE["MaxWeight"])
        reports, between = [], []

        def each(s, k, T):
            depth, mask = s.last_depth_mask(W, H)
            got = s.dense_alignment()
            assert got is not None
            want_T, want = fl.align(depth, mask, T, f"apply {apply}, frame {k}", True)          # against the map of the frames before this one
            _same_report(got[0], want, f"apply {apply}, frame {k}")
            fused = want_T if apply and want["status"] == 0 else T
            assert np.array_equal(_bits(got[1]), _bits(fused)), f"apply {apply}, frame {k}: the pose the frame was fused with"
            fl.fm.fuse(depth, mask, fused)
            reports.append(want)
            # System::LastDenseAlignment: the frame's report, then AlignDenseView's, then the NEXT frame's - whichever came later
            _same_report(s.last_dense_alignment(), want, f"apply {apply}, frame {k}: LastDenseAlignment after the frame")
            if k == 1:
                between.append(s.align_dense_view(T, depth, mask)[1])
                _same_report(s.last_dense_alignment(), between[0], "LastDenseAlignment after AlignDenseView")
                assert between[0]["rms_first"] != want["rms_first"]             # (the map holds the frame now: another report)

        s, poses = _run(_settings(tmp_path, f"apply{apply}.yaml", {**DENSE, **ALIGN, "Align.Apply": apply}), frames, each)
        assert reports[0]["status"] == 1 and reports[0]["used"] == 0 and reports[0]["iterations"] == 1      # the first frame meets an empty map
        assert all(r["used"] > 0 for r in reports[1:]), reports
        print(f"apply {apply}:", [(r["status"], r["used"], round(r["rms_first"], 4), round(r["rms_last"], 4)) for r in reports])
        # AlignDenseView on the last frame at the tracker's pose: the map now holds that frame too
        depth, mask = s.last_depth_mask(W, H)
        got_T, got_rep = s.align_dense_view(poses[-1], depth, mask)
        want_T, want = fl.align(depth, mask, poses[-1], f"apply {apply}, AlignDenseView", True)
        _same_report(got_rep, want, "AlignDenseView"); assert np.array_equal(_bits(got_T), _bits(want_T))
        assert s.save_dense_map(tmp_path / f"apply{apply}.ply")
        runs[apply] = (poses, s.dense_info())
        s.close(); fl.close()
    gc.collect()
    ctx.close()

    # without the alignment keys, and without a mapper: the same trajectory byte for byte; Apply 0 leaves the same map; without a mapper no alignment
    s2, poses2 = _run(_settings(tmp_path, "dense.yaml", DENSE), frames)
    assert s2.dense_alignment() is None and s2.save_dense_map(tmp_path / "dense.ply")
    info2 = s2.dense_info()
    s2.close()
    seen = []
    s0, poses0 = _run(_settings(tmp_path, "plain.yaml", {}), frames, lambda s, k, T: seen.append(s.dense_alignment()))
    assert seen == [None] * N_FRAMES and s0.align_dense_view(np.eye(4), np.ones((H, W), F)) is None
    s0.close()
    for other in (runs[1][0], poses2, poses0):
        assert np.array_equal(other.view(np.uint32), runs[0][0].view(np.uint32))
    assert (tmp_path / "apply0.ply").read_bytes() == (tmp_path / "dense.ply").read_bytes() and runs[0][1] == info2
