"""K9 (k_static_filter) on the ORB thread.  Once a last frame exists only a count comes of K9 (FrameCounts.n_static_new): by default it joins K10 on the ORB
thread, behind UpdateMask, and the static stage sends the renewal alone; VDO_PIPE_K9_IN_STATIC=1 keeps it in the static stage.  A synchronous pipeline with its
helper and ORB threads runs eight frames - the first one (no last frame: K9 feeds Initialization on the main thread) and two whose instance mask is missing, so
that UpdateMask repairs the mask K9 reads - at the size every sequence test runs at (the scene of the sequence helpers is laid out for that camera).  Every
FrameCounts field of every frame, every pose, the motions and the stored trajectory are equal between the two schedules."""
import os

import numpy as np
import pytest

from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
from vdo_slam_amd.ba import Context
from vdo_slam_amd.pipeline import FramePipeline, kitti_params

pytestmark = pytest.mark.gpu

W, H = synth.KITTI_W, synth.KITTI_H
N_FRAMES = 8
SWITCH = "VDO_PIPE_K9_IN_STATIC"          # (read when a pipeline is built)


@pytest.fixture(scope="module")
def frames():
    import torch
    Ts = SQ.camera_poses(N_FRAMES)
    objs = SQ.default_objects()[:2]
    fr = [SQ.render_frame(k, Ts, objs, flow_sigma=0.05, drop_masks={3: {1}, 4: {1}}) for k in range(N_FRAMES)]
    dev = [{q: torch.from_numpy(np.ascontiguousarray(f[q])).cuda() for q in ("gray", "depth_raw", "flow", "mask")} for f in fr]
    torch.cuda.synchronize()
    return dev


def _run(dev):
    ctxs = [Context(0) for _ in range(5)]
    pipe = FramePipeline(ctxs[0], ctxs[1], kitti_params(W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ, build_lm=1, defer_objects=0), ctxs[2], ctxs[3], ctxs[4])
    pipe.attach_map()
    poses, counts, motions = [], [], []
    for d in dev:
        counts.append(dict(pipe.step(d["gray"].data_ptr(), d["depth_raw"].data_ptr(), d["flow"].data_ptr(), d["mask"].data_ptr())))
        poses.append(pipe.pose().copy())
        motions.append([(m["mod_label"], m["sem_label"], m["n_inliers"], m["H"].copy()) for m in pipe.motions()])
    pipe.finalize_map()
    m = pipe.export_map(synth.KITTI_K)
    pipe.close()
    return poses, counts, motions, m


def test_k9_on_the_orb_thread_changes_no_result(frames, monkeypatch):
    assert SWITCH not in os.environ
    pa, ca, ma, mapa = _run(frames)
    monkeypatch.setenv(SWITCH, "1")
    pb, cb, mb, mapb = _run(frames)
    # the sequence reaches what the move is about: K9 with and without a last frame, and behind a repaired mask
    assert all(c["n_static_new"] > 500 for c in ca) and sum(c["n_recovered_masks"] for c in ca) >= 1
    assert all(c["n_object_samples"] > 100 for c in ca)
    for k, (x, y) in enumerate(zip(ca, cb)):
        assert x == y, (k, {q: (x[q], y[q]) for q in x if x[q] != y[q]})
    for k, (x, y) in enumerate(zip(pa, pb)):
        assert np.array_equal(x, y), f"pose of frame {k}"
    for k, (fa, fb) in enumerate(zip(ma, mb)):
        assert [q[:3] for q in fa] == [q[:3] for q in fb], f"motions of frame {k}"
        for x, y in zip(fa, fb):
            assert np.array_equal(x[3], y[3]), f"motion matrices of frame {k}"
    assert mapa["n_frames"] == mapb["n_frames"] == N_FRAMES
    assert np.array_equal(mapa["cam_pose"], mapb["cam_pose"])
    for x, y in zip(mapa["rigid_motion"], mapb["rigid_motion"]):
        assert np.array_equal(x, y)
