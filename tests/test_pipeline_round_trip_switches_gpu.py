"""The round-trip switches of FramePipeline (VDO_PIPE_NO_FUSED_STATIC, VDO_PIPE_NO_CHAIN_SPLIT, VDO_PNP_NO_GATE, VDO_ARENA_NO_MAPPED_OUT, VDO_PIPE_NO_MM_OVERLAP): each restores
an older schedule of the same work, none may change a result.  A synchronous pipeline with its helper and ORB threads (the configuration in which every new
path is taken) runs a sequence with two moving objects and a mask that goes missing; all switches off against all on and each alone: poses, motions, every
FrameCounts field of every frame, and the renewed static / object sets with their tracklets (the Map) are equal."""
import numpy as np
import pytest

from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
from vdo_slam_amd.ba import Context
from vdo_slam_amd.pipeline import FramePipeline, kitti_params

pytestmark = pytest.mark.gpu

W, H = synth.KITTI_W, synth.KITTI_H          # (the size every sequence test runs at)
SWITCHES = ("VDO_PIPE_NO_FUSED_STATIC", "VDO_PIPE_NO_CHAIN_SPLIT", "VDO_PNP_NO_GATE", "VDO_ARENA_NO_MAPPED_OUT", "VDO_PIPE_NO_MM_OVERLAP")      # (each is read when a pipeline is built)
N_FRAMES = 7


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


@pytest.fixture(scope="module")
def new_paths(frames):
    import os
    assert not any(s in os.environ for s in SWITCHES)
    return _run(frames)


def _assert_equal(a, b, what):
    pa, ca, ma, mapa = a
    pb, cb, mb, mapb = b
    assert ca == cb, (what, [(x, y) for x, y in zip(ca, cb) if x != y][:1])
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y), what
    for fa, fb in zip(ma, mb):
        assert [q[:3] for q in fa] == [q[:3] for q in fb], what
        for x, y in zip(fa, fb):
            assert np.array_equal(x[3], y[3]), what
    assert mapa["n_frames"] == mapb["n_frames"] == N_FRAMES
    assert np.array_equal(mapa["cam_pose"], mapb["cam_pose"]), what
    for k, (fa, fb) in enumerate(zip(mapa["feats"], mapb["feats"])):          # the renewed static / object sets of every frame
        for q in fa:
            assert np.array_equal(fa[q], fb[q]), (what, k, q)
    assert mapa["tr_sta"] == mapb["tr_sta"] and mapa["tr_dyn"] == mapb["tr_dyn"] and np.array_equal(mapa["obj_of_dyn"], mapb["obj_of_dyn"]), what
    for x, y in zip(mapa["rigid_motion"], mapb["rigid_motion"]):
        assert np.array_equal(x, y), what


def test_the_sequence_does_what_the_switches_are_about(new_paths):
    poses, counts, motions, m = new_paths
    assert all(1 <= c["n_objects"] <= 2 for c in counts[2:]) and max(c["n_objects"] for c in counts) == 2 and 1 <= len(motions[-1]) <= 2
    assert sum(c["n_recovered_masks"] for c in counts) >= 1            # UpdateMask repaired the mask behind the split chain's begin
    assert all(c["n_static_new"] > 500 and c["n_static_tracked"] > 500 for c in counts[1:])
    assert all(c["n_ransac_cam"] > 100 and c["n_cam_inliers"] > 100 for c in counts[2:])
    assert all(f["dyn_uv"].shape[0] > 100 for f in m["feats"])


@pytest.mark.parametrize("on", [SWITCHES] + [(s,) for s in SWITCHES], ids=["all"] + [s for s in SWITCHES])
def test_switches_change_no_result(frames, new_paths, monkeypatch, on):
    for s in on:
        monkeypatch.setenv(s, "1")
    _assert_equal(new_paths, _run(frames), on)
