"""GPU: the photometric term behind System (settings key Dense.Align.Photo; DenseMapper::AlignPhotoFrame, KeepPhotoModel, System::AlignDenseViewPhoto):
the synthetic walk of tests/test_align_system_gpu.py through System::TrackRGBD with the key set, every frame's joint report against
vdo_slam_amd/photo.py + align.py on the Python flow of the same frames and poses - whose trace is walked against the NumPy restatement -; the first
frame is aligned by the geometry alone; with the key absent or 0 the trajectory, the reports and the saved map keep their bytes."""
import gc

import numpy as np
import pytest

from tests import align_ref as A
from tests import photo_ref as P
from tests.test_align_system_gpu import ALIGN, DENSE, N_FRAMES, H, W, Flow, _run, _same_report, _settings
from tests.test_photo_gpu import _walk
from vdo_slam_amd import synth, synth_seq as SQ

pytestmark = pytest.mark.gpu
F = np.float32
WEIGHT = float(F(0.01))                                                         # the settings keep the weight as a float
PHOTO = {"Align.Photo": 0.01, "Align.Photo.MaxDiff": 80, "Align.Photo.MinPixels": 300}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_photo(got, want, what):
    for k in ("iterations", "status", "used_geo", "used_photo", "rms_geo_first", "rms_geo_last", "rms_photo_first", "rms_photo_last"):
        assert got[k] == want[k], (what, k, got, want)
    assert np.array_equal(got["xi"], want["xi"]), (what, got, want)


def _geo_only(rep):
    return dict(iterations=rep["iterations"], status=rep["status"], used_geo=rep["used"], used_photo=0, rms_geo_first=rep["rms_first"], rms_geo_last=rep["rms_last"], rms_photo_first=0.0,
                rms_photo_last=0.0, xi=rep["xi"])


class PhotoFlow(Flow):
    """The Python flow of DenseMapper with Dense.Align.Photo: Flow's map, view and aligner, and the photometric handle DenseMapper::AlignPhoto makes"""

    def __init__(self, ctx, max_diff, photo_min_pixels, *a, **kw):
        super().__init__(ctx, *a, **kw)
        from vdo_slam_amd import photo as PH
        self.max_diff, self.photo_min = max_diff, photo_min_pixels
        self.ph = PH.PhotoAligner(ctx, W, H, self.K4, subsample=self.s, min_pixels=photo_min_pixels, max_iterations=self.iterations, eps=1e-5, max_diff=max_diff, **self.prm)
        self.model = None                                                       # (packed model, its pose) as the restatement keeps it

    def align_photo(self, image, depth, mask, T, what):
        """-> (T_out, joint report) of the device flow: the joint solve walked through its trace against the restatement, or the geometry alone"""
        self.ph.set_image(image)
        I = P.grey(image)
        if self.model is not None:
            self.al.set_model_from_view(self.rc, T)
            Tn, rep, trace = self.ph.solve(self.al, depth, mask, WEIGHT, T)
            Dm, Gm, _, _ = self.rc.render(T)
            model, Tm = self.model
            photo_lin = lambda Tk: P.linearise(depth, mask, I, self.K4, Tk, model, self.K4, Tm, subsample=self.s, max_diff=self.max_diff, **self.prm)
            geo_lin = lambda Tk: A.linearise(depth, mask, self.K4, Tk, Dm, Gm, self.K4, np.asarray(T, F), subsample=self.s, **self.prm)
            _walk(trace, rep, Tn, photo_lin, geo_lin, WEIGHT, self.photo_min, self.min_pixels, self.iterations, 1e-5, what)
            if rep["status"] != 1:
                return Tn, rep
        Tn, rep = self.align(depth, mask, T, what + " (geometry alone)", True)
        return Tn, _geo_only(rep)

    def keep(self, image, depth, mask, T):
        self.ph.keep_as_model(depth, mask, T)
        want = P.keep_as_model(depth, mask, P.grey(image), self.prm["min_depth"], self.prm["max_depth"])
        assert np.array_equal(_bits(self.ph.model()), _bits(want))
        self.model = (want, np.asarray(T, F).copy())

    def close(self):
        self.ph.close()
        super().close()


def test_system_aligns_every_frame_jointly_and_without_the_key_nothing_changes(tmp_path):
    from vdo_slam_amd.ba import Context
    Ts = SQ.camera_poses(N_FRAMES, step=1.6)
    objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]
    assert frames[0]["gray"].dtype == np.uint8 and frames[0]["gray"].shape == (H, W) and frames[0]["gray"].std() > 5      # a textured image
    ctx = Context(0)
    runs = {}
    for apply in (0, 1):
        fl = PhotoFlow(ctx, PHOTO["Align.Photo.MaxDiff"], PHOTO["Align.Photo.MinPixels"], W, H, DENSE["Size"], DENSE["VoxelSize"], synth.KITTI_K, DENSE["Anchor"], DENSE["RecenterMargin"],
                       DENSE["MinWeight"], DENSE["MaxDepth"], ALIGN["Align.Iterations"], ALIGN["Align.Subsample"], ALIGN["Align.MinPixels"], max_weight=DENSE["MaxWeight"])
        reports = []

        def each(s, k, T):
            depth, mask = s.last_depth_mask(W, H)
            got = s.dense_photo_alignment()
            assert got is not None
            want_T, want = fl.align_photo(frames[k]["gray"], depth, mask, T, f"apply {apply}, frame {k}")      # against the map and the model frame of the frames before
            _same_photo(got[0], want, f"apply {apply}, frame {k}")
            fused = want_T if apply and want["status"] == 0 else T
            assert np.array_equal(_bits(got[1]), _bits(fused)), f"apply {apply}, frame {k}: the pose the frame was fused with"
            geo = s.dense_alignment()[0]                                        # the geometric half, where the older accessor looks
            assert (geo["iterations"], geo["status"], geo["used"], geo["rms_first"], geo["rms_last"]) == (want["iterations"], want["status"], want["used_geo"], want["rms_geo_first"],
                                                                                                         want["rms_geo_last"])
            fl.fm.fuse(depth, mask, fused)
            fl.keep(frames[k]["gray"], depth, mask, fused)
            reports.append(want)
            _same_photo(s.last_dense_photo_alignment(), want, f"apply {apply}, frame {k}: LastDensePhotoAlignment after the frame")

        s, poses = _run(_settings(tmp_path, f"photo{apply}.yaml", {**DENSE, **ALIGN, **PHOTO, "Align.Apply": apply}), frames, each)
        # the first frame has no model frame (and meets an empty map): the geometry alone, today's report
        assert reports[0]["status"] == 1 and reports[0]["used_geo"] == 0 and reports[0]["used_photo"] == 0 and reports[0]["iterations"] == 1
        assert all(r["used_photo"] > PHOTO["Align.Photo.MinPixels"] and r["used_geo"] > 0 and r["rms_photo_first"] > 0 for r in reports[1:]), reports
        print(f"apply {apply}:", [(r["status"], r["used_geo"], r["used_photo"], round(r["rms_geo_first"], 4), round(r["rms_geo_last"], 4), round(r["rms_photo_first"], 2),
                                   round(r["rms_photo_last"], 2)) for r in reports])
        # AlignDenseViewPhoto on the last frame at the tracker's pose: the map and the model frame now hold that frame too
        depth, mask = s.last_depth_mask(W, H)
        got_T, got_rep = s.align_dense_view_photo(poses[-1], depth, mask, frames[-1]["gray"])
        want_T, want = fl.align_photo(frames[-1]["gray"], depth, mask, poses[-1], f"apply {apply}, AlignDenseViewPhoto")
        _same_photo(got_rep, want, "AlignDenseViewPhoto"); assert np.array_equal(_bits(got_T), _bits(want_T))
        _same_photo(s.last_dense_photo_alignment(), want, "LastDensePhotoAlignment after AlignDenseViewPhoto")
        assert want["used_photo"] > 0 and want["rms_photo_first"] < reports[-1]["rms_photo_first"]      # the frame against itself
        assert s.save_dense_map(tmp_path / f"photo{apply}.ply")
        runs[apply] = poses
        s.close(); fl.close()
    gc.collect()
    ctx.close()

    # the key absent and the key 0: the same trajectory, reports and saved map, byte for byte; with the key set the tracker's trajectory is still the same
    outs = {}
    for name, keys in (("absent", {}), ("zero", {"Align.Photo": 0, "Align.Photo.MaxDiff": 80})):
        reps = []
        s, poses = _run(_settings(tmp_path, f"{name}.yaml", {**DENSE, **ALIGN, **keys, "Align.Apply": 1}), frames, lambda s, k, T: reps.append((s.dense_alignment(), s.dense_photo_alignment())))
        assert all(p is None for _, p in reps) and s.last_dense_photo_alignment() is None
        assert s.align_dense_view_photo(poses[-1], *s.last_depth_mask(W, H), frames[-1]["gray"]) is None
        assert s.save_dense_map(tmp_path / f"{name}.ply")
        outs[name] = (poses, [a for a, _ in reps], s.dense_info())
        s.close()
    assert np.array_equal(outs["absent"][0].view(np.uint32), outs["zero"][0].view(np.uint32)) and outs["absent"][2] == outs["zero"][2]
    for (ra, fa), (rz, fz) in zip(outs["absent"][1], outs["zero"][1]):
        _same_report(ra, rz, "absent against 0"); assert np.array_equal(_bits(fa), _bits(fz))
    assert (tmp_path / "absent.ply").read_bytes() == (tmp_path / "zero.ply").read_bytes()
    for apply in (0, 1):
        assert np.array_equal(runs[apply].view(np.uint32), outs["absent"][0].view(np.uint32))
