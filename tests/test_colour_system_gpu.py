"""GPU: the colourer through System (settings key Dense.Colour, System::SaveDenseMesh, System::SaveDenseMap, System::RenderDenseColour).  A short
synthetic sequence whose camera moves the volume: the saved mesh has red, green, blue, alpha; its colours equal those the restatement
(tests/colour_ref.py) computes from the same frames and poses - what was kept before a move sampled before that move -; the rendered colour view
equals the restatement's.  Without the key the files keep today's bytes and the trajectory its bits."""
import numpy as np
import pytest

from tests import colour_ref as CR
from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ

pytestmark = pytest.mark.gpu

F = np.float32
W, H = synth.KITTI_W, synth.KITTI_H
DENSE = dict(VoxelSize=0.25, Size=(96, 32, 64), MaxDepth=10.0, MaxWeight=32, MinWeight=1, Anchor=(0.5, 0.625, 0.05), RecenterMargin=4)      # as tests/test_mesh_system_gpu.py
COLOUR = {"Colour": 1, "Colour.Band": 0.5, "Colour.MaxWeight": 16, "Colour.MinWeight": 1}
N_FRAMES = 11      # as there: the volume moves five times, and the later seams cut through surface, so that kept pieces hold vertices


def _settings(tmp_path, name, extra):
    from vdo_slam_amd.system import write_settings
    p = write_settings(tmp_path / name, W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    with open(p, "a") as f:
        for k, v in dict(DENSE, Mesh=1, **extra).items():
            f.write(f"Dense.{k}: {list(v) if isinstance(v, tuple) else v}\n")
    return p


def _colour_image(gray):
    """R = grey + 8, G = grey, B = grey - 21 (clipped): three different channels whose grey conversion is the grey image again wherever nothing
    clips (8 * 4899 - 21 * 1868 = -36 of 16384), so that the tracker sees what it sees in the other tests"""
    g = gray.astype(np.int32)
    return np.ascontiguousarray(np.stack([np.clip(g + 8, 0, 255), g, np.clip(g - 21, 0, 255)], -1).astype(np.uint8))


@pytest.fixture(scope="module")
def frames():
    """the camera 0.8 m forward and 0.6 m towards -x per frame (camera-to-world poses, no rotation)"""
    Ts = []
    for k in range(N_FRAMES + 1):
        T = np.eye(4); T[:3, 3] = [-0.6 * k, 0.0, 0.8 * k]
        Ts.append(T)
    objs = SQ.default_objects()
    out = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(N_FRAMES)]
    for fr in out:
        fr["rgb"] = _colour_image(fr["gray"])
    return out


def _run(settings, frames, each=None):
    from vdo_slam_amd.system import System
    s = System(settings, sensor="rgbd")
    poses = []
    try:
        for k, fr in enumerate(frames):
            T = s.track_rgbd(fr["rgb"], fr["depth_raw"].copy(), fr["flow"], fr["mask"].copy())
            assert T is not None, k
            poses.append(T)
            if each:
                each(s, k, T)
    except BaseException:
        s.close()
        raise
    return s, np.stack(poses)


def test_coloured_mesh_points_and_view(frames, tmp_path):
    from vdo_slam_amd import colour as CL, mesh as MS
    from vdo_slam_amd.ba import Context
    ctx = Context(0)
    fm = CL.FollowingColourMesh(ctx, W, H, DENSE["Size"], DENSE["VoxelSize"], synth.KITTI_K, band=COLOUR["Colour.Band"], colour_max_weight=COLOUR["Colour.MaxWeight"],
                                colour_min_weight=COLOUR["Colour.MinWeight"], anchor=DENSE["Anchor"], margin=DENSE["RecenterMargin"], min_weight=DENSE["MinWeight"],
                                max_depth=DENSE["MaxDepth"], max_weight=DENSE["MaxWeight"])
    Cv = CR.ColourVolume(DENSE["Size"], DENSE["VoxelSize"], (0, 0, 0))
    ref_mesh, ref_pts, origins = [], [], []
    s = None
    try:
        def each(s, k, T):
            depth, mask = s.last_depth_mask(W, H)
            pieces, kept = len(fm.m_xyz), len(fm.xyz)
            fm.fuse(depth, mask, frames[k]["rgb"], T)
            # the restatement: what the flow kept in this call it kept BEFORE the volume moved - the colour volume still stands at the old origin
            for x in fm.m_xyz[pieces:]:
                ref_mesh.append(Cv.sample(x, COLOUR["Colour.MinWeight"]))
            for x in fm.xyz[kept:]:
                ref_pts.append(Cv.sample(x, COLOUR["Colour.MinWeight"]))
            o = fm.mapper.origin()
            if k == 0:
                Cv.clear(o)                                     # the first frame places the empty volume
            counts = Cv.integrate(depth, mask, frames[k]["rgb"], T, synth.KITTI_K, 0.0, DENSE["MaxDepth"], COLOUR["Colour.Band"], COLOUR["Colour.MaxWeight"], 0, 0, map_origin=o)
            assert s.dense_colour_counts() == counts and counts[0] > 0, k
            origins.append(o)
            assert s.dense_info()["origin"] == o

        s, poses = _run(_settings(tmp_path, "colour.yaml", COLOUR), frames, each)
        assert fm.recenters >= 2 and len(ref_mesh) == fm.recenters
        words, origin = fm.colourer.volume()
        assert tuple(origin) == tuple(int(v) for v in Cv.origin) and np.array_equal(words, Cv.words) and (words != 0).sum() > 1000
        # the mesh
        ply = tmp_path / "mesh.ply"
        assert s.save_dense_mesh(ply)
        head = open(ply, "rb").read(600)
        assert b"property int weight\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face" in head
        xyz, nrm, wgt, tri, rgba = CL.read_ply(ply)
        X, N, Wt, T, C = fm.coloured_mesh()
        assert len(X) > 1000 and len(T) > 1000
        assert np.array_equal(xyz.view(np.uint32), X.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), N.view(np.uint32)) and np.array_equal(wgt, Wt) and np.array_equal(tri, T)
        want = np.concatenate(ref_mesh + [Cv.sample(X[fm.m_vertices:], COLOUR["Colour.MinWeight"])])
        assert np.array_equal(rgba, want) and np.array_equal(C, want)
        kept = rgba[:fm.m_vertices]
        print(f"origins {origins}; {len(X)} vertices, {fm.m_vertices} kept before moves, {(rgba[:, 3] > 0).sum()} coloured ({(kept[:, 3] > 0).sum()} of the kept)")
        assert (rgba[:, 3] > 0).mean() > 0.5 and fm.m_vertices > 0 and (kept[:, 3] > 0).sum() > 0      # what left the volume has colour in the file
        col = rgba[rgba[:, 3] == 255].astype(int)
        assert len(col) > 100 and np.all(col[:, 0] >= col[:, 1]) and np.all(col[:, 1] >= col[:, 2]) and np.any(col[:, 0] > col[:, 2])      # R first: Camera.RGB is honoured
        # the points
        pts = tmp_path / "points.ply"
        assert s.save_dense_map(pts)
        pxyz, _, pw, ptri, prgba = CL.read_ply(pts)
        PX, _, PW, PC = fm.coloured_points()
        kept_pts = sum(len(a) for a in fm.xyz)
        want = np.concatenate(ref_pts + [Cv.sample(PX[kept_pts:], COLOUR["Colour.MinWeight"])])
        assert len(ptri) == 0 and np.array_equal(pxyz.view(np.uint32), PX.view(np.uint32)) and np.array_equal(pw, PW) and np.array_equal(prgba, want) and np.array_equal(PC, want)
        # the view
        Tv = poses[-1]
        depth, _ = s.render_dense_view(Tv)
        got = s.render_dense_colour(Tv)
        want, counts = Cv.render(depth, synth.KITTI_K, Tv, COLOUR["Colour.MinWeight"])
        assert got.shape == (H, W, 4) and np.array_equal(got, want) and counts[0] > 1000
        assert not got[depth == 0].any()
    finally:
        if s is not None:
            s.close()
        fm.close(); ctx.close()

    # the same sequence without the key, and with Dense.Colour: 0: today's bytes, the same trajectory
    for name, extra in (("plain.yaml", {}), ("off.yaml", {"Colour": 0, "Colour.Band": 0.5})):
        s0, poses0 = _run(_settings(tmp_path, name, extra), frames)
        try:
            assert np.array_equal(poses0.view(np.uint32), poses.view(np.uint32))
            assert s0.render_dense_colour(poses0[-1]) is None
            ply0, twin = tmp_path / f"mesh_{name}.ply", tmp_path / f"twin_{name}.ply"
            assert s0.save_dense_mesh(ply0)
            x0, n0, w0, t0 = MS.read_ply(ply0)
            MS.write_ply(twin, x0, n0, w0, t0)                  # the format as mesh.py has always written it
            assert open(ply0, "rb").read() == open(twin, "rb").read()
            assert np.array_equal(x0.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(t0, tri)
            pts0 = tmp_path / f"points_{name}.ply"
            assert s0.save_dense_map(pts0)
            raw = open(pts0, "rb").read()
            assert b"red" not in raw[:400] and len(raw) == raw.index(b"end_header\n") + 11 + 28 * len(pxyz)
            p0, _, pw0, _, c0 = CL.read_ply(pts0)
            assert c0 is None and np.array_equal(p0.view(np.uint32), pxyz.view(np.uint32)) and np.array_equal(pw0, pw)
        finally:
            s0.close()


@pytest.mark.parametrize("entry", ["files", "stereo"])
def test_the_entries_that_hand_over_a_device_grey_image(entry, tmp_path):
    """TrackFiles (the grey image the ingest stage decoded on the device) and TrackStereo (the left grey image where the matcher keeps it): three frames
    with Dense.Colour: 1; every frame's counts and the colour view at the end equal the restatement fed the same grey image, the depth and mask
    the frame step left, the pose and the map's origin."""
    from tests import stereo_ref as SR
    from vdo_slam_amd import dataset_files as DF
    from vdo_slam_amd.system import System
    n = 3
    Ts = SQ.camera_poses(n); objs = SQ.default_objects()
    frs = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(n)]
    rows = np.array([[0, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in (1, 2, 3)], np.float32)
    s = System(_settings(tmp_path, f"{entry}.yaml", COLOUR), sensor="stereo" if entry == "stereo" else "rgbd")
    Cv = CR.ColourVolume(DENSE["Size"], DENSE["VoxelSize"], (0, 0, 0))
    try:
        assert s.dense_colour_counts() == (0, 0, 0)
        for k, fr in enumerate(frs):
            if entry == "files":
                paths = DF.write_frame(str(tmp_path / f"{k:06d}"), fr["gray"], np.clip(fr["depth_raw"], 0, 65535).astype(np.uint16), fr["flow"], fr["mask"])
                T = s.track_files(*paths, rows, n_images=n)
            else:
                right = np.random.default_rng(500 + k).integers(0, 256, (H, W)).astype(np.uint8)      # noise under the forward warp of the left image
                SR.warp_right(fr["gray"], np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64), right)
                T = s.track_stereo(fr["gray"], right, fr["flow"], fr["mask"].copy(), rows, n_images=n)
            assert T is not None, k
            depth, mask = s.last_depth_mask(W, H)
            counts = Cv.integrate(depth, mask, fr["gray"], T, synth.KITTI_K, 0.0, DENSE["MaxDepth"], COLOUR["Colour.Band"], COLOUR["Colour.MaxWeight"], 0, 0,
                                  map_origin=s.dense_info()["origin"])
            assert s.dense_colour_counts() == counts and counts[0] > 100, (k, s.dense_colour_counts(), counts)
        depth, _ = s.render_dense_view(T)
        got = s.render_dense_colour(T)
        want, seen = Cv.render(depth, synth.KITTI_K, T, COLOUR["Colour.MinWeight"])
        assert np.array_equal(got, want) and seen[0] > 100
        grey = got[got[..., 3] > 0]
        assert np.all(grey[:, 0] == grey[:, 1]) and np.all(grey[:, 1] == grey[:, 2])      # a grey image: the three channels are one
    finally:
        s.close()


def test_no_colour_view_without_a_mapper(tmp_path):
    from vdo_slam_amd.system import System, write_settings
    s = System(write_settings(tmp_path / "nodense.yaml", W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ), sensor="rgbd")
    try:
        assert s.render_dense_colour(np.eye(4, dtype=F)) is None and s.dense_colour_counts() is None
    finally:
        s.close()
