"""GPU: the device object stage (vdo_objects_*, csrc/objects.hip) against the NumPy restatement of its contract (tests/objects_ref.py) and against
vdo_dense_integrate on twin maps.  Every comparison is array_equal: the int64 statistics, the words of every volume and the counts."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_ref as R
from tests import objects_ref as OR

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _stage(ctx, W, H, K4, **kw):
    from vdo_slam_amd.objects import ObjectStage
    return ObjectStage(ctx, W, H, K4, **kw)


# ---- statistics --------------------------------------------------------------------------------------------------------------------------------
K_STATS = (61.5, 58.25, 33.3, 4.6)


def _check_stats(st, depth, mask, prm, what):
    want = OR.stats(depth, mask, K_STATS, *prm)
    got = st.stats(depth, mask)
    assert got.dtype == np.int64 and np.array_equal(got, want), f"{what}: rows {np.nonzero((got != want).any(1))[0][:8]} differ"
    assert np.array_equal(st.last_stats(), want), what
    return want


def test_stats_of_a_partial_wave_image_with_every_kind_of_pixel(ctx):
    W, H, ML = 70, 9, 6                                                      # 630 pixels: two full workgroups of 256 and a partial wave
    rng = np.random.default_rng(1)
    depth = rng.uniform(0.6, 7.9, (H, W)).astype(F)
    mask = rng.choice(np.array([0, 0, 1, 2, ML, ML + 1, -1, -5], np.int32), (H, W)).astype(np.int32)
    mask[mask == 3] = 0; mask[mask == 4] = 0
    mask[0, :] = 3; mask[H - 1, :] = 3; mask[:, 0] = 3; mask[:, W - 1] = 3   # a label that touches all four borders
    mask[4, 37] = 4                                                          # a one-pixel label
    up = F(np.nextafter(F(8.0), F(np.inf)))
    for k, v in enumerate([np.nan, np.inf, -np.inf, 0.0, -1.0, 8.0, up, 0.5, float(np.nextafter(F(0.5), F(1))), 20.0]):
        depth[2, 3 + 2 * k] = v; mask[2, 3 + 2 * k] = 1 + k % 2
        depth[6, 3 + 2 * k] = v; mask[6, 3 + 2 * k] = ML + 1 + k % 2
    depth[0, 0] = 8.0; depth[H - 1, W - 1] = 1.0; depth[0, W - 1] = 2.0; depth[H - 1, 0] = 3.0
    st = _stage(ctx, W, H, K_STATS, min_depth=0.5, max_depth=8.0, max_labels=ML, max_batch=1)
    want = _check_stats(st, depth, mask, (0.5, 8.0, ML), "mixed")
    assert want[0, 0] > 0 and (want[[1, 2, 3, 4, 6], 0] > 0).all() and want[5, 0] == 0 and want[4].tolist()[:5] == [1, 37, 4, 37, 4] and want[3].tolist()[1:5] == [0, 0, W - 1, H - 1]
    assert np.array_equal(st.stats(depth, mask), want), "second run"
    one = np.full((H, W), 5, np.int32)
    w1 = _check_stats(st, depth, one, (0.5, 8.0, ML), "every pixel one label")
    assert w1[5, 0] > 600 and (w1[[1, 2, 3, 4, 6], 0] == 0).all()
    w0 = _check_stats(st, depth, np.zeros((H, W), np.int32), (0.5, 8.0, ML), "no label")
    assert not w0[:, 0].any() and (w0[:, 1] == W).all() and (w0[:, 4] == -1).all()
    st.close()


def test_stats_of_1023_labels_and_strided_host_and_device_sources(ctx):
    import torch
    W, H, ML = 64, 16, 1023
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.2, 30.0, (H, W)).astype(F)
    mask = rng.permutation(W * H).astype(np.int32).reshape(H, W)             # 0..1023: every label once, every lane of a wave another one
    st = _stage(ctx, W, H, K_STATS, min_depth=0.0, max_depth=25.0, max_labels=ML, max_batch=1)
    want = _check_stats(st, depth, mask, (0.0, 25.0, ML), "1023 labels")
    assert (want[1:, 0] <= 1).all() and want[1:, 0].sum() > 700
    wide_d = np.full((H, W + 5), 1.0, F); wide_d[:, :W] = depth
    wide_m = np.full((H, W + 3), 9, np.int32); wide_m[:, :W] = mask
    assert np.array_equal(st.stats(wide_d[:, :W], wide_m[:, :W]), want), "strided host"
    td, tm, twd, twm = (torch.from_numpy(a).cuda() for a in (depth, mask, wide_d, wide_m))
    torch.cuda.synchronize()
    assert np.array_equal(st.stats_raw(td.data_ptr(), W, tm.data_ptr(), W, True), want), "packed device"
    assert np.array_equal(st.stats_raw(twd.data_ptr(), W + 5, twm.data_ptr(), W + 3, True), want), "strided device"
    wall, dev = st.timing()
    assert wall > 0 and dev >= 0
    st.close()


# ---- fusion ------------------------------------------------------------------------------------------------------------------------------------
W, H, K4 = 96, 48, (60.0, 55.0, 47.75, 24.1)
PRM = dict(min_depth=0.0, max_depth=10.0)


def _pose(n, origin, voxel, at, yaw=0.0, pitch=0.0):
    """T (object frame -> camera) that puts the volume's centre at the camera point `at`, turned by yaw (about y) and pitch (about x)"""
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rm = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    centre = (np.array(origin) + 0.5 * np.array(n)) * voxel
    T = np.eye(4); T[:3, :3] = Rm; T[:3, 3] = np.array(at) - Rm @ centre
    return T.astype(F)


def _images(seed, n_labels=3):
    """A slanted surface around 3 m with noise and holes; the mask in vertical stripes of labels 0..n_labels with salt of other values"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    depth = (3.0 + 0.5 * (xs / (W - 1) - 0.5) + rng.normal(0, 0.03, (H, W))).astype(F)
    holes = rng.random((H, W))
    depth[holes < 0.03] = 0; depth[(holes >= 0.03) & (holes < 0.05)] = np.nan; depth[(holes >= 0.05) & (holes < 0.06)] = np.inf; depth[(holes >= 0.06) & (holes < 0.07)] = 11.0
    mask = ((xs // 14) % (n_labels + 1)).astype(np.int32)
    salt = rng.random((H, W))
    mask[salt < 0.03] = -2; mask[(salt >= 0.03) & (salt < 0.06)] = 1; mask[(salt >= 0.06) & (salt < 0.08)] = 900
    return depth, mask


class Obj:
    """A device map, its restatement and a twin device map for vdo_dense_integrate, kept in step"""

    def __init__(self, ctx, n, voxel, origin, label, T, max_weight=64, trunc=None, max_depth=10.0):
        from vdo_slam_amd.dense import DenseMapper
        trunc = 4.0 * float(F(voxel)) if trunc is None else trunc
        kw = dict(origin=origin, trunc=trunc, min_depth=0.0, max_depth=max_depth, max_weight=max_weight, stage_points=4096)
        self.m = DenseMapper(ctx, W, H, n, voxel, K4, **kw)
        self.twin = DenseMapper(ctx, W, H, n, voxel, K4, **kw)
        self.V = R.Volume(n, voxel, origin)
        self.label, self.T, self.prm = label, T, (trunc, 0.0, max_depth, max_weight)

    def seed(self, rng):
        t = rng.integers(-3000, 3000, self.V.words.shape).astype(np.int16)
        w = rng.integers(0, 3, self.V.words.shape).astype(np.uint32)
        words = np.where(w > 0, (w << 16) | t.view(np.uint16).astype(np.uint32), 0).astype(np.uint32)
        self.m.set_volume(words); self.twin.set_volume(words); self.V.words = words.copy()

    def close(self):
        self.m.close(); self.twin.close()


def _fuse_and_check(st, objs, depth, mask, what):
    """One batched call; every volume and count against the restatement and against vdo_dense_integrate with the mask image (mask != label)"""
    stats = OR.stats(depth, mask, K4, 0.0, 10.0, st.max_labels)
    out = st.integrate(depth, mask, [o.m for o in objs], [o.label for o in objs], [o.T for o in objs])
    assert np.array_equal(st.last_stats(), stats), what
    for i, o in enumerate(objs):
        upd, occ = OR.integrate(o.V, depth, mask, o.label, o.T, K4, *o.prm)
        assert out[i].tolist() == [upd, occ, int(stats[o.label, 0])], f"{what}: object {i} counts {out[i].tolist()} against {(upd, occ, int(stats[o.label, 0]))}"
        words, _ = o.m.volume()
        assert np.array_equal(words, o.V.words), f"{what}: object {i}: {int((words != o.V.words).sum())} words differ from the restatement"
        tu, _, to = o.twin.integrate(depth, (mask != o.label).astype(np.int32), o.T)
        assert (tu, to) == (upd, occ) and np.array_equal(o.twin.volume()[0], words), f"{what}: object {i} differs from vdo_dense_integrate on its twin"
    return out


@pytest.mark.parametrize("cull", [1, 0])
def test_a_mixed_batch_against_the_restatement_and_the_dense_mapper(ctx, cull):
    depth, mask = _images(5)
    st = _stage(ctx, W, H, K4, max_labels=1000, max_batch=8, **PRM)
    st.set_cull(cull)
    rng = np.random.default_rng(9)
    objs = [Obj(ctx, (20, 12, 9), 0.1, (-10, -6, -4), 1, _pose((20, 12, 9), (-10, -6, -4), 0.1, (-0.9, 0.1, 3.0), yaw=0.2, pitch=-0.15), max_weight=3),
            Obj(ctx, (70, 5, 6), 0.04, (3, -2, 7), 2, _pose((70, 5, 6), (3, -2, 7), 0.04, (0.3, -0.2, 3.05), yaw=-0.1, pitch=0.05)),
            Obj(ctx, (9, 9, 9), 0.08, (0, 0, 0), 3, _pose((9, 9, 9), (0, 0, 0), 0.08, (0.05, 0.0, 3.2))),                      # overlaps the next one in space
            Obj(ctx, (11, 8, 9), 0.08, (-1, -1, 0), 1, _pose((11, 8, 9), (-1, -1, 0), 0.08, (-0.3, 0.05, 3.2), yaw=0.05)),     # label 1 a second time: its salt pixels
            Obj(ctx, (6, 5, 4), 0.1, (0, 0, 0), 7, _pose((6, 5, 4), (0, 0, 0), 0.1, (0.0, 0.0, 3.0))),                         # a label absent from the frame
            Obj(ctx, (65, 2, 5), 0.05, (-70, 0, 0), 900, _pose((65, 2, 5), (-70, 0, 0), 0.05, (0.0, 0.4, 3.0)))]              # a label of salt pixels only
    objs[4].seed(rng)
    before = objs[4].V.words.copy()
    for k in range(5):                                                       # object 0 reaches its weight cap of 3
        out = _fuse_and_check(st, objs, depth, mask, f"cull {cull}, pass {k}")
    assert out[0][0] > 0 and out[1][0] > 0 and out[2][0] > 0 and out[3][0] > 0 and out[5][0] > 0 and out[:, 1].sum() > 0
    assert out[4].tolist() == [0, 0, 0] and np.array_equal(objs[4].m.volume()[0], before)                                      # untouched bit for bit
    assert int(objs[0].V.w().max()) == 3
    depth2, mask2 = _images(6)
    _fuse_and_check(st, objs[1:2], depth2, mask2, f"cull {cull}, a batch of 1")
    _fuse_and_check(st, [], depth2, mask2, f"cull {cull}, an empty batch")
    wall, dev = st.timing()
    assert wall > 0 and dev >= 0
    for o in objs:
        o.close()
    st.close()


def test_integrate_of_strided_host_and_device_sources(ctx):
    """vdo_objects_integrate brings its images to the device as vdo_objects_stats does: host rows with a stride, device rows with a stride and packed
    device images (read where they lie) give the words and the counts of the packed host call, bit for bit"""
    import torch
    from vdo_slam_amd.dense import DenseMapper
    w, h, k4, n = 13, 7, (10.0, 9.0, 6.2, 3.1), (6, 5, 4)
    rng = np.random.default_rng(3)
    depth = rng.uniform(0.8, 1.2, (h, w)).astype(F); depth[2, 6] = np.nan
    mask = np.repeat((np.arange(w) // 4).astype(np.int32)[None, :], h, 0)    # stripes of the labels 0 .. 3; the volumes see the columns 3 .. 9
    wide_d = np.full((h, 16), 1.0, F); wide_d[:, :w] = depth
    wide_m = np.full((h, 16), 1, np.int32); wide_m[:, :w] = mask
    T = np.stack([np.eye(4, dtype=F)] * 2)
    st = _stage(ctx, w, h, k4, max_labels=4, max_batch=2, **PRM)

    def run(call):
        maps = [DenseMapper(ctx, w, h, n, 0.1, k4, origin=(-3, -2, 8), min_depth=0.0, max_depth=10.0, stage_points=64) for _ in range(2)]
        out = call(maps)
        words = [m.volume()[0] for m in maps]
        for m in maps:
            m.close()
        return out, words

    want_out, want_words = run(lambda maps: st.integrate(depth, mask, maps, [1, 2], T))
    assert (want_out[:, 0] > 0).all() and all(wd.any() for wd in want_words)
    td, tm, twd, twm = (torch.from_numpy(a).cuda() for a in (depth, mask, wide_d, wide_m))
    torch.cuda.synchronize()
    for what, call in [("strided host", lambda maps: st.integrate(wide_d[:, :w], wide_m[:, :w], maps, [1, 2], T)),
                       ("strided device", lambda maps: st.integrate_raw(twd.data_ptr(), 16, twm.data_ptr(), 16, True, maps, [1, 2], T)),
                       ("packed device", lambda maps: st.integrate_raw(td.data_ptr(), w, tm.data_ptr(), w, True, maps, [1, 2], T))]:
        out, words = run(call)
        assert np.array_equal(out, want_out) and all(np.array_equal(a, b) for a, b in zip(words, want_words)), what
    st.close()


@pytest.mark.parametrize("cull", [1, 0])
def test_a_batch_of_max_batch(ctx, cull):
    depth, mask = _images(7, n_labels=5)
    st = _stage(ctx, W, H, K4, max_labels=1000, max_batch=64, **PRM)
    st.set_cull(cull)
    objs = []
    for i in range(64):
        n = (5 + i % 4, 3 + i % 3, 4 + i % 2)
        X = -1.8 + 0.055 * i
        label = (int(K4[0] * X / 3.0 + K4[2]) // 14) % 6 if i % 4 else 6      # the stripe under the volume's centre (0: background); every fourth an absent label
        objs.append(Obj(ctx, n, 0.1, (-2, -1, 0), max(label, 1), _pose(n, (-2, -1, 0), 0.1, (X, -0.5 + 0.1 * (i % 9), 3.0), yaw=0.01 * i)))
    out = _fuse_and_check(st, objs, depth, mask, f"cull {cull}, 64 objects")
    assert (out[:, 0] > 0).sum() >= 32 and (out[::4, 2] == 0).all()
    for o in objs:
        o.close()
    st.close()


@pytest.mark.parametrize("cull", [1, 0])
def test_a_voxel_whose_pixel_is_exactly_a_box_edge(ctx, cull):
    """A 1-voxel volume (centre 0.25 m, voxel 0.5) whose pixel walks over a 6 x 5 image with f = 2; the label's box is x 2..3, y 1..3"""
    from vdo_slam_amd.dense import DenseMapper
    from vdo_slam_amd.objects import ObjectStage
    Wd, Hd, Kd = 6, 5, (2.0, 2.0, 0.0, 0.0)
    depth = (np.arange(Wd * Hd, dtype=F).reshape(Hd, Wd) * F(0.01) + F(2.0)).astype(F)
    mask = np.zeros((Hd, Wd), np.int32); mask[1:4, 2:4] = 4
    st = ObjectStage(ctx, Wd, Hd, Kd, min_depth=0.0, max_depth=10.0, max_labels=4, max_batch=1)
    st.set_cull(cull)
    assert OR.stats(depth, mask, Kd, 0.0, 10.0, 4)[4].tolist()[:5] == [6, 2, 1, 3, 3]
    m = DenseMapper(ctx, Wd, Hd, (1, 1, 1), 0.5, Kd, trunc=0.5, max_depth=10.0, max_weight=255, stage_points=16)
    V = R.Volume((1, 1, 1), 0.5)
    hits = 0
    for ux in range(Wd):
        for vy in range(Hd):
            T = np.eye(4, dtype=F); T[0, 3] = -0.25 + ux; T[1, 3] = -0.25 + vy; T[2, 3] = 1.75       # u = X, v = Y at Zc = 2
            out = st.integrate(depth, mask, [m], [4], [T])
            upd, occ = OR.integrate(V, depth, mask, 4, T, Kd, 0.5, 0.0, 10.0, 255)
            assert out[0].tolist() == [upd, occ, 6] and np.array_equal(m.volume()[0], V.words), (ux, vy)
            assert upd == int(2 <= ux <= 3 and 1 <= vy <= 3), (ux, vy)
            hits += upd
    assert hits == 6
    m.close(); st.close()


# ---- the readers on an object volume, and the lifecycle over the C ABI ---------------------------------------------------------------------------
def test_the_lifecycle_and_the_readers_on_an_object_volume(ctx, tmp_path):
    """objects.py's ObjectMaps against the restatement's RefMaps on hand-made frames (48 x 32 images, a 24^3 volume, a label that walks and then
    disappears); vdo_dense_extract and vdo_raycast_render on the fused object volume against dense_ref / raycast_ref at T = Tcw * Two"""
    from tests import raycast_ref as RR
    from vdo_slam_amd.objects import ObjectMaps
    from vdo_slam_amd.raycast import Raycaster
    Wd, Hd, Kd = 48, 32, (40.0, 40.0, 23.5, 15.5)
    prm = dict(size=(24, 24, 24), max_depth=10.0, min_pixels=20, min_frames=2, min_weight=1, max_labels=7)
    dev = ObjectMaps(ctx, Wd, Hd, Kd, 0.05, max_objects=2, stage_points=512, **prm)
    ref = OR.RefMaps(Wd, Hd, Kd, 0.05, max_objects=2, **prm)
    Tcw = np.eye(4); a = 0.1
    Tcw[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]; Tcw[:3, 3] = [0.05, -0.02, 0.1]
    ys, xs = np.mgrid[0:Hd, 0:Wd]

    def frame(k, gone=False):
        depth = np.full((Hd, Wd), 4.0, F); mask = np.zeros((Hd, Wd), np.int32)
        if not gone:
            sel = (xs >= 10 + 2 * k) & (xs < 24 + 2 * k) & (ys >= 8) & (ys < 22)
            depth[sel] = (2.0 + 0.01 * (xs - 17 - 2 * k))[sel]; mask[sel] = 3                # a slanted face that walks 2 pixels (0.1 m) a frame
        mask[2:6, 40:46] = 5                                                                # a second label on the background at 4 m
        return depth, mask

    Hm = np.eye(4); Hm[:3, 3] = Tcw[:3, :3].T @ [0.1, 0.0, 0.0]                             # the walk in the world frame
    for k in range(4):
        depth, mask = frame(k)
        motions = [(11, 3, Hm), (12, 5, np.eye(4)), (13, 6, np.eye(4))]
        s1 = dev.fuse(k, depth, mask, Tcw, motions); s2 = ref.fuse(k, depth, mask, Tcw, motions)
        assert np.array_equal(s1, s2) and dev.info() == ref.info() and (dev.skipped, dev.dropped) == (ref.skipped, ref.dropped), k
    live = dev.live[0]
    rl = ref.live[0]
    assert live.mod_label == 11 and live.frames == 4 and np.array_equal(live.Two, rl.Two)
    words, origin = live.mapper.volume()
    assert tuple(origin) == (-12, -12, -12) and np.array_equal(words, rl.V.words)
    xyz, grad, wgt, n = live.mapper.extract_all(1)
    rx, rg, rw = rl.V.extract(rl.V.origin, rl.V.origin + 24, 1)
    assert n == len(rx) > 100 and np.array_equal(xyz.view(np.uint32), rx.view(np.uint32)) and np.array_equal(grad, rg) and np.array_equal(wgt, rw)
    T = (Tcw @ live.Two).astype(F)
    view = Raycaster(live.mapper, Wd, Hd, Kd, 1.0, 0.025, 96, min_weight=1)
    d, g, w, counts = view.render(T)
    rd, rg2, rw2, rcounts = RR.render(rl.V, Wd, Hd, Kd, 1.0, 0.025, 96, 1, T)
    assert counts == rcounts and counts[0] > 50
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32)) and np.array_equal(g.view(np.uint32), rg2.view(np.uint32)) and np.array_equal(w, rw2)
    view.close()
    # the label disappears: the model is retired with its points, its handle is cleared and goes back to the pool
    depth, mask = frame(4, gone=True)
    dev.fuse(4, depth, mask, Tcw, [(12, 5, np.eye(4))]); ref.fuse(4, depth, mask, Tcw, [(12, 5, np.eye(4))])
    assert dev.info() == ref.info() and [m.mod_label for m in dev.finished] == [11] and len(dev.pool) == 1
    assert not dev.pool[0].volume()[0].any() and dev.pool[0].origin() == (-12, -12, -12)
    for md, mr in zip(dev.models(), ref.models()):
        assert np.array_equal(md["xyz"].view(np.uint32), mr["xyz"].view(np.uint32)) and np.array_equal(md["grad"], mr["grad"]) and np.array_equal(md["weight"], mr["weight"])
        assert all(fa == fb and np.array_equal(Ta, Tb) for (fa, Ta), (fb, Tb) in zip(md["trajectory"], mr["trajectory"])) and len(md["trajectory"]) == len(mr["trajectory"])
    # saving twice changes nothing
    from vdo_slam_amd.dense import read_ply
    dev.save(str(tmp_path / "a")); dev.save(str(tmp_path / "b"))
    for name in ("_11.ply", "_12.ply", "_poses.txt"):
        assert (tmp_path / ("a" + name)).read_bytes() == (tmp_path / ("b" + name)).read_bytes()
    px, _, pw = read_ply(str(tmp_path / "a_11.ply"))
    assert np.array_equal(px.view(np.uint32), dev.finished[0].xyz.view(np.uint32)) and np.array_equal(pw, dev.finished[0].wgt)
    assert len((tmp_path / "a_poses.txt").read_text().splitlines()) == 4 + 5
    dev.close()


# ---- refusals and vdo_dense_clear ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_volumes_and_the_stats_unchanged(ctx):
    from vdo_slam_amd import objects as O
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.dense import DenseMapper
    from vdo_slam_amd.frontend import FrameImages
    L = O._lib()
    L.vdo_last_error.restype = C.c_char_p
    h = C.c_void_p()

    def create(Wc=8, Hc=8, **kw):
        prm = dict(K=(4.0, 4.0, 4.0, 4.0), min_depth=0.0, max_depth=10.0, max_labels=3, max_batch=2)
        prm.update(kw)
        pc = O.ObjectsParamsC((C.c_float * 4)(*prm["K"]), prm["min_depth"], prm["max_depth"], prm["max_labels"], prm["max_batch"])
        return L.vdo_objects_create(ctx._h, Wc, Hc, C.byref(pc), C.byref(h)), L.vdo_last_error().decode()

    nan, inf = float("nan"), float("inf")
    for kw, word in [(dict(Wc=0), "width"), (dict(Hc=0), "height"), (dict(K=(0.0, 4.0, 4.0, 4.0)), "fx"), (dict(K=(4.0, 4.0, nan, 4.0)), "K[2]"), (dict(min_depth=-1.0), "min_depth"),
                     (dict(max_depth=0.0), "max_depth"), (dict(max_depth=inf), "max_depth"), (dict(max_labels=0), "max_labels"), (dict(max_labels=1024), "max_labels"),
                     (dict(max_batch=0), "max_batch"), (dict(max_batch=65), "max_batch")]:
        rc, msg = create(**kw)
        assert rc == -1 and word in msg and not h.value, (kw, rc, msg)
    rc, msg = create(Wc=4096, Hc=4096, K=(1e-6, 1e-6, 0.0, 0.0), max_depth=1e30)     # a sum could leave int64
    assert rc == -4 and "int64" in msg and not h.value, (rc, msg)

    depth, mask = _images(3)
    st = _stage(ctx, W, H, K4, max_labels=5, max_batch=2, **PRM)
    T = _pose((6, 5, 4), (0, 0, 0), 0.1, (-1.0, 0.0, 3.0))
    a, b, c = (Obj(ctx, (6, 5, 4), 0.1, (0, 0, 0), l, T) for l in (1, 2, 3))
    _fuse_and_check(st, [a, b], depth, mask, "seed")
    stats = st.last_stats()
    other_ctx = Context(0)
    foreign = DenseMapper(other_ctx, W, H, (4, 4, 4), 0.1, K4, max_depth=10.0)
    small = DenseMapper(ctx, W - 1, H, (4, 4, 4), 0.1, K4, max_depth=10.0)
    deep = DenseMapper(ctx, W, H, (4, 4, 4), 0.1, K4, max_depth=12.0)
    out = np.full((3, 3), -5, np.int64)
    Ts = np.ascontiguousarray(np.stack([T, T, T]).reshape(3, 16))
    dp, mp = depth.ctypes.data, mask.ctypes.data

    def call(n, maps, labels, depth_p=dp, mask_p=mp, ds=W, ms=W, hh=None, Tp=Ts.ctypes.data, outp=out.ctypes.data):
        hs = (C.c_void_p * 3)(*[m._h.value if m is not None else None for m in maps]) if maps is not None else None
        lab = np.array(labels, np.int32) if labels is not None else None
        rc = L.vdo_objects_integrate(st._h if hh is None else hh, depth_p, ds, mask_p, ms, 0, n, hs, lab.ctypes.data if lab is not None else None, Tp, outp)
        return rc, L.vdo_last_error().decode()

    for args, word in [((-1, [a.m, b.m, None], [1, 2, 1]), "n -1"), ((3, [a.m, b.m, c.m], [1, 2, 3]), "max_batch"), ((2, [a.m, None, None], [1, 2, 1]), "maps[1] is null"),
                       ((2, [a.m, a.m, None], [1, 2, 1]), "once in a batch"), ((2, [a.m, foreign, None], [1, 2, 1]), "another context"),
                       ((2, [a.m, small, None], [1, 2, 1]), "images"), ((2, [a.m, deep, None], [1, 2, 1]), "depth range"), ((2, [a.m, b.m, None], [1, 0, 1]), "labels[1]"),
                       ((2, [a.m, b.m, None], [6, 2, 1]), "labels[0]"), ((2, [a.m, b.m, None], [-3, 2, 1]), "labels[0]"), ((2, None, [1, 2, 1]), "maps is null"),
                       ((2, [a.m, b.m, None], None), "labels is null")]:
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (args[0], args[2], rc, msg)
    for kw, word in [(dict(mask_p=None), "mask is null"), (dict(depth_p=None), "depth is null"), (dict(ds=W - 1), "depth_stride"), (dict(ms=W - 1), "mask_stride"),
                     (dict(Tp=None), "T is null"), (dict(outp=None), "out is null")]:
        rc, msg = call(2, [a.m, b.m, None], [1, 2, 1], **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert L.vdo_objects_integrate(None, dp, W, mp, W, 0, 0, None, None, None, None) == -1
    fi = FrameImages(ctx, W - 1, H)
    assert L.vdo_objects_integrate_frame(st._h, fi._h, 0, None, None, None, None) == -1 and "frame is" in L.vdo_last_error().decode()
    assert L.vdo_objects_integrate_frame(st._h, None, 0, None, None, None, None) == -1 and L.vdo_objects_stats_frame(st._h, None, None) == -1
    assert L.vdo_objects_stats(st._h, dp, W, None, W, 0, None) == -1 and L.vdo_objects_stats(st._h, None, W, mp, W, 0, None) == -1
    assert L.vdo_objects_set_cull(st._h, 2) == -1 and L.vdo_objects_set_cull(None, 1) == -1 and L.vdo_objects_last_stats(st._h, None) == -1
    assert L.vdo_objects_last_timing(st._h, None) == -1 and L.vdo_objects_destroy(None) == 0 and L.vdo_dense_clear(None) == -1
    fresh = _stage(ctx, W, H, K4, max_labels=5, max_batch=2, **PRM)
    assert L.vdo_objects_last_stats(fresh._h, stats.ctypes.data) == -1 and "yet" in L.vdo_last_error().decode()
    fresh.close()
    assert (out == -5).all() and np.array_equal(st.last_stats(), stats)
    for o in (a, b):
        assert np.array_equal(o.m.volume()[0], o.V.words)
    assert not c.m.volume()[0].any()
    # the frame form equals the array form
    full = FrameImages(ctx, W, H)
    full.upload(depth, np.zeros((H, W, 2), F), mask)
    got = st.integrate_frame(full._h, [a.m, b.m], [1, 2], [T, T])
    for i, o in enumerate((a, b)):
        upd, occ = OR.integrate(o.V, depth, mask, o.label, T, K4, *o.prm)
        assert got[i].tolist()[:2] == [upd, occ] and np.array_equal(o.m.volume()[0], o.V.words)
    assert np.array_equal(st.stats_frame(full._h), stats)
    for o in (a, b, c):
        o.close()
    for m in (foreign, small, deep):
        m.close()
    st.close(); other_ctx.close()


def test_dense_clear_leaves_zeros_and_keeps_the_origin(ctx):
    from vdo_slam_amd import objects as O
    from vdo_slam_amd.dense import DenseMapper
    m = DenseMapper(ctx, 8, 8, (7, 5, 3), 0.1, (4.0, 4.0, 4.0, 4.0), origin=(-3, 2, 9))
    m.set_volume(np.random.default_rng(0).integers(1, 1 << 24, (3, 5, 7)).astype(np.uint32))
    assert m.volume()[0].all()
    O.clear(m)
    words, origin = m.volume()
    assert not words.any() and tuple(origin) == (-3, 2, 9)
    m.close()
