"""GPU: the device colourer (vdo_colour_*, csrc/colour.hip) against the NumPy restatement of its contract (tests/colour_ref.py).  Every comparison
is array_equal: the colour words, the counts, the sampled and the rendered colours.

The shapes are the smallest that still reach every edge: a 40 x 22 x 9 volume (x no multiple of 64, y of none of 2, 4 and 8, z no multiple of 4;
more than one workgroup along y and z) at a negative origin (so that origin mod size is not 0 on any axis), 61 x 37 images, voxel 0.25 so that
voxel centres, depths and the band are exact in fp32."""
import ctypes as C

import numpy as np
import pytest

from tests import colour_ref as CR
from tests import dense_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
N, ORIGIN, VOXEL = (40, 22, 9), (-23, -9, -3), 0.25
W, H, K4 = 61, 37, (10.0, 10.0, 30.0, 18.0)
TRUNC, MIN_D, MAX_D, BAND, MAX_W = 1.0, 0.3, 3.0, 0.25, 64


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def make(ctx):
    """make(...) -> (device mapper, its colourer, the restatement's colour volume).  Whatever a test made is closed when it ends, borrowers first, also
    when it failed: no handle outlives the module's context."""
    from vdo_slam_amd.colour import Colourer
    from vdo_slam_amd.dense import DenseMapper
    made = []

    def _make(band=BAND, max_weight=MAX_W, stage_points=64, origin=ORIGIN):
        m = DenseMapper(ctx, W, H, N, VOXEL, K4, origin=origin, trunc=TRUNC, min_depth=MIN_D, max_depth=MAX_D, max_weight=64, stage_points=64)
        made.append(m)
        c = Colourer(m, band, max_weight, stage_points)
        made.append(c)
        return m, c, CR.ColourVolume(N, VOXEL, origin)
    _make.closing = lambda h: (made.append(h), h)[1]
    yield _make
    for h in reversed(made):
        h.close()


class Frame:
    """A vdo_frame_images holding a depth and a mask, through untyped entries of a library object of its own: this module declares no argument
    types that another test module may rely on not being declared."""

    def __init__(self, ctx, w, h):
        from vdo_slam_amd import _capi as K
        K.lib()
        self.L = C.CDLL(K.LIB_PATH)
        self.w, self.h, self._h = w, h, C.c_void_p()
        assert self.L.vdo_frame_images_create(ctx._h, C.c_int(w), C.c_int(h), C.byref(self._h)) == 0

    def upload(self, depth, mask):
        d = np.ascontiguousarray(depth, F); m = np.ascontiguousarray(mask, np.int32); f = np.zeros((self.h, self.w, 2), F)
        assert self.L.vdo_frame_images_upload(self._h, C.c_void_p(d.ctypes.data), C.c_void_p(f.ctypes.data), C.c_void_p(m.ctypes.data)) == 0

    def download(self):
        d = np.zeros((self.h, self.w), F); m = np.zeros((self.h, self.w), np.int32)
        assert self.L.vdo_frame_images_download_depth(self._h, C.c_void_p(d.ctypes.data)) == 0
        assert self.L.vdo_frame_images_download_mask(self._h, C.c_void_p(m.ctypes.data)) == 0
        return d, m

    def close(self):
        if self._h:
            self.L.vdo_frame_images_destroy(self._h); self._h = C.c_void_p()


def ref_integrate(V, depth, mask, image, T, label=0, rgb_order=0, band=BAND, max_weight=MAX_W, map_origin=None):
    return V.integrate(depth, mask, image, T, K4, MIN_D, MAX_D, band, max_weight, label, rgb_order, map_origin)


def pose(tilt=0.06, t=(0.05, -0.1, 0.02)):
    c, s = np.cos(tilt), np.sin(tilt)
    T = np.eye(4, dtype=F)
    T[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], F) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]], F)
    T[:3, 3] = t
    return T


def frame(seed, channels=3):
    """a tilted wall about 1 m ahead with every kind of unusable depth sprinkled in, a three-label mask, a random image"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    depth = (1.0 + 0.004 * (xs - W / 2) - 0.003 * (ys - H / 2) + rng.normal(0, 0.02, (H, W))).astype(F)
    bad = rng.random((H, W))
    for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, 0.2, MIN_D, 5.0, -1.0)):       # 0.2 < min_depth, min_depth itself (d > min_depth fails), 5 > max_depth
        depth[(bad >= 0.02 * k) & (bad < 0.02 * (k + 1))] = v
    mask = np.zeros((H, W), np.int32)
    mask[5:20, 8:30] = 1; mask[15:34, 35:55] = 2
    image = rng.integers(0, 256, (H, W) if channels == 1 else (H, W, channels), dtype=np.uint8)
    return depth, mask, image


def same(col, V, what):
    words, origin = col.volume()
    assert tuple(origin) == tuple(int(v) for v in V.origin), what
    assert np.array_equal(words, V.words), f"{what}: {(words != V.words).sum()} colour words differ"


def test_voxels_per_thread_and_a_few_frames(ctx, make):
    """several frames from different poses: the running mean over many voxels; all four word-traffic settings give the same words and counts"""
    got = []
    for vpt in (1, 2, 4, 8):
        m, col, V = make()
        col.set_voxels_per_thread(vpt)
        for k in range(3):
            depth, mask, image = frame(k)
            T = pose(0.05 * k, (0.05 * k, -0.1, 0.02))
            counts = col.integrate(depth, mask, image, T)
            assert counts == ref_integrate(V, depth, mask, image, T), f"vpt {vpt}, frame {k}"
            assert counts[0] > 150 and counts[1] > 50 and counts[2] > 500
        same(col, V, f"vpt {vpt}")
        assert (V.words >> 24).max() == 3                                             # some voxels were seen by all three frames
        got.append(col.volume()[0])
        col.close(); m.close()
    assert all(np.array_equal(got[0], g) for g in got[1:])


@pytest.mark.parametrize("how", ["host", "host strided", "device", "device strided"])
def test_source_formats(ctx, make, how):
    """channels 1, 3 and 4 with both orders, packed and strided, host and device: one frame each into one volume"""
    import torch
    m, col, V = make()
    T = pose()
    k = 0
    for channels in (1, 3, 4):
        for order in (0, 1):
            depth, mask, image = frame(10 + k, channels); k += 1
            pad = 5 if "strided" in how else 0
            dd = np.full((H, W + pad), 7.0, F); mm = np.full((H, W + pad), 1, np.int32); ii = np.full((H, W + pad) + image.shape[2:], 99, np.uint8)
            dd[:, :W] = depth; mm[:, :W] = mask; ii[:, :W] = image
            if "device" in how:
                td, tm, ti = (torch.from_numpy(a).cuda() for a in (dd, mm, ii))
                torch.cuda.synchronize()
                counts = col.integrate_raw(td.data_ptr(), W + pad, tm.data_ptr(), W + pad, ti.data_ptr(), (W + pad) * channels, channels, order, True, 0, T)
            elif pad:
                counts = col.integrate(dd[:, :W], mm[:, :W], ii[:, :W], T, 0, order)      # K.rows hands the views over with their strides
            else:
                counts = col.integrate(depth, mask, image, T, 0, order)
            assert counts == ref_integrate(V, depth, mask, image, T, 0, order), f"{how}, channels {channels}, order {order}"
            same(col, V, f"{how}, channels {channels}, order {order}")
    w = V.words[V.words != 0]
    assert len(w) > 150 and np.any((w & 0xFF) != ((w >> 16) & 0xFF))                  # R and B differ somewhere: the order matters
    col.close(); m.close()


def test_a_frame_images_source_equals_the_array_source(ctx, make):
    """vdo_colour_integrate_frame: the resident depth and mask of a vdo_frame_images, read where they lie and not written; the image from the host,
    strided, and from the device; labels 0, 2 and -1"""
    import torch
    m, col, V = make()
    fi = make.closing(Frame(ctx, W, H))
    T = pose()
    for k, (label, channels, order, on_device) in enumerate(((0, 3, 0, False), (2, 4, 1, True), (-1, 1, 0, True), (0, 3, 1, False))):
        depth, mask, image = frame(20 + k, channels)
        fi.upload(depth, mask)
        wide = np.full((H, W + 3) + image.shape[2:], 99, np.uint8); wide[:, :W] = image
        if on_device:
            t = torch.from_numpy(wide).cuda(); torch.cuda.synchronize()
            counts = col.integrate_frame(fi._h, t.data_ptr(), (W + 3) * channels, channels, order, True, T, label)
        else:
            counts = col.integrate_frame(fi._h, wide.ctypes.data, (W + 3) * channels, channels, order, False, T, label)
        assert counts == ref_integrate(V, depth, mask, image, T, label, order) and counts[0] > 0, (label, channels, order, on_device)
        same(col, V, f"from a frame, label {label}")
        d_back, m_back = fi.download()
        assert np.array_equal(m_back, mask) and np.array_equal(d_back.view(np.uint32), depth.view(np.uint32))      # read-only on them


def test_the_order_and_grey_are_what_they_say(ctx, make):
    """one observation of a constant image: the word IS the packed pixel, weight 1"""
    for channels, order, px, want in ((3, 0, (10, 20, 30), 10 | 20 << 8 | 30 << 16), (3, 1, (10, 20, 30), 30 | 20 << 8 | 10 << 16),
                                      (4, 0, (10, 20, 30, 200), 10 | 20 << 8 | 30 << 16), (4, 1, (10, 20, 30, 200), 30 | 20 << 8 | 10 << 16), (1, 0, (77,), 77 * 0x010101)):
        m, col, V = make()
        image = np.broadcast_to(np.array(px, np.uint8), (H, W, channels)).copy()
        counts = col.integrate(np.full((H, W), 1.375, F), None, image, np.eye(4, dtype=F), 0, order)
        words = col.volume()[0]
        assert counts[0] > 0 and set(np.unique(words)) == {0, want | 1 << 24}
        col.close(); m.close()


def test_band_edge_and_depth_values(ctx, make):
    """T = identity: Zc is the voxel centre's z, exact.  Depth 1.375 puts the voxels at z = 1.125 exactly ON the band (|s| == band: inside), the next
    float above puts them just beyond it; the voxels at z = 1.375 are inside either way.  Unusable depths colour nothing."""
    m, col, V = make()
    T = np.eye(4, dtype=F)
    depth = np.full((H, W), 1.375, F)
    depth[:, W // 2:] = np.nextafter(F(1.375), F(2))
    for r, v in enumerate((np.nan, np.inf, -np.inf, 0.0, 0.2, MIN_D, 5.0)):
        depth[4 * r:4 * r + 4, :] = v
    image = np.full((H, W), 200, np.uint8)
    counts = col.integrate(depth, None, image, T)
    assert counts == ref_integrate(V, depth, None, image, T)
    same(col, V, "band edge")
    cw = (V.words >> 24).astype(int)
    gz = V.globals_of_slots(2)
    z_of = lambda z: int(np.nonzero((gz.astype(F) + F(0.5)) * F(VOXEL) == F(z))[0][0])
    on_edge, inside = cw[z_of(1.125)], cw[z_of(1.375)]
    assert inside.sum() > on_edge.sum() > 0 and cw.sum() == inside.sum() + on_edge.sum()      # no other z is within the band
    # the voxels on the edge all look at the left half of the image; the rows of unusable depth coloured nothing at either z
    gx = V.globals_of_slots(0)
    left = ((gx.astype(F) + F(0.5)) * F(VOXEL) * F(K4[0]) / F(1.125) + F(K4[2])) < (W // 2 - 0.5)
    assert on_edge[:, left].sum() == on_edge.sum() and inside[:, ~left].sum() > 0
    assert counts[0] == cw.sum() and counts[2] > 0
    col.close(); m.close()


@pytest.mark.parametrize("label", [0, 2, -1])
def test_label_rule(ctx, make, label):
    for with_mask in (True, False):
        m, col, V = make()
        depth, mask, image = frame(3)
        mk = mask if with_mask else None
        T = pose()
        counts = col.integrate(depth, mk, image, T, label)
        assert counts == ref_integrate(V, depth, mk, image, T, label)
        same(col, V, f"label {label}, mask {with_mask}")
        if label > 0 and not with_mask:
            assert counts[0] == 0 and counts[2] == 0 and counts[1] > 0               # m = 0 is not the label: nothing is coloured
        elif label < 0 or not with_mask:
            assert counts[1] == 0 and counts[0] > 0
        else:
            assert counts[0] > 0 and counts[1] > 0
        col.close(); m.close()


def test_running_mean_rounding_and_saturation(ctx, make):
    """0, 255, 1 on the same voxels: 0 -> (2*255 + 2) / 4 = 128 -> (2*(128*2 + 1) + 3) / 6 = 86 (the exact mean 85.33 would round to 85).  Then
    max_weight 3, five frames and more: the weight stays 3, and a frame that changes no word still counts its voxels as updated."""
    T = np.eye(4, dtype=F)
    depth = np.full((H, W), 1.375, F)
    m, col, V = make()
    for v in (0, 255, 1):
        image = np.full((H, W), v, np.uint8)
        assert col.integrate(depth, None, image, T) == ref_integrate(V, depth, None, image, T)
    same(col, V, "0, 255, 1")
    assert set(np.unique(V.words)) == {0, 86 * 0x010101 | 3 << 24}
    col.close(); m.close()
    m, col, V = make(max_weight=3)
    seen = []
    for k, v in enumerate((40, 90, 200, 200, 200) + (200,) * 25):                    # five frames pin the saturation; the rest run the mean to its fixed point
        image = np.full((H, W), v, np.uint8)
        counts = col.integrate(depth, None, image, T)
        assert counts == ref_integrate(V, depth, None, image, T, max_weight=3)
        seen.append((counts, col.volume()[0]))
    same(col, V, "saturation")
    assert (seen[4][1] >> 24).max() == 3 and (seen[1][1] >> 24).max() == 2
    # the fixed point under 200 at weight 3: (2 * (199 * 3 + 200) + 4) / 8 = 199 - the rounded mean stops one short of the observation
    assert set(np.unique(V.words)) == {0, 199 * 0x010101 | 3 << 24}
    assert np.array_equal(seen[-1][1], seen[-2][1]) and seen[-1][0] == seen[0][0] and seen[-1][0][0] > 0
    col.close(); m.close()


def test_follow_recentre_and_clear(ctx, make):
    m, col, V = make()
    rng = np.random.default_rng(5)
    full = rng.integers(1, 1 << 32, N[::-1], dtype=np.uint64).astype(np.uint32) | np.uint32(1 << 24)
    depth, mask, image = frame(4)
    T = pose()
    o = list(ORIGIN)
    for d in ((5, -3, 2), (0, 0, -1), (-39, 21, 8), (40, 0, 0), (1, -22, 0), (0, 0, 9), (3, 3, 3), (-3, -3, -3)):
        m.recenter(ORIGIN); V.follow(ORIGIN)                                          # every move starts where the frames are in view
        o = list(ORIGIN)
        col.set_volume(full); V.words = full.copy()
        q = [o[a] + d[a] for a in range(3)]
        m.recenter(q)
        # brute force: every slot's global voxel before and after; a word survives iff they are the same
        keep = np.ones(N[::-1], bool)
        for a in range(3):
            s = np.arange(N[a])
            before = np.array([next(g for g in range(o[a], o[a] + N[a]) if g % N[a] == si) for si in s])
            after = np.array([next(g for g in range(q[a], q[a] + N[a]) if g % N[a] == si) for si in s])
            shape = [1, 1, 1]; shape[2 - a] = N[a]
            keep &= (before == after).reshape(shape)
        V.follow(q)
        assert np.array_equal(V.words, np.where(keep, full, 0))
        if max(abs(v) / n for v, n in zip(d, N)) >= 1:
            assert not V.words.any()
        same(col, V, f"moved by {d}")                                                 # get_volume follows
        counts = col.integrate(depth, mask, image, T)                                 # and a frame on top of what stayed
        assert counts == ref_integrate(V, depth, mask, image, T)
        same(col, V, f"moved by {d}, then a frame")
    m.recenter(ORIGIN)
    # two frames with a move between them, the colourer not asked in between
    col.clear(); V.clear(o)
    assert not col.volume()[0].any()
    assert col.integrate(depth, mask, image, T) == ref_integrate(V, depth, mask, image, T)
    q = [o[0] + 5, o[1] - 3, o[2] + 2]
    m.recenter(q)
    d2, m2, i2 = frame(6)
    assert col.integrate(d2, m2, i2, T) == ref_integrate(V, d2, m2, i2, T, map_origin=q)
    same(col, V, "a move between two frames")
    assert V.words.any()
    # away and back between two entries: only the difference counts
    m.recenter([q[0] + 7, q[1], q[2]]); m.recenter(q)
    same(col, V, "away and back")
    m.clear(); col.clear(); V.clear(q)
    same(col, V, "cleared")
    col.close(); m.close()


def random_words(seed, p_empty=0.3):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 24, N[::-1]).astype(np.uint32) | (rng.integers(1, 256, N[::-1]).astype(np.uint32) << 24)
    w[rng.random(N[::-1]) < p_empty] = 0
    return w


def sample_points(seed):
    rng = np.random.default_rng(seed)
    o, n, v = np.array(ORIGIN), np.array(N), F(VOXEL)
    gx, gy, gz = np.meshgrid(*[np.arange(o[a] - 1, o[a] + n[a] + 1) for a in range(3)], indexing="ij")
    centres = (np.stack([gx, gy, gz], -1).reshape(-1, 3).astype(F) + F(0.5)) * v     # fi = 0 on every axis, one ring outside the volume included
    below = np.nextafter(centres, F(-np.inf))
    near0 = np.array([[np.nextafter(F(0.125), F(0))] * 3], F)                         # u - 0.5 = -2^-25: b = -1 and u - b rounds up to 1: fi = 256
    faces = []
    for a in range(3):
        for side in (o[a], o[a] + n[a]):                                              # on a face: b = side - 1 and side, half the corners outside
            p = (o + rng.random((40, 3)) * n) * v
            p[:, a] = side * v + rng.choice([-0.124, -0.01, 0.0, 0.01, 0.124], 40)
            faces.append(p.astype(F))
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1048576.0, 0, 0], [0, -1048576.0, 0], [0, 0, 1.2e6], [1e30, 0, 0], [-1e30, 0, 0],
                    [1048575.8, 0, 0], [-1048575.9, 0, 0], [3.4e38, 3.4e38, 3.4e38]], F)
    rnd = ((o - 1.5) + rng.random((1000, 3)) * (n + 3)) * v
    return np.concatenate([centres, below, near0] + faces + [odd, rnd.astype(F)])


def test_sample(ctx, make):
    import torch
    m, col, V = make(stage_points=64)
    words = random_words(1)
    words[0, 0, 0] = 0x123456 | 9 << 24                                               # global voxel (0, 0, 0) lives at slot (0, 0, 0)
    col.set_volume(words); V.words = words.copy()
    pts = sample_points(2)
    # the point a hair below the centre of voxel (0, 0, 0) has fi = 256 on every axis: all its weight lies on that voxel
    near0 = np.array([[np.nextafter(F(0.125), F(0))] * 3], F)
    assert tuple(V.sample(near0, 1)[0]) == (0x56, 0x34, 0x12, 255)
    for mw in (1, 3, 100, 255):
        want = V.sample(pts, mw)
        got, n_col = col.sample(pts, mw)                                              # host: through windows of 64 points
        assert np.array_equal(got, want), f"min_weight {mw}: {(got != want).any(1).sum()} points differ"
        assert n_col == int((want[:, 3] != 0).sum())
        tp = torch.from_numpy(pts).cuda(); to = torch.full((len(pts), 4), 77, dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert col.sample_raw(len(pts), tp.data_ptr(), mw, to.data_ptr(), True) == n_col
        assert np.array_equal(to.cpu().numpy(), want)
    a1 = V.sample(pts, 1)
    assert (a1[:, 3] == 0).sum() > 100 and (a1[:, 3] == 255).sum() > 100 and ((a1[:, 3] > 0) & (a1[:, 3] < 255)).sum() > 100
    assert (V.sample(pts, 255)[:, 3] != 0).sum() < (a1[:, 3] != 0).sum()              # the gate takes corners away
    assert not a1[-1011:-1000].any()                                                  # the non-finite and far points have no colour
    assert col.sample(np.zeros((0, 3), F))[1] == 0
    col.close(); m.close()


def test_render(ctx, make):
    """a fused, coloured wall; its depth view at 31 x 17 with other intrinsics, holes punched in; the colour image of that depth image"""
    from vdo_slam_amd.raycast import Raycaster
    import torch
    m, col, V = make(stage_points=100)
    ys, xs = np.mgrid[0:H, 0:W]
    depth = (0.95 + 0.002 * (xs - W / 2)).astype(F)
    image = np.stack([4 * xs, 6 * ys, 255 - 3 * xs], -1).astype(np.uint8)
    Ts = [pose(0.0, (0, 0, 0)), pose(0.04, (0.03, 0.02, 0.0))]
    for T in Ts:
        m.integrate(depth, None, T)
        assert col.integrate(depth, None, image, T) == ref_integrate(V, depth, None, image, T)
    Kv = (14.0, 15.0, 15.5, 8.25)
    view = make.closing(Raycaster(m, 31, 17, Kv, 0.3, 0.1, 25, 1))
    Tv = pose(0.02, (0.01, 0.0, 0.0))
    d, _, _, hits = view.render(Tv)
    assert hits[0] > 150
    d[3:5, 4:9] = 0.0; d[10, 20] = np.nan; d[11, 21] = np.inf; d[12, 22] = -1.0; d[0, 0] = 100.0
    for mw in (1, 2):
        want, wc = V.render(d, Kv, Tv, mw)
        got, gc = col.render(d, Kv, Tv, mw)                                           # host: windows of 100 pixels
        assert np.array_equal(got, want) and gc == wc
        td = torch.from_numpy(d).cuda(); to = torch.full((17, 31, 4), 9, dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert col.render_raw(td.data_ptr(), 31, 17, Kv, Tv, mw, to.data_ptr(), True) == wc
        assert np.array_equal(to.cpu().numpy(), want)
    want, wc = V.render(d, Kv, Tv, 1)
    assert wc[0] > 120 and wc[1] >= 1 and not want[3:5, 4:9].any() and not want[10, 20].any() and not want[0, 0].any()
    view.close(); col.close(); m.close()


def test_refusals_leave_everything_untouched(ctx, make):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd.colour import ColourParamsC, Colourer, _lib
    m, col, V = make()
    L = _lib()
    words = random_words(3)
    col.set_volume(words)
    depth, mask, image = frame(0)
    T = np.eye(4, dtype=F).reshape(16)
    out = (C.c_int64 * 3)(-7, -7, -7)
    pd, pm, pi, pT = depth.ctypes.data, mask.ctypes.data, image.ctypes.data, T.ctypes.data

    def refused(rc, what):
        assert rc == K.VDO_ERR_INVALID, f"{what}: {rc}"
        assert list(out) == [-7, -7, -7], what
        assert np.array_equal(col.volume()[0], words), what

    ok = dict(h=col._h, depth=pd, ds=W, mask=pm, ms=W, image=pi, istride=3 * W, ch=3, order=0, dev=0, label=0, T=pT, out=out)
    for change, what in ((dict(h=None), "handle"), (dict(depth=None), "depth"), (dict(image=None), "image"), (dict(T=None), "T"), (dict(out=None), "out"),
                         (dict(ds=W - 1), "depth stride"), (dict(ms=W - 1), "mask stride"), (dict(istride=3 * W - 1), "image stride"), (dict(ch=2), "channels 2"),
                         (dict(ch=0), "channels 0"), (dict(ch=5), "channels 5"), (dict(order=2), "rgb_order 2"), (dict(order=-1), "rgb_order -1")):
        a = dict(ok, **change)
        refused(L.vdo_colour_integrate(a["h"], a["depth"], a["ds"], a["mask"], a["ms"], a["image"], a["istride"], a["ch"], a["order"], a["dev"], a["label"], a["T"], a["out"]),
                "integrate: " + what)
    # the same refusals from a resident frame: a null frame, a frame of another size, and with a valid frame everything the array entry refuses
    good = make.closing(Frame(ctx, W, H)); small = make.closing(Frame(ctx, W - 1, H))
    good.upload(depth, mask)
    okf = dict(ok, frame=good._h)
    for change, what in ((dict(h=None), "handle"), (dict(frame=None), "a null frame"), (dict(frame=small._h), "a frame of another size"), (dict(image=None), "image"),
                         (dict(T=None), "T"), (dict(out=None), "out"), (dict(istride=3 * W - 1), "image stride"), (dict(ch=2), "channels 2"), (dict(ch=0), "channels 0"),
                         (dict(ch=5), "channels 5"), (dict(order=2), "rgb_order 2"), (dict(order=-1), "rgb_order -1")):
        a = dict(okf, **change)
        refused(L.vdo_colour_integrate_frame(a["h"], a["frame"], a["image"], a["istride"], a["ch"], a["order"], 0, 0, a["T"], a["out"]), "integrate_frame: " + what)
    # sample
    pts = np.zeros((4, 3), F); rgba = np.full((4, 4), 7, np.uint8); nc = C.c_int64(-7)
    for args, what in (((None, 4, pts.ctypes.data, 1, rgba.ctypes.data, 0, C.byref(nc)), "handle"), ((col._h, -1, pts.ctypes.data, 1, rgba.ctypes.data, 0, C.byref(nc)), "n"),
                       ((col._h, 4, None, 1, rgba.ctypes.data, 0, C.byref(nc)), "xyz"), ((col._h, 4, pts.ctypes.data, 1, None, 0, C.byref(nc)), "rgba"),
                       ((col._h, 4, pts.ctypes.data, 0, rgba.ctypes.data, 0, C.byref(nc)), "min_weight 0"), ((col._h, 4, pts.ctypes.data, 256, rgba.ctypes.data, 0, C.byref(nc)), "min_weight 256"),
                       ((col._h, 4, pts.ctypes.data, 1, rgba.ctypes.data, 0, None), "n_coloured")):
        refused(L.vdo_colour_sample(*args), "sample: " + what)
        assert (rgba == 7).all() and nc.value == -7, what
    import torch
    d_pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda"); d_rgba = torch.full((24,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for off in (1, 2, 3):                                                             # a device output is written one word per point: it must be 4-byte aligned
        refused(L.vdo_colour_sample(col._h, 4, d_pts.data_ptr(), 1, d_rgba.data_ptr() + off, 1, C.byref(nc)), f"sample: a device rgba at offset {off}")
        assert nc.value == -7 and bool((d_rgba == 7).all())
    # render
    d = np.ones((3, 4), F); img = np.full((3, 4, 4), 7, np.uint8); Kc = (C.c_float * 4)(10, 10, 2, 1.5); o2 = (C.c_int64 * 2)(-7, -7)
    okr = dict(h=col._h, depth=d.ctypes.data, w=4, hh=3, K=Kc, T=pT, mw=1, rgba=img.ctypes.data, dev=0, out=o2)
    bad_K = [(C.c_float * 4)(*v) for v in ((0, 10, 2, 1.5), (10, -1, 2, 1.5), (np.nan, 10, 2, 1.5), (10, 10, np.inf, 1.5))]
    for change, what in ([(dict(h=None), "handle"), (dict(depth=None), "depth"), (dict(w=0), "width"), (dict(hh=0), "height"), (dict(K=None), "K"), (dict(T=None), "T"),
                          (dict(mw=0), "min_weight 0"), (dict(mw=256), "min_weight 256"), (dict(rgba=None), "rgba"), (dict(out=None), "out")] + [(dict(K=k), "a bad K") for k in bad_K]):
        a = dict(okr, **change)
        refused(L.vdo_colour_render(a["h"], a["depth"], a["w"], a["hh"], a["K"], a["T"], a["mw"], a["rgba"], a["dev"], a["out"]), "render: " + what)
        assert (img == 7).all() and list(o2) == [-7, -7], what
    d_depth = torch.ones((3, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for off in (1, 2, 3):
        refused(L.vdo_colour_render(col._h, d_depth.data_ptr(), 4, 3, Kc, pT, 1, d_rgba.data_ptr() + off, 1, o2), f"render: a device rgba at offset {off}")
        assert list(o2) == [-7, -7] and bool((d_rgba == 7).all())
    # VDO_ERR_UNSUPPORTED: over 2^26 pixels; over 2^24 on a side (either one) with fewer pixels than that
    for wh in ((1 << 14, 1 << 13), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        assert L.vdo_colour_render(col._h, d.ctypes.data, wh[0], wh[1], Kc, pT, 1, img.ctypes.data, 0, o2) == -4 and list(o2) == [-7, -7] and (img == 7).all(), wh
        assert np.array_equal(col.volume()[0], words)
    # the rest
    for rc, what in ((L.vdo_colour_clear(None), "clear"), (L.vdo_colour_get_volume(None, None, None), "get_volume: handle"), (L.vdo_colour_get_volume(col._h, None, None), "get_volume: both null"),
                     (L.vdo_colour_set_volume(None, words.ctypes.data), "set_volume: handle"), (L.vdo_colour_set_volume(col._h, None), "set_volume: words"),
                     (L.vdo_colour_set_voxels_per_thread(None, 4), "vpt: handle"), (L.vdo_colour_set_voxels_per_thread(col._h, 3), "vpt 3"),
                     (L.vdo_colour_last_timing(None, (C.c_double * 2)()), "timing: handle"), (L.vdo_colour_last_timing(col._h, None), "timing: ms")):
        refused(rc, what)
    # create
    hnd = C.c_void_p()
    for p, mp, o, what in ((ColourParamsC(0.25, 64, 8), None, C.byref(hnd), "map"), (None, m._h, C.byref(hnd), "params"), (ColourParamsC(0.25, 64, 8), m._h, None, "out"),
                           (ColourParamsC(0.0, 64, 8), m._h, C.byref(hnd), "band 0"), (ColourParamsC(-1.0, 64, 8), m._h, C.byref(hnd), "band < 0"),
                           (ColourParamsC(float(np.nextafter(F(TRUNC), F(2))), 64, 8), m._h, C.byref(hnd), "band > trunc"), (ColourParamsC(float("nan"), 64, 8), m._h, C.byref(hnd), "band nan"),
                           (ColourParamsC(0.25, 0, 8), m._h, C.byref(hnd), "max_weight 0"), (ColourParamsC(0.25, 256, 8), m._h, C.byref(hnd), "max_weight 256"),
                           (ColourParamsC(0.25, 64, 0), m._h, C.byref(hnd), "stage_points 0")):
        refused(L.vdo_colour_create(mp, C.byref(p) if p is not None else None, o), "create: " + what)
        assert not hnd.value, what
    edge = make.closing(Colourer(m, TRUNC, 255, 1))                                               # band == trunc, the largest weight and the smallest window are in range
    edge.close()
    # and after all that the handle still works
    col.set_volume(np.zeros(N[::-1], np.uint32))
    assert col.integrate(depth, mask, image, pose()) == ref_integrate(V, depth, mask, image, pose())
    same(col, V, "after the refusals")
    assert col.timing()[1] > 0
    col.close(); m.close()
