"""GPU: the device photometric aligner (vdo_photo_*, csrc/photo.hip) against the NumPy restatement of its contract (tests/photo_ref.py).  Sums are
compared as uint64 views, counts with array_equal, rows, grey images and packed models as uint32 views; a joint solve is walked through its trace,
with and without a vdo_align."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import align_ref as A
from tests import photo_ref as P
from tests.test_photo_ref import WALL_WEIGHT, wall_case

pytestmark = pytest.mark.gpu

F = np.float32
I4 = np.eye(4, dtype=F)
K1 = (1.0, 1.0, 0.0, 0.0)
PRM = dict(min_depth=0.3, max_depth=7.0, max_dist=0.15, max_diff=150.0)


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    gc.collect()                                        # whatever a raised error's traceback kept alive is destroyed while its context exists
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: counts {got[1].tolist()} against {want[1].tolist()}"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: sums differ at {np.nonzero(_bits(got[0]) != _bits(want[0]))[0].tolist()}: {got[0]} against {want[0]}"


class FrameImages:
    """The resident images of a frame (vdo_frame_images_*), called with typed pointers and no argtypes of its own"""

    def __init__(self, ctx, width, height):
        from vdo_slam_amd import photo as PH
        self._L, self.w, self.h = PH._lib(), width, height
        self._h = C.c_void_p()
        assert self._L.vdo_frame_images_create(ctx._h, C.c_int(width), C.c_int(height), C.byref(self._h)) == 0

    def upload(self, depth, mask):
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        d = np.ascontiguousarray(depth, F); f = np.zeros(d.shape + (2,), F); m = np.ascontiguousarray(mask, np.int32)
        assert self._L.vdo_frame_images_upload(self._h, d.ctypes.data_as(fp), f.ctypes.data_as(fp), m.ctypes.data_as(ip)) == 0

    def download_depth(self):
        out = np.zeros((self.h, self.w), F)
        assert self._L.vdo_frame_images_download_depth(self._h, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
        return out

    def close(self):
        if self._h:
            self._L.vdo_frame_images_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        self.close()


def _photo(ctx, W, H, K4, **kw):
    from vdo_slam_amd.photo import PhotoAligner
    prm = dict(PRM); prm.update(kw)
    return PhotoAligner(ctx, W, H, K4, **prm)


def _scene(W, H, Wm, Hm, seed):
    """A W x H frame looking where a Wm x Hm model of other intrinsics and another pose looks: surfaces near 3 m on both sides (most samples pass the
    occlusion gate, some do not), random grey values (some fail max_diff), holes, NaNs and negatives in the depth and in both model channels, a mask.
    -> dict(D, mask, img uint8 [H, W, 3], I, K4, T, Dm, Im, model, Km, Tm)"""
    rng = np.random.default_rng(seed)
    Km = (44.0 * Wm / 40, 40.0 * Hm / 22, 0.49 * Wm, 0.55 * Hm)
    sx, sy = W / Wm, H / Hm
    K4 = (Km[0] * sx, Km[1] * sy, (Km[2] + 0.5) * sx - 0.5, (Km[3] + 0.5) * sy - 0.5)
    Tm = A.perturbed(I4, (0.02, -0.01, 0.1), (1.0, -2.0, 0.5))
    T = A.perturbed(Tm, (0.01, -0.005, 0.008), (0.2, -0.3, 0.1))
    D = (3.0 + rng.normal(0, 0.04, (H, W))).astype(F)
    for bad in (0.0, np.nan, np.inf, -2.0, 9.0):
        D[rng.random((H, W)) < 0.01] = bad
    mask = (rng.random((H, W)) < 0.08).astype(np.int32) * 5
    base = rng.integers(40, 200)
    img = np.clip(base + rng.integers(-60, 60, (H, W, 3)), 0, 255).astype(np.uint8)
    Dm = (3.0 + rng.normal(0, 0.04, (Hm, Wm))).astype(F)
    Im = rng.uniform(base - 60, base + 60, (Hm, Wm)).astype(F)
    for bad in (0.0, np.nan, np.inf, -1.0):
        Dm[rng.random((Hm, Wm)) < 0.01] = bad
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        Im[rng.random((Hm, Wm)) < 0.01] = bad
    return dict(D=D, mask=mask, img=img, I=P.grey(img), K4=K4, T=T, Dm=Dm, Im=Im, model=P.pack_model(Dm, Im), Km=Km, Tm=Tm)


def _want(S, subsample=1, mask=True, T=None, **kw):
    prm = dict(PRM); prm.update(kw)
    return P.linearise(S["D"], S["mask"] if mask else None, S["I"], S["K4"], S["T"] if T is None else T, S["model"], S["Km"], S["Tm"], subsample=subsample, **prm)


def _loaded(ctx, S, **kw):
    W, H = S["D"].shape[1], S["D"].shape[0]
    ph = _photo(ctx, W, H, S["K4"], **kw)
    ph.set_image(S["img"])
    ph.set_model(S["Dm"], S["Im"], S["Km"], S["Tm"])
    return ph


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------------
# (W, H, Wm, Hm, subsample): 61 x 37 against 40 x 22 at every kind of subsample; 136 x 128: 272 tiles, a second tree launch whose one workgroup is
# partial (272 of 512 padded nodes); one tile, full and of one sample; models of one cell and of none
SHAPES = [(61, 37, 40, 22, s) for s in (1, 2, 3, 8)] + [(136, 128, 40, 22, 1), (1, 1, 1, 1, 1), (8, 8, 7, 9, 1), (61, 37, 2, 2, 1), (61, 37, 1, 9, 1), (61, 37, 9, 1, 1)]


@pytest.mark.parametrize("W,H,Wm,Hm,s", SHAPES, ids=lambda v: str(v))
def test_shapes_against_a_model_of_another_size(ctx, W, H, Wm, Hm, s):
    S = _scene(W, H, Wm, Hm, 1000 * W + 10 * Wm + s)
    want = _want(S, s)
    ph = _loaded(ctx, S, subsample=s, keep_rows=True)
    assert np.array_equal(_bits(ph.image()), _bits(S["I"])) and np.array_equal(_bits(ph.model()), _bits(S["model"]))
    got = ph.linearise(S["D"], S["mask"], S["T"])
    _same(got, want, f"{W}x{H} against {Wm}x{Hm} / {s}")
    assert np.array_equal(_bits(ph.rows()), _bits(want[2])), "rows"
    if Wm >= 40 and W * H // (s * s) >= 200:
        assert want[1][0] > 20 and (want[1][1:] > 0).all(), want[1]             # every class occurs
    if Wm == 2:
        assert want[1][0] > 0                                                    # one cell is a model
    if min(Wm, Hm) < 2:
        assert want[1][P.USED] == 0 and want[1][P.FAR] == 0 and want[1][P.NO_MODEL] > 0 and not got[0].any() and not np.signbit(got[0]).any()
    _same(ph.linearise(S["D"], S["mask"], S["T"]), want, "again")               # two runs, the same bits
    ph.close()


def test_272_tiles_take_a_second_tree_launch():
    tiles = (-(-136 // 8)) * (-(-128 // 8))
    assert tiles == 272 and 256 < tiles < 512


# ---- edge inputs -------------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_worked_by_hand_on_the_device(ctx):
    """tests/test_photo_ref.py's: u exactly integer, x0 = Wm - 2 and u = Wm - 1 exactly; the two pixels by hand; both gates at the bound and one float
    beyond, at each corner.  Four frame rows of zero depth below make room for the models (a model has at most the frame's pixel count)."""
    def run(D, I, dm, im, Tm, max_dist, max_diff, min_depth=0.0, max_depth=10.0, mask=None):
        D2 = np.zeros((5, D.shape[1]), F); D2[0] = D[0]
        I2 = np.zeros((5, D.shape[1]), np.uint8); I2[0] = I[0]
        m2 = None
        if mask is not None:
            m2 = np.zeros((5, D.shape[1]), np.int32); m2[0] = mask[0]
        ph = _photo(ctx, D.shape[1], 5, K1, min_depth=min_depth, max_depth=max_depth, max_dist=max_dist, max_diff=max_diff, keep_rows=True)
        ph.set_image(I2); ph.set_model(dm, im, K1, Tm)
        got = ph.linearise(D2, m2, I4)
        want = P.linearise(D2, m2, I2.astype(F), K1, I4, P.pack_model(dm, im), K1, Tm, min_depth, max_depth, max_dist, max_diff)
        _same(got, want, "by hand")
        assert np.array_equal(_bits(ph.rows()), _bits(want[2]))
        ph.close()
        c = got[1].copy(); c[P.NO_DEPTH] -= 4 * D.shape[1]                      # the four rows of zero depth
        return c.tolist(), want[2][0]

    D = np.array([[2.0, 2.0, 2.0]], F); I = np.array([[1, 2, 3]]); dm = np.full((2, 3), 2.0, F); im = np.array([[8, 16, 24], [12, 28, 44]], F)
    counts, rw = run(D, I, dm, im, I4, 1.0, 255.0)
    assert counts == [2, 0, 0, 1, 0] and rw[0, 6] == 7.0 and rw[1, 6] == 14.0 and rw[1, 0] == 4.0 and rw[1, 1] == 6.0 and not rw[2].any()
    Tm = I4.copy(); Tm[0, 3] = 0.25; Tm[1, 3] = 0.5
    D = np.array([[2.0, 2.0]], F); I = np.array([[10, 20]])
    counts, rw = run(D, I, dm, im, Tm, 1.0, 255.0)
    assert counts == [2, 0, 0, 0, 0] and rw[0].tolist() == [5.0, 2.5, -1.25, -5.0, 10.0, 0.0, 0.25, 1.0] and rw[1].tolist() == [5.0, 6.5, -7.25, -13.0, 24.5, 13.0, 0.25, 1.0]
    assert run(D, I, dm, im, Tm, 1.0, 255.0, mask=np.array([[0, 7]], np.int32))[0] == [1, 0, 1, 0, 0]
    below_half, below_quarter = float(np.nextafter(F(0.5), F(0))), float(np.nextafter(F(0.25), F(0)))
    D1 = np.array([[2.0]], F); I1 = np.array([[10]]); im1 = np.array([[8, 16], [12, 28]], F)
    for corner in range(4):
        for depth in (2.5, 1.5):
            dm1 = np.full((2, 2), 2.0, F); dm1.ravel()[corner] = depth
            assert run(D1, I1, dm1, im1, Tm, 0.5, 255.0)[0] == [1, 0, 0, 0, 0] and run(D1, I1, dm1, im1, Tm, below_half, 255.0)[0] == [0, 0, 0, 0, 1], (corner, depth)
    dm1 = np.full((2, 2), 2.0, F)
    assert run(D1, I1, dm1, im1, Tm, 1.0, 0.25)[0] == [1, 0, 0, 0, 0] and run(D1, I1, dm1, im1, Tm, 1.0, below_quarter)[0] == [0, 0, 0, 0, 1]
    assert run(D1, np.array([[255]]), dm1, np.zeros((2, 2), F), Tm, 1.0, 255.0)[0] == [1, 0, 0, 0, 0]       # 255 turns the gate off
    assert run(D1, I1, dm1, im1, Tm, 1.0, 255.0, max_depth=2.0)[0] == [1, 0, 0, 0, 0] and run(D1, I1, dm1, im1, Tm, 1.0, 255.0, min_depth=2.0)[0] == [0, 1, 0, 0, 0]


def test_holes_at_each_corner_bad_values_masks_and_non_finite_poses(ctx):
    S = _scene(61, 37, 40, 22, 77)
    S["D"] = np.where(np.isfinite(S["D"]) & (S["D"] > 1) & (S["D"] < 5), S["D"], F(3.0)).astype(F)
    S["Dm"] = np.full_like(S["Dm"], 3.0); S["Im"] = np.where(np.isfinite(S["Im"]) & (S["Im"] >= 0), S["Im"], F(100)).astype(F)
    S["model"] = P.pack_model(S["Dm"], S["Im"])
    on = _loaded(ctx, S, keep_rows=True, max_dist=0.5)
    off = _loaded(ctx, S, keep_rows=False, max_dist=0.5)

    def both(what, D=None, mask=None, T=None, Dm=None, Im=None, Tm=None):
        D = S["D"] if D is None else D; T = S["T"] if T is None else T
        Dm = S["Dm"] if Dm is None else Dm; Im = S["Im"] if Im is None else Im; Tm = S["Tm"] if Tm is None else Tm
        for h in (on, off):
            h.set_model(Dm, Im, S["Km"], Tm)
        want = P.linearise(D, mask, S["I"], S["K4"], T, P.pack_model(Dm, Im), S["Km"], Tm, PRM["min_depth"], PRM["max_depth"], 0.5, PRM["max_diff"])
        _same(on.linearise(D, mask, T), want, what)
        _same(off.linearise(D, mask, T), want, what + ", keep_rows off")         # the stored image changes no sum
        assert np.array_equal(_bits(on.rows()), _bits(want[2])), what + ": rows"
        return want[1], want[2]

    base, rw0 = both("clean")
    assert base[P.USED] > 1000 and base[P.NO_DEPTH] == 0 and base[P.MASKED] == 0
    # one sample in the middle and its cell
    rws, cls = P.rows(S["D"], None, S["I"], S["K4"], S["T"], S["model"], S["Km"], S["Tm"], PRM["min_depth"], PRM["max_depth"], 0.5, PRM["max_diff"])
    assert cls[18, 30] == P.USED
    Pc = np.array([(30 - S["K4"][2]) / S["K4"][0], (18 - S["K4"][3]) / S["K4"][1], 1.0]) * S["D"][18, 30]
    Pm = S["Tm"][:3, :3].astype(np.float64) @ (S["T"][:3, :3].astype(np.float64).T @ (Pc - S["T"][:3, 3])) + S["Tm"][:3, 3]
    x0, y0 = int(np.floor(S["Km"][0] * Pm[0] / Pm[2] + S["Km"][2])), int(np.floor(S["Km"][1] * Pm[1] / Pm[2] + S["Km"][3]))
    for dy in (0, 1):
        for dx in (0, 1):
            for ch, bad in ((0, 0.0), (0, np.nan), (0, np.inf), (0, -3.0), (1, np.nan), (1, np.inf), (1, -np.inf), (1, -1.0)):
                Dm = S["Dm"].copy(); Im = S["Im"].copy()
                (Dm if ch == 0 else Im)[y0 + dy, x0 + dx] = bad
                c, rw = both(f"corner ({dx}, {dy}) channel {ch} = {bad}", Dm=Dm, Im=Im)
                assert not rw[18, 30].any() and c[P.NO_MODEL] > base[P.NO_MODEL] and c[P.USED] < base[P.USED]
    Dm = S["Dm"].copy(); Dm[y0 + 1, x0] = 3.0 + 0.75                              # an occluder at one corner: far
    c, rw = both("a depth step at a corner", Dm=Dm)
    assert not rw[18, 30].any() and c[P.FAR] > base[P.FAR] and c[P.NO_MODEL] == base[P.NO_MODEL]
    bad = S["D"].copy(); bad[3, 4] = np.nan; bad[6, 6] = np.inf; bad[7, 8] = -np.inf; bad[9, 10] = 0.0; bad[11, 12] = 7.5; bad[13, 14] = 0.3; bad[15, 16] = -2.0
    c, _ = both("NaN, Inf, zero, too far, at min_depth, negative", D=bad)
    assert c[P.NO_DEPTH] == 7
    mask = np.zeros(S["D"].shape, np.int32); mask[2:6, 3:9] = -1; mask[20, 20] = 1 << 30
    c, _ = both("a mask", D=bad, mask=mask)
    assert c[P.NO_DEPTH] == 7 and c[P.MASKED] == 25 - 1                          # the NaN at (3, 4) lies under the mask: no depth comes first
    c, _ = both("behind the model's camera", T=A.perturbed(S["T"], (0.0, 0.0, 0.0), (0.0, 180.0, 0.0)))
    assert c[P.NO_MODEL] == 61 * 37
    for bad_v in (np.nan, np.inf, -np.inf):
        for at in (0, 3, 5, 6, 10, 11):
            Tb = S["T"].copy(); Tb.reshape(16)[at] = bad_v
            c, _ = both(f"T[{at}] = {bad_v}", T=Tb)
            assert c[P.USED] == 0
    for at in (2, 7, 9):
        Tb = S["Tm"].copy(); Tb.reshape(16)[at] = np.nan
        c, _ = both(f"Tm[{at}] = NaN", Tm=Tb)
        assert c[P.USED] == 0
    none, _ = both("no depth anywhere", D=np.zeros(S["D"].shape, F))
    assert none.tolist() == [0, 61 * 37, 0, 0, 0]
    sums, _ = on.linearise(np.zeros(S["D"].shape, F), None, S["T"])
    assert not sums.any() and not np.signbit(sums).any()
    on.close(); off.close()


# ---- entry variants ------------------------------------------------------------------------------------------------------------------------------------
def test_host_strided_device_and_frame_sources(ctx):
    import torch
    S = _scene(61, 37, 40, 22, 5)
    W, H = 61, 37
    D, mask, T = S["D"], S["mask"], S["T"]
    want, want_nomask = _want(S), _want(S, mask=False)
    assert want[1][0] > 300 and want[1][2] > 50
    ph = _loaded(ctx, S)
    _same(ph.linearise(D, mask, T), want, "host")
    _same(ph.linearise(D, None, T), want_nomask, "host, no mask")
    wide_d = np.full((H, W + 5), np.nan, F); wide_d[:, :W] = D
    wide_m = np.full((H, W + 3), 9, np.int32); wide_m[:, :W] = mask
    _same(ph.linearise(wide_d[:, :W], wide_m[:, :W], T), want, "strided host")
    dd = torch.from_numpy(D.copy()).cuda(); dm = torch.from_numpy(mask.copy()).cuda(); dwide = torch.from_numpy(wide_d.copy()).cuda(); mwide = torch.from_numpy(wide_m.copy()).cuda()
    torch.cuda.synchronize()
    _same(ph.linearise_raw(dd.data_ptr(), W, dm.data_ptr(), W, True, T), want, "packed device")
    _same(ph.linearise_raw(dwide.data_ptr(), W + 5, mwide.data_ptr(), W + 3, True, T), want, "strided device")
    fi = FrameImages(ctx, W, H)
    fi.upload(D, mask)
    _same(ph.linearise_frame(fi._h, T), want, "frame images")
    assert np.array_equal(_bits(fi.download_depth()), _bits(D))                 # read-only on them
    # the model from device images
    gd = torch.from_numpy(S["Dm"].copy()).cuda(); gi = torch.from_numpy(S["Im"].copy()).cuda()
    torch.cuda.synchronize()
    ph.set_model(np.ones((3, 3), F), np.ones((3, 3), F), S["Km"], S["Tm"])
    ph.set_model_device(gd.data_ptr(), gi.data_ptr(), 40, 22, S["Km"], S["Tm"])
    del gd, gi                                                                   # copied, not borrowed
    assert np.array_equal(_bits(ph.model()), _bits(S["model"]))
    _same(ph.linearise(D, mask, T), want, "model from device images")
    wall, dev = ph.timing()
    assert wall > 0 and dev >= 0
    fi.close(); ph.close()


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("rgb_order", [0, 1])
def test_the_grey_image_from_every_layout(ctx, channels, rgb_order):
    import torch
    W, H = 61, 37
    rng = np.random.default_rng(channels * 2 + rgb_order)
    img = rng.integers(0, 256, (H, W, channels)).astype(np.uint8)
    img[0, :6] = [[0] * channels, [255] * channels, [77] * channels, [1] * channels, [254] * channels, [128] * channels]
    want = P.grey(img, rgb_order)
    if channels > 1:
        assert want[0, :6].tolist() == [0, 255, 77, 1, 254, 128]                # grey stays grey
        assert not np.array_equal(want, P.grey(img, 1 - rgb_order))             # the order matters
    ph = _photo(ctx, W, H, (50.0, 50.0, 30.0, 18.0))
    ph.set_image(img if channels > 1 else img[..., 0], rgb_order)
    assert np.array_equal(_bits(ph.image()), _bits(want)), "packed host"
    wide = np.full((H, W * channels + 7), 201, np.uint8); wide[:, :W * channels] = img.reshape(H, -1)
    ph.set_image(np.zeros((H, W), np.uint8))
    ph.set_image_raw(wide.ctypes.data, W * channels + 7, channels, rgb_order, False)
    assert np.array_equal(_bits(ph.image()), _bits(want)), "strided host"
    t = torch.from_numpy(wide.copy()).cuda(); tp = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    ph.set_image(np.zeros((H, W), np.uint8))
    ph.set_image_raw(t.data_ptr(), W * channels + 7, channels, rgb_order, True)
    assert np.array_equal(_bits(ph.image()), _bits(want)), "strided device"
    ph.set_image(np.zeros((H, W), np.uint8))
    ph.set_image_raw(tp.data_ptr(), W * channels, channels, rgb_order, True)
    assert np.array_equal(_bits(ph.image()), _bits(want)), "packed device"
    ph.close()


def test_keep_as_model_from_arrays_and_from_a_resident_frame(ctx):
    import torch
    S = _scene(61, 37, 40, 22, 9)
    W, H = 61, 37
    D, mask = S["D"], S["mask"]
    Tk = A.perturbed(S["T"], (0.03, 0.0, -0.02), (0.0, 0.5, 0.0))
    want_model = P.keep_as_model(D, mask, S["I"], PRM["min_depth"], PRM["max_depth"])
    want_nomask = P.keep_as_model(D, None, S["I"], PRM["min_depth"], PRM["max_depth"])
    assert (want_model[..., 0] == 0).sum() > (want_nomask[..., 0] == 0).sum() > 0 and np.isfinite(want_model).all()
    ph = _loaded(ctx, S)
    # the next frame: another image and depth against the kept model
    S2 = _scene(61, 37, 40, 22, 10)
    want = P.linearise(S2["D"], S2["mask"], S2["I"], S["K4"], S["T"], want_model, S["K4"], Tk, **PRM)
    assert want[1][0] > 200

    def check(what, model=want_model):
        assert np.array_equal(_bits(ph.model()), _bits(model)), what
        ph.set_image(S2["img"])
        _same(ph.linearise(S2["D"], S2["mask"], S["T"]), P.linearise(S2["D"], S2["mask"], S2["I"], S["K4"], S["T"], model, S["K4"], Tk, **PRM), what)
        ph.set_image(S["img"]); ph.set_model(S["Dm"], S["Im"], S["Km"], S["Tm"])

    ph.keep_as_model(D, mask, Tk); check("host")
    ph.keep_as_model(D, None, Tk); check("host, no mask", want_nomask)
    wide_d = np.full((H, W + 5), np.nan, F); wide_d[:, :W] = D
    wide_m = np.full((H, W + 3), 9, np.int32); wide_m[:, :W] = mask
    ph.keep_as_model(wide_d[:, :W], wide_m[:, :W], Tk); check("strided host")
    dd = torch.from_numpy(D.copy()).cuda(); dm = torch.from_numpy(mask.copy()).cuda(); dwide = torch.from_numpy(wide_d.copy()).cuda()
    torch.cuda.synchronize()
    ph.keep_as_model_raw(dd.data_ptr(), W, dm.data_ptr(), W, True, Tk); check("packed device")
    ph.keep_as_model_raw(dwide.data_ptr(), W + 5, dm.data_ptr(), W, True, Tk); check("strided device")
    fi = FrameImages(ctx, W, H)
    fi.upload(D, mask)
    ph.keep_as_model_frame(fi._h, Tk); check("resident frame")
    assert np.array_equal(_bits(fi.download_depth()), _bits(D))
    fi.close(); ph.close()


# ---- the joint solve, walked through its trace -------------------------------------------------------------------------------------------------------------
def _walk(trace, rep, T_out, photo_lin, geo_lin, weight, min_pixels, geo_min_pixels, max_iterations, eps, what):
    """Every round's sums and counts against the restatement's linearisations AT THE DEVICE'S T; every next T against the restated combine + step from
    those sums, bit for bit (photo_ref.step writes the exponential out in vdo_align_step's order)"""
    assert len(trace) == rep["iterations"] >= 1
    for it, row in enumerate(trace):
        T = row[:16].astype(F).reshape(4, 4)
        assert np.array_equal(T.astype(np.float64).ravel(), row[:16])
        sp, cp = photo_lin(T)[:2]
        _same((row[49:77], row[77:82].astype(np.int64)), (sp, cp), f"{what}, round {it}, photometric")
        if geo_lin is not None:
            sg, cg = geo_lin(T)[:2]
            _same((row[16:44], row[44:49].astype(np.int64)), (sg, cg), f"{what}, round {it}, geometric")
        else:
            sg, cg = None, np.zeros(5, np.int64)
            assert not row[16:49].any() and not np.signbit(row[16:49]).any()
        last = it == len(trace) - 1
        nxt = T_out if last else trace[it + 1][:16].astype(F).reshape(4, 4)
        if cp[0] < min_pixels or (geo_lin is not None and cg[0] < geo_min_pixels):
            status, Tn, xi = 1, T, np.zeros(6)
        else:
            status, Tn, xi, _ = P.step(P.combine(sg, sp, weight), int(cg[0] + cp[0]), 6, T)
        assert np.array_equal(_bits(nxt), _bits(Tn)), f"{what}, round {it}: the step"
        if last:
            assert rep["status"] == status and rep["used_geo"] == cg[0] and rep["used_photo"] == cp[0] and np.array_equal(_bits(rep["xi"]), _bits(xi))
            assert rep["rms_photo_last"] == P._rms(sp[27], int(cp[0])) and rep["rms_geo_last"] == (P._rms(sg[27], int(cg[0])) if sg is not None else 0.0)
            assert status != 0 or (np.abs(xi) <= F(eps)).all() or it + 1 == max_iterations      # why it stopped
        else:
            assert status == 0 and not (np.abs(xi) <= F(eps)).all()
        if it == 0:
            assert rep["rms_photo_first"] == P._rms(sp[27], int(cp[0])) and rep["rms_geo_first"] == (P._rms(sg[27], int(cg[0])) if sg is not None else 0.0)


@pytest.fixture(scope="module")
def wall():
    D, If, T_true, T_init, Dm, Gm, Im = wall_case()
    return dict(D=D, If=If, img=If.astype(np.uint8), T_true=T_true, T_init=T_init, Dm=Dm, Gm=Gm, Im=Im)


@pytest.mark.parametrize("with_geo", [True, False], ids=["joint", "photometric alone"])
def test_a_solve_in_front_of_the_textured_wall_walked_through_its_trace(ctx, wall, with_geo):
    """The CPU test's scene (tests/test_photo_ref.py) on the device, from host images and from a resident frame: the same bits; the CPU test's accuracy
    conditions hold for the device's result."""
    from vdo_slam_amd.align import Aligner
    w = P.WALL
    K4, q = w["K4"], wall
    assert np.array_equal(q["img"].astype(F), q["If"])
    ph = _photo(ctx, w["W"], w["H"], K4, min_depth=0.0, max_depth=10.0, max_dist=w["max_dist"], max_diff=255.0, max_iterations=w["max_iterations"], eps=w["eps"])
    ph.set_image(q["img"]); ph.set_model(q["Dm"], q["Im"], K4, I4)
    al = None
    if with_geo:
        al = Aligner(ctx, w["W"], w["H"], K4, min_depth=0.0, max_depth=10.0, max_dist=w["max_dist"])
        al.set_model(q["Dm"], q["Gm"], K4, I4)
    photo_lin = lambda T: P.linearise(q["D"], None, q["If"], K4, T, P.pack_model(q["Dm"], q["Im"]), K4, I4, 0.0, 10.0, w["max_dist"], 255.0)
    geo_lin = (lambda T: A.linearise(q["D"], None, K4, T, q["Dm"], q["Gm"], K4, I4, 0.0, 10.0, w["max_dist"])) if with_geo else None
    T, rep, trace = ph.solve(al, q["D"], None, WALL_WEIGHT, q["T_init"])
    _walk(trace, rep, T, photo_lin, geo_lin, WALL_WEIGHT, 6, 6, w["max_iterations"], w["eps"], "wall")
    want_T, want_rep, _ = P.solve(photo_lin, geo_lin, WALL_WEIGHT, q["T_init"], 6, 6, w["max_iterations"], w["eps"])
    assert np.array_equal(_bits(T), _bits(want_T)) and rep["iterations"] == want_rep["iterations"] and rep["status"] == want_rep["status"] == 0
    dt0, _ = A.pose_error(q["T_init"], q["T_true"]); dt, _ = A.pose_error(T, q["T_true"])
    assert dt < 0.1 * dt0 and dt < 0.5 * w["Z0"] / K4[0]
    fi = FrameImages(ctx, w["W"], w["H"])
    fi.upload(q["D"], np.zeros(q["D"].shape, np.int32))
    T2, rep2, trace2 = ph.solve_frame(al, fi._h, WALL_WEIGHT, q["T_init"])
    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(_bits(trace), _bits(trace2)) and rep2["iterations"] == rep["iterations"]      # two runs, two sources: the same bits
    fi.close(); ph.close()
    if al is not None:
        al.close()


def test_a_solve_with_a_mask_subsampling_the_iteration_cap_and_both_status_1_rules(ctx, wall):
    from vdo_slam_amd.align import Aligner
    w = P.WALL
    K4, q = w["K4"], wall
    mask = np.zeros(q["D"].shape, np.int32); mask[:, :6] = 2
    geo_args = dict(min_depth=0.0, max_depth=10.0, max_dist=w["max_dist"])
    Tg = A.perturbed(I4, (0.0, 0.0, 0.0), (0.4, -0.3, 0.0))                       # the aligner's model from another pose than the photometric one
    Dg = A.plane_depth([((0.0, 0.0, 1.0), w["Z0"])], Tg, w["W"], w["H"], K4)
    for s, iters, eps, min_px, geo_min, weight, status in ((2, 2, 0.0, 40, 40, 0.02, 0), (3, 12, 1e-4, 40, 40, WALL_WEIGHT, 0), (1, 5, 1e-6, 3000, 6, 0.01, 1), (1, 5, 1e-6, 6, 3000, 0.01, 1)):
        ph = _photo(ctx, w["W"], w["H"], K4, subsample=s, min_pixels=min_px, max_iterations=iters, eps=eps, max_diff=255.0, **geo_args)
        ph.set_image(q["img"]); ph.set_model(q["Dm"], q["Im"], K4, I4)
        al = Aligner(ctx, w["W"], w["H"], K4, subsample=s, min_pixels=geo_min, **geo_args)
        al.set_model(Dg, q["Gm"], K4, Tg)
        photo_lin = lambda T: P.linearise(q["D"], mask, q["If"], K4, T, P.pack_model(q["Dm"], q["Im"]), K4, I4, 0.0, 10.0, w["max_dist"], 255.0, s)
        geo_lin = lambda T: A.linearise(q["D"], mask, K4, T, Dg, q["Gm"], K4, Tg, 0.0, 10.0, w["max_dist"], s)
        T, rep, trace = ph.solve(al, q["D"], mask, weight, q["T_init"])
        _walk(trace, rep, T, photo_lin, geo_lin, weight, min_px, geo_min, iters, eps, f"subsample {s}")
        assert rep["status"] == status
        if status == 1:
            assert rep["iterations"] == 1 and np.array_equal(_bits(T), _bits(q["T_init"])) and not rep["xi"].any() and rep["used_photo"] > 2000 and rep["used_geo"] > 2000
        else:
            assert rep["iterations"] == 2 if iters == 2 else rep["iterations"] < 12
        ph.close(); al.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_keep_the_model(ctx):
    from vdo_slam_amd import align as AL
    from vdo_slam_amd import photo as PH
    L = PH._lib()
    L.vdo_last_error.restype = C.c_char_p
    h = C.c_void_p()
    K4 = (4.0, 4.0, 4.0, 4.0)

    def create(W=8, H=8, c=ctx._h, **kw):
        prm = dict(K4=K4); prm.update(kw)
        pc = PH.params(**prm)
        return L.vdo_photo_create(c, W, H, C.byref(pc), C.byref(h)), L.vdo_last_error().decode()

    nan, inf = float("nan"), float("inf")
    for kw, word in [(dict(W=0), "width"), (dict(H=0), "height"), (dict(K4=(0.0, 4.0, 4.0, 4.0)), "fx"), (dict(K4=(4.0, -1.0, 4.0, 4.0)), "fy"), (dict(K4=(4.0, 4.0, nan, 4.0)), "K[2]"),
                     (dict(K4=(inf, 4.0, 4.0, 4.0)), "K[0]"), (dict(min_depth=-0.1), "min_depth"), (dict(min_depth=nan), "min_depth"), (dict(max_depth=0.0), "max_depth"),
                     (dict(max_depth=inf), "max_depth"), (dict(max_dist=0.0), "max_dist"), (dict(max_dist=nan), "max_dist"), (dict(max_dist=inf), "max_dist"),
                     (dict(max_diff=0.0), "max_diff"), (dict(max_diff=-1.0), "max_diff"), (dict(max_diff=nan), "max_diff"), (dict(max_diff=inf), "max_diff"), (dict(subsample=0), "subsample"),
                     (dict(subsample=9), "subsample"), (dict(min_pixels=5), "min_pixels"), (dict(max_iterations=0), "max_iterations"), (dict(max_iterations=65), "max_iterations"),
                     (dict(eps=-1e-9), "eps"), (dict(eps=nan), "eps"), (dict(keep_rows=2), "keep_rows"), (dict(c=None), "ctx is null")]:
        rc, msg = create(**kw)
        assert rc == -1 and word in msg and not h.value, (kw, rc, msg)
    for W, H in (((1 << 24) + 1, 1), (1 << 14, 1 << 13)):
        rc, msg = create(W=W, H=H)
        assert rc == -4 and not h.value, (W, H, rc, msg)
    pc = PH.params(K4)
    assert L.vdo_photo_create(ctx._h, 8, 8, None, C.byref(h)) == -1 and "params is null" in L.vdo_last_error().decode()
    assert L.vdo_photo_create(ctx._h, 8, 8, C.byref(pc), None) == -1 and "out is null" in L.vdo_last_error().decode()
    for edge in (dict(subsample=8, min_pixels=6, max_iterations=64, eps=0.0, min_depth=0.0, keep_rows=1, max_diff=1e-3), dict(subsample=1, max_iterations=1)):      # the range edges are taken
        rc, msg = create(**edge)
        assert rc == 0 and h.value, (edge, msg)
        assert L.vdo_photo_destroy(h) == 0
        h = C.c_void_p()
    assert L.vdo_photo_create(ctx._h, 8, 8, C.byref(pc), C.byref(h)) == 0 and h.value
    W = H = 8
    D = np.full((H, W), 2.0, F); mask = np.zeros((H, W), np.int32); img = np.arange(64, dtype=np.uint8).reshape(8, 8)
    T = np.ascontiguousarray(np.eye(4, dtype=F).reshape(16)); Km = np.array(K4, F)
    sums = np.full(28, -7.0); counts = np.full(5, -5, np.int64); out = np.full(16, -7.0, F); rep = PH.PhotoReportC(); rep.iterations = -3; trace = np.full(10 * PH.TRACE_ROW, -7.0)
    grey = np.full((H, W), -7.0, F); pairs = np.full((H, W, 2), -7.0, F); wm = C.c_int(-3)
    p = lambda a: a.ctypes.data
    err = lambda: L.vdo_last_error().decode()
    lin = lambda *a: L.vdo_photo_linearise(*a)
    sol = lambda *a: L.vdo_photo_solve(*a)
    ok_lin = (h, p(D), W, p(mask), W, 0, p(T), p(sums), p(counts))
    ok_sol = (h, None, p(D), W, None, 0, 0, 0.01, p(T), p(out), C.addressof(rep), p(trace))
    # nothing set yet
    assert lin(*ok_lin) == -1 and "no image" in err() and sol(*ok_sol) == -1 and "no image" in err()
    assert L.vdo_photo_keep_as_model(h, p(D), W, None, 0, 0, p(T)) == -1 and "no image" in err()
    assert L.vdo_photo_get_image(h, p(grey)) == -1 and L.vdo_photo_get_model(h, p(pairs), C.byref(wm), None) == -1 and L.vdo_photo_get_image(None, p(grey)) == -1
    for args, word in [((None, p(img), W, 1, 0, 0), "handle is null"), ((h, None, W, 1, 0, 0), "image is null"), ((h, p(img), W - 1, 1, 0, 0), "image_stride_bytes"),
                       ((h, p(img), 3 * W - 1, 3, 0, 0), "image_stride_bytes"), ((h, p(img), W, 2, 0, 0), "channels"), ((h, p(img), W, 0, 0, 0), "channels"), ((h, p(img), W, 1, 2, 0), "rgb_order"),
                       ((h, p(img), W, 1, -1, 0), "rgb_order")]:
        assert L.vdo_photo_set_image(*args) == -1 and word in err(), word
    assert lin(*ok_lin) == -1 and "no image" in err()
    assert L.vdo_photo_set_image(h, p(img), W, 1, 0, 0) == 0
    assert lin(*ok_lin) == -1 and "no model" in err() and sol(*ok_sol) == -1 and "no model" in err()
    Dm = np.full((H, W), 2.0, F); Im = np.arange(64, dtype=F).reshape(8, 8); K_fx = np.array([0, 4, 4, 4], F); K_nan = np.array([4, 4, nan, 4], F)
    ok_model = (h, p(Dm), p(Im), W, H, p(Km), p(T), 0)
    for args, word in [((None,) + ok_model[1:], "handle is null"), ((h, None) + ok_model[2:], "depth is null"), ((h, p(Dm), None) + ok_model[3:], "intensity is null"),
                       ((h, p(Dm), p(Im), 0, H, p(Km), p(T), 0), "model_width"), ((h, p(Dm), p(Im), W, -1, p(Km), p(T), 0), "model_height"), ((h, p(Dm), p(Im), W, H, None, p(T), 0), "Km is null"),
                       ((h, p(Dm), p(Im), W, H, p(Km), None, 0), "Tm is null"), ((h, p(Dm), p(Im), W, H, p(K_fx), p(T), 0), "fx"), ((h, p(Dm), p(Im), W, H, p(K_nan), p(T), 0), "Km[2]")]:
        assert L.vdo_photo_set_model(*args) == -1 and word in err(), word
    big = np.ones((H + 1, W), F)
    assert L.vdo_photo_set_model(h, p(big), p(big), W, H + 1, p(Km), p(T), 0) == -4 and L.vdo_photo_set_model(h, p(big), p(big), W, H + 1, p(Km), p(T), 1) == -4
    assert lin(*ok_lin) == -1 and "no model" in err()                             # still no model
    assert L.vdo_photo_set_model(*ok_model) == 0
    assert lin(*ok_lin) == 0 and counts.sum() == W * H and counts[0] > 20
    first = (sums.copy(), counts.copy())
    sums[:] = -7.0; counts[:] = -5
    # every refusal from here on leaves the model as it is
    for args, word in [((None,) + ok_model[1:], "handle is null"), ((h, p(Dm), None) + ok_model[3:], "intensity is null"), ((h, p(Dm), p(Im), W, H, p(K_fx), p(T), 0), "fx")]:
        assert L.vdo_photo_set_model(*args) == -1 and word in err(), word
    assert L.vdo_photo_set_model(h, p(big), p(big), W, H + 1, p(Km), p(T), 0) == -4
    for args, word in [((None, p(D), W, None, 0, 0, p(T)), "handle is null"), ((h, None, W, None, 0, 0, p(T)), "depth is null"), ((h, p(D), W - 1, None, 0, 0, p(T)), "depth_stride"),
                       ((h, p(D), W, p(mask), W - 1, 0, p(T)), "mask_stride"), ((h, p(D), W, None, 0, 0, None), "T is null")]:
        assert L.vdo_photo_keep_as_model(*args) == -1 and word in err(), word
    small = FrameImages(ctx, W - 1, H)
    assert L.vdo_photo_keep_as_model_frame(h, small._h, p(T)) == -1 and "frame is" in err() and L.vdo_photo_keep_as_model_frame(h, None, p(T)) == -1
    assert L.vdo_photo_keep_as_model_frame(None, small._h, p(T)) == -1
    for args, word in [((None,) + ok_lin[1:], "handle is null"), ((h, None) + ok_lin[2:], "depth is null"), ((h, p(D), W - 1) + ok_lin[3:], "depth_stride"),
                       ((h, p(D), W, p(mask), W - 1) + ok_lin[5:], "mask_stride"), (ok_lin[:6] + (None, p(sums), p(counts)), "T is null"), (ok_lin[:7] + (None, p(counts)), "sums is null"),
                       (ok_lin[:8] + (None,), "counts is null")]:
        assert lin(*args) == -1 and word in err(), word
    al_other = AL.Aligner(ctx, W - 1, H, K4)
    al_nomodel = AL.Aligner(ctx, W, H, K4)
    for args, word in [((None,) + ok_sol[1:], "handle is null"), (ok_sol[:2] + (None,) + ok_sol[3:], "depth is null"), (ok_sol[:3] + (W - 1,) + ok_sol[4:], "depth_stride"),
                       (ok_sol[:4] + (p(mask), W - 1) + ok_sol[6:], "mask_stride"), (ok_sol[:8] + (None,) + ok_sol[9:], "T_init is null"), (ok_sol[:9] + (None,) + ok_sol[10:], "T_out is null"),
                       (ok_sol[:7] + (0.0,) + ok_sol[8:], "weight"), (ok_sol[:7] + (-0.01,) + ok_sol[8:], "weight"), (ok_sol[:7] + (nan,) + ok_sol[8:], "weight"),
                       (ok_sol[:7] + (inf,) + ok_sol[8:], "weight"), ((h, al_other._h) + ok_sol[2:], "geo is for"), ((h, al_nomodel._h) + ok_sol[2:], "geo has no model")]:
        assert sol(*args) == -1 and word in err(), word
    assert L.vdo_photo_linearise_frame(h, small._h, p(T), p(sums), p(counts)) == -1 and "frame is" in err()
    assert L.vdo_photo_linearise_frame(h, None, p(T), p(sums), p(counts)) == -1 and L.vdo_photo_linearise_frame(None, small._h, p(T), p(sums), p(counts)) == -1
    assert L.vdo_photo_solve_frame(h, None, small._h, 0.01, p(T), p(out), None, None) == -1 and L.vdo_photo_solve_frame(h, None, None, 0.01, p(T), p(out), None, None) == -1
    small.close(); al_other.close(); al_nomodel.close()
    rows = np.full((H, W, 8), -7.0, F)
    assert L.vdo_photo_get_rows(h, p(rows)) == -1 and "keep_rows" in err() and L.vdo_photo_get_rows(None, p(rows)) == -1 and L.vdo_photo_get_model(None, p(pairs), None, None) == -1
    assert L.vdo_photo_get_image(h, None) == -1
    assert (sums == -7).all() and (counts == -5).all() and (out == -7).all() and rep.iterations == -3 and (trace == -7).all() and (rows == -7).all() and (grey == -7).all()
    assert (pairs == -7).all() and wm.value == -3
    ms = (C.c_double * 2)()
    assert L.vdo_photo_last_timing(h, None) == -1 and L.vdo_photo_last_timing(None, ms) == -1 and L.vdo_photo_destroy(None) == 0
    # the model and the image are intact
    assert lin(*ok_lin) == 0
    _same((sums, counts), first, "after the refusals")
    assert L.vdo_photo_get_model(h, p(pairs), C.byref(wm), None) == 0 and wm.value == W and np.array_equal(pairs, P.pack_model(Dm, Im))
    assert sol(h, None, p(D), W, None, 0, 0, 0.01, p(T), p(out), None, None) == 0                        # report and trace are optional
    assert L.vdo_photo_destroy(h) == 0
    kr = _photo(ctx, W, H, K4, keep_rows=True)
    with pytest.raises(Exception, match="no linearisation"):
        kr.rows()
    kr.close()
