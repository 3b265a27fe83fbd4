"""GPU: the device stereo matcher (vdo_stereo_*, csrc/stereo.hip) against the NumPy restatement of its contract (tests/stereo_ref.py).
Integer results throughout: every comparison is array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import stereo_ref as R

pytestmark = pytest.mark.gpu

STAGES = ("census_l", "census_r", "cost", "aggregated", "disparity256", "n_valid")


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _matcher(ctx, H, W, **prm):
    from vdo_slam_amd.stereo import StereoMatcher
    return StereoMatcher(ctx, W, H, **prm)


def _device_stages(m, left, right):
    out, n = m.compute(left, right)
    return dict(census_l=m.census(0), census_r=m.census(1), cost=m.cost(), aggregated=m.aggregated(), disparity256=out, n_valid=n)


def _same(got, want, what=""):
    for k in STAGES:
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    assert got["disparity256"].dtype == np.float32


@functools.lru_cache(maxsize=None)
def _scene_and_ref(H, W, D, paths=8):
    """A built scene of one size and the restatement's stages: computed once, shared"""
    left, right, _, _ = R.scene(H, W, D, seed=1000 * H + W)
    return left, right, R.stages(left, right, max_disparity=D, paths=paths)


# ---- the four stage pins across sizes ---------------------------------------------------------------------------------------------
SIZES = [(40, 96, 32), (37, 131, 48), (48, 160, 64), (24, 70, 128), (16, 300, 256), (64, 416, 128), (12, 20, 32), (1, 1, 16), (1, 50, 16), (50, 1, 16), (7, 9, 16)]


@pytest.mark.parametrize("H,W,D", SIZES)
def test_every_stage_equals_the_restatement(ctx, H, W, D):
    left, right, want = _scene_and_ref(H, W, D)
    m = _matcher(ctx, H, W, max_disparity=D)
    _same(_device_stages(m, left, right), want, f"{H}x{W}x{D}")
    wall, dev = m.last_timing()
    assert wall > 0 and dev > 0
    m.close()


@pytest.mark.parametrize("H,W,D", [(37, 131, 48), (12, 20, 32), (16, 300, 256), (1, 50, 16), (50, 1, 16)])
def test_four_paths_across_sizes(ctx, H, W, D):
    left, right, want = _scene_and_ref(H, W, D, 4)
    m = _matcher(ctx, H, W, max_disparity=D, paths=4)
    _same(_device_stages(m, left, right), want, f"{H}x{W}x{D} paths 4")
    m.close()


# ---- the parameter grid on one small scene ---------------------------------------------------------------------------------------
GRID_SCENE = (37, 131, 48)


@functools.lru_cache(maxsize=None)
def _grid_volume(paths, p1, p2):
    left, right, _, _ = R.scene(*GRID_SCENE, seed=3)
    st = R.stages(left, right, max_disparity=GRID_SCENE[2], paths=paths, p1=p1, p2=p2)
    return left, right, st


@pytest.mark.parametrize("paths,p1,p2", [(4, 10, 120), (8, 10, 120), (8, 40, 40), (4, 1, 1), (8, 10, 1000), (4, 1000, 1000)])
def test_penalties_and_paths(ctx, paths, p1, p2):
    left, right, want = _grid_volume(paths, p1, p2)
    H, W, D = GRID_SCENE
    m = _matcher(ctx, H, W, max_disparity=D, paths=paths, p1=p1, p2=p2)
    _same(_device_stages(m, left, right), want, f"paths {paths} P1 {p1} P2 {p2}")
    m.close()


@pytest.mark.parametrize("subpixel", [0, 1])
@pytest.mark.parametrize("lr", [-1, 0, 1])
@pytest.mark.parametrize("uniqueness", [0, 5, 99])
def test_selection_filters(ctx, uniqueness, lr, subpixel):
    left, right, st = _grid_volume(8, 10, 120)
    H, W, D = GRID_SCENE
    want = R.select(st["aggregated"], uniqueness, lr, subpixel)
    m = _matcher(ctx, H, W, max_disparity=D, uniqueness=uniqueness, lr_max_diff=lr, subpixel=subpixel)
    out, n = m.compute(left, right)
    assert np.array_equal(out, want) and n == np.count_nonzero(want)
    m.close()


def test_the_grid_scene_exercises_every_rule():
    """(no device: what the scene above makes the selection kernel decide)"""
    _, _, st = _grid_volume(8, 10, 120)
    S = st["aggregated"]
    plain = R.select(S, 0, -1, 0)
    assert 0 < np.count_nonzero(R.select(S, 5, -1, 0)) < np.count_nonzero(plain)            # uniqueness rejects some, not all
    assert 0 < np.count_nonzero(R.select(S, 0, 0, 0)) < np.count_nonzero(R.select(S, 0, 1, 0)) < np.count_nonzero(plain)      # so does each LR bound
    sub = R.select(S, 0, -1, 1)
    assert ((sub - plain) > 0).any() and ((sub - plain) < 0).any()
    dstar = S.astype(np.int64).argmin(axis=2)
    assert (dstar == 0).any()                                                                # rule (a)
    srt = np.sort(S, axis=2)
    assert (srt[..., 0] == srt[..., 1]).any()                                                # ties of the minimum


# ---- hand-made cases through the device -------------------------------------------------------------------------------------------
def test_constant_images_have_no_valid_pixel(ctx):
    img = np.full((10, 30), 77, np.uint8)
    m = _matcher(ctx, 10, 30, max_disparity=16)
    out, n = m.compute(img, img)
    assert n == 0 and not out.any()
    assert not m.census(0).any() and not m.cost()[:, 15:].any()
    m.close()


def test_shift_by_five(ctx):
    base = np.random.default_rng(0).integers(0, 256, (24, 70)).astype(np.uint8)
    left, right = np.ascontiguousarray(base[:, :64]), np.ascontiguousarray(base[:, 5:69])
    m = _matcher(ctx, 24, 64, max_disparity=16, subpixel=0)
    out, n = m.compute(left, right)
    assert (out[:, 5 + 16:] == 5 * 256).all()
    want, n_want = R.compute(left, right, max_disparity=16, subpixel=0)
    assert np.array_equal(out, want) and n == n_want
    m.close()


def test_mostly_flat_images_tie_often(ctx):
    """A flat image with a few bars and dots: runs of equal census words, so equal sums across d and along the LR diagonal - the lowest d must win on both"""
    rng = np.random.default_rng(5)
    left = np.full((20, 90), 9, np.uint8)
    cols = rng.choice(90, 12, replace=False)
    left[:, cols] = rng.integers(0, 256, 12).astype(np.uint8)[None]
    left[rng.integers(0, 20, 15), rng.integers(0, 90, 15)] = 255
    right = np.roll(left, -7, axis=1)
    for D, sub in ((16, 1), (32, 0)):
        want = R.stages(left, right, max_disparity=D, subpixel=sub, uniqueness=0)
        srt = np.sort(want["aggregated"], axis=2)
        assert (srt[..., 0] == srt[..., 1]).mean() > 0.05 and want["n_valid"] > 0
        m = _matcher(ctx, 20, 90, max_disparity=D, subpixel=sub, uniqueness=0)
        _same(_device_stages(m, left, right), want, f"binary D {D}")
        m.close()


def test_last_disparity_wins(ctx):
    """A shift of D - 1: d* = D - 1 takes no sub-pixel offset"""
    base = np.random.default_rng(6).integers(0, 256, (12, 100)).astype(np.uint8)
    left, right = np.ascontiguousarray(base[:, :80]), np.ascontiguousarray(base[:, 15:95])
    want = R.stages(left, right, max_disparity=16)
    assert (want["disparity256"][:, 40:] == 15 * 256).mean() > 0.9
    m = _matcher(ctx, 12, 80, max_disparity=16)
    _same(_device_stages(m, left, right), want, "d* = D - 1")
    m.close()


# ---- strides, device / host inputs and outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dev", [False, True])
@pytest.mark.parametrize("src_dev", [False, True])
def test_padded_strides_and_memory_spaces(ctx, src_dev, out_dev):
    import torch
    H, W, D = 37, 131, 48
    left, right, want = _scene_and_ref(H, W, D)
    sl, sr = W + 13, W + 1                                       # two different odd paddings
    bufl = np.full((H, sl), 255, np.uint8); bufl[:, :W] = left
    bufr = np.full((H, sr), 0, np.uint8); bufr[:, :W] = right
    m = _matcher(ctx, H, W, max_disparity=D)
    keep = []
    if src_dev:
        tl, tr = torch.from_numpy(bufl).cuda(), torch.from_numpy(bufr).cuda()
        keep += [tl, tr]
        pl, pr = tl.data_ptr(), tr.data_ptr()
    else:
        pl, pr = bufl.ctypes.data, bufr.ctypes.data
    if out_dev:
        to = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda")
        po = to.data_ptr()
    else:
        ho = np.full((H, W), -1.0, np.float32)
        po = ho.ctypes.data
    torch.cuda.synchronize()
    n = m.compute_raw(pl, sl, pr, sr, src_dev, po, out_dev)
    out = to.cpu().numpy() if out_dev else ho
    assert np.array_equal(out, want["disparity256"]) and n == want["n_valid"]
    assert np.array_equal(m.census(0), want["census_l"]) and np.array_equal(m.census(1), want["census_r"])
    m.close()


def test_two_computes_on_one_handle_share_no_state(ctx):
    H, W, D = 40, 96, 32
    left, right, want = _scene_and_ref(H, W, D)
    l2, r2, _, _ = R.scene(H, W, D, seed=77)
    want2 = R.stages(l2, r2, max_disparity=D)
    m = _matcher(ctx, H, W, max_disparity=D)
    _same(_device_stages(m, left, right), want, "first")
    _same(_device_stages(m, l2, r2), want2, "second")
    _same(_device_stages(m, left, right), want, "first again")
    m.close()


def test_output_scale_is_one_multiply(ctx):
    H, W, D = 40, 96, 32
    left, right, want = _scene_and_ref(H, W, D)
    m = _matcher(ctx, H, W, max_disparity=D)
    for scale in (0.5, 4.0, 1.0, 1000.0 / 256.0):
        m.set_output_scale(scale)
        out, n = m.compute(left, right)
        assert np.array_equal(out, want["disparity256"] * np.float32(scale)) and n == want["n_valid"]
    from vdo_slam_amd import _capi as K
    for bad in (0.0, -1.0, float("nan"), 1e9):
        with pytest.raises(K.VdoError, match="scale"):
            m.set_output_scale(bad)
    m.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word,code", [
    (dict(W=0), "width", -1), (dict(H=0), "height", -1), (dict(W=-5), "width", -1),
    (dict(max_disparity=0), "max_disparity", -1), (dict(max_disparity=24), "max_disparity", -1), (dict(max_disparity=272), "max_disparity", -1), (dict(max_disparity=8), "max_disparity", -1),
    (dict(paths=5), "paths", -1), (dict(paths=0), "paths", -1), (dict(paths=16), "paths", -1),
    (dict(p1=0), "p1", -1), (dict(p1=50, p2=49), "p1", -1), (dict(p2=1001), "p2", -1), (dict(p1=1001, p2=1001), "p2", -1),
    (dict(uniqueness=-1), "uniqueness", -1), (dict(uniqueness=100), "uniqueness", -1),
    (dict(lr_max_diff=-2), "lr_max_diff", -1),
    (dict(W=4096, H=4097, max_disparity=16), "2^28", -4), (dict(W=1 << 14, H=1 << 10, max_disparity=32), "2^28", -4),
])
def test_create_refusals(ctx, kw, word, code):
    from vdo_slam_amd import _capi as K
    kw = dict(kw)
    W, H = kw.pop("W", 32), kw.pop("H", 16)
    with pytest.raises(K.VdoError, match=word.replace("^", r"\^")) as e:
        _matcher(ctx, H, W, **{**dict(max_disparity=16), **kw})
    assert e.value.code == code


def test_compute_refusals_write_nothing(ctx):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd import stereo
    H, W = 16, 32
    m = _matcher(ctx, H, W, max_disparity=16)
    img = np.zeros((H, W), np.uint8)
    out = np.full((H, W), -7.0, np.float32)
    for args, word in (((0, W, img.ctypes.data, W), "left"), ((img.ctypes.data, W, 0, W), "right"), ((img.ctypes.data, W - 1, img.ctypes.data, W), "left_stride"),
                       ((img.ctypes.data, W, img.ctypes.data, W - 1), "right_stride"), ((img.ctypes.data, 0, img.ctypes.data, W), "left_stride")):
        with pytest.raises(K.VdoError, match=word) as e:
            m.compute_raw(*args, False, out.ctypes.data, False)
        assert e.value.code == -1 and (out == -7.0).all()
    L = stereo._lib()
    n = C.c_int32(-7)
    assert L.vdo_stereo_compute(m._h, img.ctypes.data, W, img.ctypes.data, W, 0, None, 0, C.byref(n)) == -1 and n.value == -7
    assert L.vdo_stereo_compute(m._h, img.ctypes.data, W, img.ctypes.data, W, 0, out.ctypes.data, 0, None) == -1 and (out == -7.0).all()
    assert L.vdo_stereo_compute(None, img.ctypes.data, W, img.ctypes.data, W, 0, out.ctypes.data, 0, C.byref(n)) == -1 and (out == -7.0).all()
    with pytest.raises(K.VdoError, match="no vdo_stereo_compute"):                     # inspection before the first compute
        m.cost()
    m.compute(img, img)
    with pytest.raises(K.VdoError, match="which"):
        m.census(2)
    assert L.vdo_stereo_create(ctx._h, W, H, None, C.byref(C.c_void_p())) == -1
    m.close()


# ---- composition with K1 ----------------------------------------------------------------------------------------------------------
def test_device_output_feeds_k1(ctx):
    import torch
    from tests import image_kernels_ref as IR
    from vdo_slam_amd.frontend import FrameImages
    H, W, D = 48, 160, 64
    left, right, want = _scene_and_ref(H, W, D)
    m = _matcher(ctx, H, W, max_disparity=D)
    disp = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    flow = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    mask = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = m.compute_raw(left.ctypes.data, W, right.ctypes.data, W, False, disp.data_ptr(), True)
    assert n == want["n_valid"] and 0 < n < H * W
    bf = 387.5744
    im = FrameImages(ctx, W, H)
    im.ingest_device(disp.data_ptr(), flow.data_ptr(), mask.data_ptr(), bf, 256.0, True)
    assert np.array_equal(im.download_depth(), IR.depth_preprocess(want["disparity256"], bf, 256.0))        # zeros included
    # another DepthMapFactor: the output scale factor / 256 keeps the composition exact for a power of two
    m.set_output_scale(1024.0 / 256.0)
    m.compute_raw(left.ctypes.data, W, right.ctypes.data, W, False, disp.data_ptr(), True)
    im.ingest_device(disp.data_ptr(), flow.data_ptr(), mask.data_ptr(), bf, 1024.0, True)
    assert np.array_equal(im.download_depth(), IR.depth_preprocess(want["disparity256"], bf, 256.0))
    m.close()


# ---- host classes -----------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_stereomatcher_class_equals_the_c_entry(ctx):
    from vdo_slam_amd import _capi as K
    host = K.load_host_lib()
    host.host_stereo_compute.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    H, W, D = 37, 131, 48
    left, right, want = _scene_and_ref(H, W, D)
    m = _matcher(ctx, H, W, max_disparity=D, paths=4, uniqueness=10, lr_max_diff=0)
    out, n = m.compute(left, right)
    m.close()
    prm = np.array([D, 10, 120, 4, 10, 0, 1], np.int32)
    padded = np.zeros((H, W + 5), np.uint8); padded[:, :W] = left                      # (a cv::Mat with a row step of its own)
    got = np.full((H, W), -1.0, np.float32)
    assert host.host_stereo_compute(_ptr(padded), W + 5, _ptr(right), W, W, H, _ptr(prm), _ptr(got)) == n
    assert np.array_equal(got, out)
    prm[0] = 20                                                                         # a refusal surfaces as a failure, not as an exit
    assert host.host_stereo_compute(_ptr(left), W, _ptr(right), W, W, H, _ptr(prm), _ptr(got)) == -1


def test_trackstereo_equals_trackrgbd_on_the_device_disparity(ctx, tmp_path):
    """System(STEREO).TrackStereo over 3 frames against System(RGBD).TrackRGBD fed the disparity vdo_stereo_compute returned for the same pairs"""
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.system import System, write_settings
    W, H, n_frames = synth.KITTI_W, synth.KITTI_H, 3
    cfg = write_settings(tmp_path / "k.yaml", W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    assert SF.DEPTH_MAP_FACTOR == 256
    Ts = SQ.camera_poses(n_frames); objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(n_frames)]
    rights = []
    for k, fr in enumerate(frames):                              # the right image: noise under the forward warp of the left one by the true disparity
        disp = np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64)
        right = np.random.default_rng(500 + k).integers(0, 256, (H, W)).astype(np.uint8)
        R.warp_right(fr["gray"], disp, right)
        rights.append(right)
    rows = np.array([[0, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in (1, 2, 3)], np.float32)
    s = System(cfg, sensor="stereo")
    poses = [s.track_stereo(fr["gray"], rights[k], fr["flow"], fr["mask"].copy(), rows, n_images=n_frames) for k, fr in enumerate(frames)]
    depth_stereo = s.frame_images(W, H)[0]
    s.close()
    assert all(T is not None for T in poses)
    m = _matcher(ctx, H, W)                                      # the settings file has no Stereo.* key: the defaults
    disps = [m.compute(fr["gray"], rights[k]) for k, fr in enumerate(frames)]
    m.close()
    assert all(n > 0.5 * W * H for _, n in disps)                # most of the image has a disparity
    s = System(cfg)
    want = [s.track_rgbd(fr["gray"], disps[k][0].copy(), fr["flow"], fr["mask"].copy(), rows, n_images=n_frames) for k, fr in enumerate(frames)]
    depth_rgbd = s.frame_images(W, H)[0]
    s.close()
    for k in range(n_frames):
        assert np.array_equal(poses[k], want[k]), k
    assert np.array_equal(depth_stereo, depth_rgbd)
    assert not np.array_equal(poses[-1], np.eye(4, dtype=np.float32))
