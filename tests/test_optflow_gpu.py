"""GPU: the device dense optical-flow matcher (vdo_optflow_*, csrc/optflow.hip) against the NumPy restatement of its contract
(tests/optflow_ref.py), stage by stage.  Integer results throughout: every comparison is array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import optflow_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _matcher(ctx, H, W, **prm):
    from vdo_slam_amd.optflow import FlowMatcher
    return FlowMatcher(ctx, W, H, **prm)


def _check_stages(m, want, what=""):
    """Everything the handle can show of its last compute against the restatement's stages"""
    L = m.params.levels
    sizes = R.level_sizes(m.width, m.height, L)
    for l in range(L):
        assert m.level_size(l) == sizes[l], f"{what}: size of level {l}"
        for which in (0, 1):
            assert np.array_equal(m.pyramid(which, l), want[f"pyramid{which}"][l]), f"{what}: pyramid {which} level {l}"
            assert np.array_equal(m.census(which, l), want[f"census{which}"][l]), f"{what}: census {which} level {l}"
    for l in range(L - 1, -1, -1):                               # coarse to fine: the first level that differs is the one named
        assert np.array_equal(m.level_flow(0, l), want["forward"][l]), f"{what}: forward flow level {l}"
        if want["backward"] is not None:
            assert np.array_equal(m.level_flow(1, l), want["backward"][l]), f"{what}: backward flow level {l}"


def _same(m, im0, im1, want, what=""):
    flow, valid, n = m.compute(im0, im1)
    _check_stages(m, want, what)
    assert flow.dtype == np.float32 and np.array_equal(flow, want["flow"]), f"{what}: flow"
    assert np.array_equal(valid, want["valid"]), f"{what}: valid"
    assert n == want["n_valid"], f"{what}: n_valid"


def _noise_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)


def _moved_pair(H, W, seed):
    """Smoothed noise, the second image moved by (2, -1) with wrap-around and a patch of fresh noise: flows, occlusions and borders at every size"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (H, W)).astype(np.float64)
    a = ((t + np.roll(t, 1, 1) + np.roll(t, 1, 0) + np.roll(t, (1, 1), (0, 1))) / 4).astype(np.uint8)
    b = np.roll(a, (-1, 2), (0, 1)).copy()
    b[H // 3:H // 3 + max(1, H // 4), W // 2:W // 2 + max(1, W // 5)] = rng.integers(0, 256, (max(1, H // 4), max(1, W // 5)))[:H - H // 3, :W - W // 2]
    return a, b


# ---- every stage across sizes (W x H): tiles, halos and the ceil(/2) rule; 65 and 131 are two search tiles / two pyramid regions plus a remainder --
SIZES = [(1, 1), (2, 1), (3, 3), (7, 5), (9, 7), (33, 9), (64, 16), (65, 17), (96, 64), (131, 67), (129, 9)]


@functools.lru_cache(maxsize=None)
def _moved_and_ref(W, H):
    a, b = _moved_pair(H, W, seed=1000 * H + W)
    return a, b, R.stages(a, b)


@pytest.mark.parametrize("W,H", SIZES)
def test_every_stage_equals_the_restatement(ctx, W, H):
    a, b, want = _moved_and_ref(W, H)
    m = _matcher(ctx, H, W)
    _same(m, a, b, want, f"{W}x{H}")
    wall, dev = m.timing()
    assert wall > 0 and dev > 0
    m.close()


# ---- the parameter grid: every value of every parameter at both sizes, r = 4 with w = 4 among them; noise pairs (ties are frequent at w = 0) ----
GRID = {
    (65, 17): [(1, 1, 0, 0, -1, 0), (2, 2, 1, 1, 0, 1), (7, 3, 2, 1, 1, 1), (3, 4, 4, 1, 3, 1), (3, 4, 0, 0, 1, 0), (2, 1, 4, 1, -1, 1)],
    (96, 64): [(1, 2, 2, 0, 1, 1), (2, 1, 4, 1, 3, 0), (3, 4, 0, 1, 0, 1), (7, 3, 1, 0, -1, 1), (3, 2, 2, 1, 1, 1)],
}
GRID_CASES = [(W, H) + p for (W, H), ps in GRID.items() for p in ps]


def _prm(L, r, w, med, fb, sub):
    return dict(levels=L, radius=r, window=w, median=med, fb_max_diff=fb, subpixel=sub)


def test_the_grid_covers_every_value():
    for ps in GRID.values():
        cols = list(zip(*ps))
        assert set(cols[0]) == {1, 2, 3, 7} and set(cols[1]) == {1, 2, 3, 4} and set(cols[2]) == {0, 1, 2, 4}
        assert set(cols[3]) == {0, 1} and set(cols[4]) == {-1, 0, 1, 3} and set(cols[5]) == {0, 1}
    assert any(p[1] == 4 and p[2] == 4 for ps in GRID.values() for p in ps)


@pytest.mark.parametrize("W,H,L,r,w,med,fb,sub", GRID_CASES)
def test_parameter_grid(ctx, W, H, L, r, w, med, fb, sub):
    a, b = _noise_pair(H, W, seed=W + 7 * L + r)
    want = R.stages(a, b, **_prm(L, r, w, med, fb, sub))
    m = _matcher(ctx, H, W, **_prm(L, r, w, med, fb, sub))
    _same(m, a, b, want, f"{W}x{H} L{L} r{r} w{w} median{med} fb{fb} sub{sub}")
    m.close()


def test_noise_at_window_zero_ties():
    """(no device: what the w = 0 cases above make the argmin decide)"""
    a, b = _noise_pair(17, 65, seed=65 + 7 + 1)
    A = R.block_costs(R.census(a), R.census(b), np.zeros((17, 65, 2), np.int64), 1, 0)
    srt = np.sort(A, axis=0)
    assert (srt[0] == srt[1]).mean() > 0.05


# ---- contents ----------------------------------------------------------------------------------------------------------------------
def test_constant_pair(ctx):
    a = np.full((17, 65), 131, np.uint8)
    m = _matcher(ctx, 17, 65, levels=3, radius=4, window=1)
    flow, valid, n = m.compute(a, a)
    assert not flow.any() and valid.all() and n == 17 * 65
    _check_stages(m, R.stages(a, a, levels=3, radius=4, window=1), "constant")
    m.close()


@pytest.mark.parametrize("case,seed", [("i", 0), ("ii", 1), ("iii", 2)])
def test_two_motion_scene(ctx, case, seed):
    from tests.test_optflow_ref import CASES
    I0, I1, _ = R.two_motion_pair(seed, *CASES[case])
    prm = dict(levels=3, radius=2, window=2, median=1, fb_max_diff=1, subpixel=1)
    want = R.stages(I0, I1, **prm)
    assert 0 < want["n_valid"] < I0.size and (want["flow"] != np.rint(want["flow"])).any()
    m = _matcher(ctx, 64, 96, **prm)
    _same(m, I0, I1, want, f"two motions ({case})")
    m.close()


def test_shift_beyond_the_search_range(ctx):
    """A shift of 20 with a range of 1 * (2^2 - 1) = 3: whatever the search settles on, most pixels fail the check, and a second matcher whose priors
    are pushed far outside the image (range 4 * 127 on a 40-pixel image) walks the clamp"""
    I0, I1 = R.shifted_pair(20, 0, H=24, W=40)
    for prm in (dict(levels=2, radius=1, window=2, fb_max_diff=0), dict(levels=7, radius=4, window=1, fb_max_diff=0)):
        want = R.stages(I0, I1, **prm)
        m = _matcher(ctx, 24, 40, **prm)
        _same(m, I0, I1, want, f"beyond the range {prm}")
        m.close()
    want = R.stages(I0, I1, levels=2, radius=1, window=2, fb_max_diff=0)
    assert want["n_valid"] < 0.5 * I0.size
    far = R.stages(I0, I1, levels=7, radius=4, window=1, fb_max_diff=0)
    xs = np.arange(40)[None, :] + far["forward"][0][..., 0]
    assert ((xs < 0) | (xs >= 40)).any()                         # targets outside the image occur


def test_flow_leaving_the_image(ctx):
    """True flow (-5, 0): the five left columns move out through the border and must come out invalid or wrong, never out of bounds"""
    I0, I1 = R.shifted_pair(-5, 0, H=32, W=48)
    want = R.stages(I0, I1, levels=3)
    assert (want["forward"][0][8:-8, 16:-8] == (-5, 0)).all(axis=-1).mean() > 0.99
    assert want["valid"][:, :5].mean() < want["valid"][:, 8:].mean()
    m = _matcher(ctx, 32, 48, levels=3)
    _same(m, I0, I1, want, "leaving")
    m.close()


# ---- strides, device / host inputs and outputs, valid = NULL -----------------------------------------------------------------------------
@pytest.mark.parametrize("out_dev", [False, True])
@pytest.mark.parametrize("src_dev", [False, True])
def test_padded_strides_and_memory_spaces(ctx, src_dev, out_dev):
    import torch
    W, H = 65, 17
    a, b, want = _moved_and_ref(W, H)
    s0, s1 = W + 13, W + 1
    buf0 = np.full((H, s0), 255, np.uint8); buf0[:, :W] = a
    buf1 = np.full((H, s1), 0, np.uint8); buf1[:, :W] = b
    m = _matcher(ctx, H, W)
    keep = []
    if src_dev:
        t0, t1 = torch.from_numpy(buf0).cuda(), torch.from_numpy(buf1).cuda()
        keep += [t0, t1]
        p0, p1 = t0.data_ptr(), t1.data_ptr()
    else:
        p0, p1 = buf0.ctypes.data, buf1.ctypes.data
    if out_dev:
        tf = torch.full((H, W, 2), -1.0, dtype=torch.float32, device="cuda")
        tv = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
        pf, pv = tf.data_ptr(), tv.data_ptr()
    else:
        hf = np.full((H, W, 2), -1.0, np.float32); hv = np.full((H, W), 7, np.uint8)
        pf, pv = hf.ctypes.data, hv.ctypes.data
    torch.cuda.synchronize()
    n = m.compute_raw(p0, s0, p1, s1, src_dev, pf, pv, out_dev)
    flow, valid = (tf.cpu().numpy(), tv.cpu().numpy()) if out_dev else (hf, hv)
    assert np.array_equal(flow, want["flow"]) and np.array_equal(valid, want["valid"]) and n == want["n_valid"]
    _check_stages(m, want, "strided")
    # valid = NULL: the flow and the count as before, nothing else written
    if out_dev:
        tf.fill_(-1.0); tv.fill_(7); torch.cuda.synchronize()
    else:
        hf.fill(-1.0); hv.fill(7)
    n = m.compute_raw(p0, s0, p1, s1, src_dev, pf, None, out_dev)
    flow, valid = (tf.cpu().numpy(), tv.cpu().numpy()) if out_dev else (hf, hv)
    assert np.array_equal(flow, want["flow"]) and n == want["n_valid"] and (valid == 7).all()
    m.close()


def test_the_handles_own_device_images(ctx):
    """vdo_optflow_device_images: a host compute leaves the pair in the handle's staging images; passing those as a device pair reads them in place"""
    import torch
    W, H = 33, 9
    a, b, want = _moved_and_ref(W, H)
    a2, b2 = _noise_pair(H, W, seed=5)
    m = _matcher(ctx, H, W)
    d0, d1, df, dv = m.device_images()
    assert d0 and d1 and df and dv and len({d0, d1, df, dv}) == 4
    m.compute(a2, b2)
    m.compute(a, b)                                              # the staging images now hold (a, b)
    tf = torch.full((H, W, 2), -1.0, dtype=torch.float32, device="cuda")
    tv = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = m.compute_raw(d0, W, d1, W, True, tf.data_ptr(), tv.data_ptr(), True)
    assert np.array_equal(tf.cpu().numpy(), want["flow"]) and np.array_equal(tv.cpu().numpy(), want["valid"]) and n == want["n_valid"]
    assert m.compute_raw(d0, W, d1, W, True, df, dv, True) == want["n_valid"]           # outputs into the handle's own images
    _check_stages(m, want, "own images")
    m.close()


def test_two_computes_on_one_handle_share_no_state(ctx):
    W, H = 96, 64
    a, b, want = _moved_and_ref(W, H)
    a2, b2 = _noise_pair(H, W, seed=77)
    want2 = R.stages(a2, b2)
    m = _matcher(ctx, H, W)
    _same(m, a, b, want, "first")
    _same(m, a2, b2, want2, "second")
    _same(m, a, b, want, "first again")
    m.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word,code", [
    (dict(W=0), "width", -1), (dict(H=0), "height", -1), (dict(W=-5), "width", -1),
    (dict(levels=0), "levels", -1), (dict(levels=8), "levels", -1), (dict(radius=0), "radius", -1), (dict(radius=5), "radius", -1),
    (dict(window=-1), "window", -1), (dict(window=5), "window", -1), (dict(median=2), "median", -1), (dict(median=-1), "median", -1),
    (dict(fb_max_diff=-2), "fb_max_diff", -1), (dict(subpixel=2), "subpixel", -1),
    (dict(W=8192, H=8193), "2^26", -4),
])
def test_create_refusals(ctx, kw, word, code):
    from vdo_slam_amd import _capi as K
    kw = dict(kw)
    W, H = kw.pop("W", 32), kw.pop("H", 16)
    with pytest.raises(K.VdoError, match=word.replace("^", r"\^")) as e:
        _matcher(ctx, H, W, **kw)
    assert e.value.code == code


def test_compute_refusals_write_nothing(ctx):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd import optflow
    H, W = 16, 32
    m = _matcher(ctx, H, W, levels=2)
    img = np.zeros((H, W), np.uint8)
    flow = np.full((H, W, 2), -7.0, np.float32); valid = np.full((H, W), 9, np.uint8)
    untouched = lambda: (flow == -7.0).all() and (valid == 9).all()      # noqa: E731
    p = img.ctypes.data
    for args, word in (((0, W, p, W), "im0"), ((p, W, 0, W), "im1"), ((p, W - 1, p, W), "stride0"), ((p, W, p, W - 1), "stride1"), ((p, 0, p, W), "stride0")):
        with pytest.raises(K.VdoError, match=word) as e:
            m.compute_raw(*args, False, flow.ctypes.data, valid.ctypes.data, False)
        assert e.value.code == -1 and untouched()
    L = optflow._lib()
    n = C.c_int32(-7)
    assert L.vdo_optflow_compute(m._h, p, W, p, W, 0, None, valid.ctypes.data, 0, C.byref(n)) == -1 and n.value == -7 and untouched()
    assert L.vdo_optflow_compute(m._h, p, W, p, W, 0, flow.ctypes.data, valid.ctypes.data, 0, None) == -1 and untouched()
    assert L.vdo_optflow_compute(None, p, W, p, W, 0, flow.ctypes.data, valid.ctypes.data, 0, C.byref(n)) == -1 and untouched() and n.value == -7
    for fn in (m.pyramid, m.census, m.level_flow):                                     # inspection before the first compute
        with pytest.raises(K.VdoError, match="no vdo_optflow_compute"):
            fn(0, 0)
    m.compute(img, img)
    for fn, word in ((m.pyramid, "which"), (m.census, "which"), (m.level_flow, "dir")):
        with pytest.raises(K.VdoError, match=word):
            fn(2, 0)
    with pytest.raises(K.VdoError, match="level"):
        m.census(0, 2)
    with pytest.raises(K.VdoError, match="level"):
        m.level_size(-1)
    assert L.vdo_optflow_create(ctx._h, W, H, None, C.byref(C.c_void_p())) == -1
    m.close()
    m = _matcher(ctx, H, W, levels=2, fb_max_diff=-1)
    m.compute(img, img)
    with pytest.raises(K.VdoError, match="backward"):
        m.level_flow(1, 0)
    m.close()


# ---- host classes -------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_flowmatcher_class_equals_the_c_entry(ctx):
    from vdo_slam_amd import _capi as K
    host = K.load_host_lib()
    host.host_optflow_compute.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    W, H = 131, 67
    a, b, want = _moved_and_ref(W, H)
    prm = np.array([6, 2, 2, 1, 1, 1], np.int32)
    padded = np.zeros((H, W + 5), np.uint8); padded[:, :W] = a                         # (a cv::Mat with a row step of its own)
    flow = np.full((H, W, 2), -1.0, np.float32); valid = np.full((H, W), 7, np.uint8)
    assert host.host_optflow_compute(_ptr(padded), W + 5, _ptr(b), W, W, H, _ptr(prm), _ptr(flow), _ptr(valid)) == want["n_valid"]
    assert np.array_equal(flow, want["flow"]) and np.array_equal(valid, want["valid"])
    flow.fill(-1.0)
    assert host.host_optflow_compute(_ptr(padded), W + 5, _ptr(b), W, W, H, _ptr(prm), _ptr(flow), None) == want["n_valid"]
    assert np.array_equal(flow, want["flow"])
    prm[1] = 9                                                                          # a refusal surfaces as a failure, not as an exit
    assert host.host_optflow_compute(_ptr(a), W, _ptr(b), W, W, H, _ptr(prm), _ptr(flow), None) == -1


def _forward_warp(img, flow, seed):
    """The next image of a frame: noise under the forward warp of `img` by its (rounded) flow"""
    H, W = img.shape
    out = np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    xt, yt = xs + np.rint(flow[..., 0]).astype(np.int64), ys + np.rint(flow[..., 1]).astype(np.int64)
    ok = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
    out[yt[ok], xt[ok]] = img[ok]
    return out


def test_trackstereopair_equals_trackstereo_on_the_device_flow(ctx, tmp_path):
    """System(STEREO).TrackStereoPair over 3 frames against TrackStereo fed the flow vdo_optflow_compute returned for the same image pairs"""
    from tests import stereo_ref as SR
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.system import System, write_settings
    W, H, n_frames = synth.KITTI_W, synth.KITTI_H, 3
    cfg = write_settings(tmp_path / "k.yaml", W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    Ts = SQ.camera_poses(n_frames); objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs) for k in range(n_frames)]
    rights, nexts = [], []
    for k, fr in enumerate(frames):
        disp = np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64)
        right = np.random.default_rng(500 + k).integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(fr["gray"], disp, right)
        rights.append(right)
        nexts.append(_forward_warp(fr["gray"], fr["flow"], 900 + k))
    rows = np.array([[0, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in (1, 2, 3)], np.float32)
    s = System(cfg, sensor="stereo")
    poses = [s.track_stereo_pair(fr["gray"], rights[k], nexts[k], fr["mask"].copy(), rows, n_images=n_frames) for k, fr in enumerate(frames)]
    motions = s.motions()
    s.close()
    assert all(T is not None for T in poses)
    m = _matcher(ctx, H, W)                                      # the settings file has no Flow.* key: the defaults
    flows = [m.compute(fr["gray"], nexts[k]) for k, fr in enumerate(frames)]
    m.close()
    s = System(cfg, sensor="stereo")
    want = [s.track_stereo(fr["gray"], rights[k], flows[k][0], fr["mask"].copy(), rows, n_images=n_frames) for k, fr in enumerate(frames)]
    want_motions = s.motions()
    s.close()
    for k in range(n_frames):
        assert np.array_equal(poses[k], want[k]), k
    assert len(motions) == len(want_motions)
    for (la, Ha), (lb, Hb) in zip(motions, want_motions):
        assert la == lb and np.array_equal(Ha, Hb)
    assert not np.array_equal(poses[-1], np.eye(4, dtype=np.float32))
    for k, fr in enumerate(frames):                              # the matcher finds the scene's motion where it says so
        flow, valid, n = flows[k]
        print(f"frame {k}: valid share {n / (W * H):.3f}, within 1 px of the truth on valid pixels "
              f"{(np.abs(flow - fr['flow']).max(axis=-1)[valid > 0] <= 1.0).mean():.3f}")
        assert n > 0
