"""GPU: the device motion segmenter (vdo_motionseg_*, csrc/motionseg.hip) against the NumPy restatement of its contract (tests/motionseg_ref.py).
Every comparison is array_equal: state, residual bits, class image, the three counts, the sample lists."""
import ctypes as C

import numpy as np
import pytest

from tests import motionseg_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
TW, TH = 64, 16                                                  # the vote tile of csrc/motionseg.hip
UNIT = 256.0
I4 = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _camera(W, H):
    """A camera for a W x H image: (K4, bf)"""
    f = 0.6 * max(W, H, 8)
    return (f, f, 0.5 * W, 0.5 * H), 0.5 * f


def _segmenter(ctx, H, W, **prm):
    from vdo_slam_amd.motionseg import MotionSegmenter
    K4, bf = _camera(W, H)
    prm.setdefault("disp_unit", UNIT)
    return MotionSegmenter(ctx, W, H, prm.pop("K4", K4), prm.pop("bf", bf), prm.pop("disp_unit"), **prm)


def _ref(m, d0, d1, flow, valid, T):
    p = m.params
    return R.stages(d0, d1, flow, valid, T, tuple(p.K), p.bf, p.disp_unit, sigma_flow=p.sigma_flow, sigma_disp=p.sigma_disp, chi2=p.chi2, min_disparity=p.min_disparity,
                    vote_radius=p.vote_radius, vote_num=p.vote_num, vote_den=p.vote_den, min_known=p.min_known, class_value=p.class_value)


def _same(m, d0, d1, flow, valid, T, want, what=""):
    cls, counts = m.compute(d0, d1, flow, valid, T)
    assert np.array_equal(m.state(), want["state"]), f"{what}: state"
    assert np.array_equal(m.residual().view(np.uint32), want["residual"].view(np.uint32)), f"{what}: residual bits"
    assert cls.dtype == np.uint8 and np.array_equal(cls, want["cls"]), f"{what}: class image"
    assert counts == want["counts"], f"{what}: counts {counts} against {want['counts']}"


def _check(ctx, d0, d1, flow, valid=None, T=I4, what="", **prm):
    H, W = d0.shape
    m = _segmenter(ctx, H, W, **prm)
    want = _ref(m, d0, d1, flow, valid, T)
    _same(m, d0, d1, flow, valid, T, want, what)
    m.close()
    return want


def _noise(H, W, seed):
    """Disparities of 2..30 px with holes, a second disparity and a flow that put the residual under the identity on both sides of chi2 = 9"""
    rng = np.random.default_rng(seed)
    d0 = (rng.uniform(2, 30, (H, W)) * UNIT).astype(F)
    d1 = (d0 + rng.normal(0, 0.7 * UNIT, (H, W))).astype(F)
    d0[rng.random((H, W)) < 0.1] = 0
    d1[rng.random((H, W)) < 0.1] = 0
    flow = rng.normal(0, 1.0, (H, W, 2)).astype(F)
    return d0, d1, flow


def _small_motion():
    T = I4.copy()
    T[0, 3], T[2, 3], T[0, 2], T[2, 0] = 0.01, -0.05, 0.002, -0.002
    return T


# ---- sizes: one pixel, one row / column, around the wave, around the vote tile in both axes, a window spanning two tiles in each axis ---------------
SIZES = ([(1, 1), (1, 7), (7, 1)] + [(w, h) for w in (31, 32, 33) for h in (7, 8, 9)] + [(96, 64), (200, 37)] +
         [(TW, TH), (TW + 1, TH + 1), (TW - 1, TH - 1), (2 * TW + 2, 2 * TH + 1)])


@pytest.mark.parametrize("W,H", SIZES)
def test_sizes(ctx, W, H):
    d0, d1, flow = _noise(H, W, 1000 * H + W)
    want = [_check(ctx, d0, d1, flow, None, _small_motion(), f"{W}x{H} noise r={r}", vote_radius=r) for r in (2, 7)]      # radius 7: the halo spans two tiles at 130 x 33
    if W * H > 200:
        assert min(want[0]["counts"]) > 0                        # all three states and moving pixels occur
    const = np.full((H, W), 8 * UNIT, F)
    want = _check(ctx, const, const, np.zeros((H, W, 2), F), None, I4, f"{W}x{H} constant")
    assert want["counts"] == (0, W * H, 0)
    want = _check(ctx, const, (const + F(3 * UNIT)), np.zeros((H, W, 2), F), None, I4, f"{W}x{H} constant, moving", min_known=1)
    assert want["counts"] == (W * H, 0, 0)


def test_rendered_frames_scaled(ctx):
    """synth_seq frames rendered at 96 x 64 with K scaled: the true camera motion, exact and noisy inputs"""
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    W, H = 96, 64
    sx, sy = W / synth.KITTI_W, H / synth.KITTI_H
    fx, fy, cx, cy = synth.KITTI_K
    K4 = (fx * sx, fy * sy, cx * sx, cy * sy)
    bf = SF.BF * sx
    Ts = SQ.camera_poses(2); objs = SQ.default_objects()
    for kw in ({}, dict(flow_sigma=0.02, invalid_depth=0.02, zero_flow=0.01)):       # (noise and sigmas scaled with the image: 0.3 and 0.5 px at 1242 wide)
        f0, f1 = [SQ.render_frame(k, Ts, objs, w=W, h=H, K4=K4, **kw) for k in range(2)]
        d0, d1 = [(f["depth_raw"] * F(sx)).astype(F) for f in (f0, f1)]      # render_frame's disparity is for the full baseline
        T = (f0["Tcw_next"] @ np.linalg.inv(f0["Tcw"])).astype(F)
        want = _check(ctx, d0, d1, f0["flow"], None, T, "rendered", K4=K4, bf=bf, min_disparity=bf / SF.TH_DEPTH_BG, sigma_flow=0.05, sigma_disp=0.05)
        obj = f0["mask"] > 0
        assert obj.sum() > 50 and (want["cls"][obj] > 0).mean() > 0.9 and (want["cls"][~obj] > 0).mean() < 0.05


def test_flows_that_leave_the_image_and_rounding_ties(ctx):
    W, H = 70, 20
    d0 = np.full((H, W), 10 * UNIT, F)
    d1 = d0.copy(); d1[:, 0] = 14 * UNIT; d1[:, W - 1] = 15 * UNIT; d1[0, :] = 16 * UNIT; d1[H - 1, :] = 17 * UNIT      # the borders tell who was read
    ys, xs = np.mgrid[0:H, 0:W]
    cases = {}
    for side, (fu, fv) in dict(left=(-xs - 0.5, 0 * ys), left_out=(np.nextafter((-xs - 0.5).astype(F), F(-100)), 0 * ys), right=(W - 1.5 - xs, 0 * ys), right_out=(W - 0.5 - xs, 0 * ys),
                               up=(0 * xs, -ys - 0.5), up_out=(0 * xs, np.nextafter((-ys - 0.5).astype(F), F(-100))), down=(0 * xs, H - 1.5 - ys), down_out=(0 * xs, H - 0.5 - ys),
                               far=(1e6 + 0 * xs, -1e6 + 0 * ys), ties=(0.5 + 0 * xs, 1.5 + 0 * ys), neg_ties=(-1.5 + 0 * xs, -0.5 + 0 * ys)).items():
        flow = np.stack([fu, fv], -1).astype(F)
        cases[side] = _check(ctx, d0, d1, flow, None, I4, side)
    for side in ("left", "right", "up", "down"):                 # uo = -0.5 rounds to 0, uo = W - 1.5 to W - 1: every pixel reads the border
        assert (cases[side]["state"] != 2).all(), side
        assert (cases[side + "_out"]["state"] == 2).all(), side
    assert (cases["far"]["state"] == 2).all()
    assert (cases["ties"]["state"][:, W - 1] == 2).all() and (cases["ties"]["state"][: H - 2, : W - 1] != 2).all()      # +0.5 goes to x + 1, -0.5 stays
    assert (cases["neg_ties"]["state"][:, 0] == 2).all() and (cases["neg_ties"]["state"][0, 1:] != 2).all()


def test_non_finite_and_extreme_values(ctx):
    W, H = 67, 19
    base = _noise(H, W, 5)
    rng = np.random.default_rng(6)
    specials = [np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, -3 * UNIT, float(2 ** 24), float(2 ** 24) * UNIT, 1e-38, 1e-42, 3e38]
    for which in range(3):                                       # the flow, disp0, disp1 in turn, then all at once
        d0, d1, flow = [a.copy() for a in base]
        target = (d0, d1, flow.reshape(H, 2 * W))[which]
        idx = rng.random(target.shape) < 0.4
        target[idx] = rng.choice(np.array(specials, F), int(idx.sum()))
        _check(ctx, d0, d1, flow, None, _small_motion(), f"specials in input {which}")
    d0, d1, flow = [a.copy() for a in base]
    for a in (d0, d1, flow):
        idx = rng.random(a.shape) < 0.3
        a[idx] = rng.choice(np.array(specials, F), int(idx.sum()))
    want = _check(ctx, d0, d1, flow, None, _small_motion(), "specials everywhere")
    assert want["counts"][2] > W * H // 3
    # T itself not finite: every pixel is unknown
    T = I4.copy(); T[0, 3] = np.nan
    want = _check(ctx, *base, None, T, "T with a NaN")
    assert want["counts"] == (0, 0, W * H)


def test_camera_motions(ctx):
    W, H = 64, 24
    d0, d1, flow = _noise(H, W, 9)
    _check(ctx, d0, d1, flow, None, I4, "identity")
    back = I4.copy(); back[2, 3] = -1e4                          # every point behind the camera
    want = _check(ctx, d0, d1, flow, None, back, "behind")
    assert want["counts"] == (0, 0, W * H)
    half = I4.copy(); half[2, 2] = -1.0                          # a half turn: Z' = -Z
    assert _check(ctx, d0, d1, flow, None, half, "half turn")["counts"][2] == W * H
    # Z' tiny: a wall at one depth moved to within a few ulps of the camera plane, in front of it and behind
    K4, bf = _camera(W, H)
    wall = np.full((H, W), 10 * UNIT, F)
    Z = F(bf) / F(10)
    for eps, name in ((np.nextafter(Z, F(1e9)) - Z, "tiny"), (F(0), "zero"), (Z - np.nextafter(Z, F(1e9)), "tiny negative")):
        T = I4.copy(); T[2, 3] = -Z + eps
        want = _check(ctx, wall, wall, np.zeros((H, W, 2), F), None, T, "Z' " + name)
        if name != "tiny":
            assert want["counts"][2] == W * H
    fast = _small_motion(); fast[:3, 3] *= 100
    _check(ctx, d0, d1, flow, None, fast, "fast")


def test_e_at_chi2_and_min_disparity_at_the_value(ctx):
    W, H = 40, 12
    d0, d1, flow = _noise(H, W, 21)
    T = _small_motion()
    first = _check(ctx, d0, d1, flow, None, T, "first", vote_radius=0, min_known=1)
    y, x = np.argwhere(first["state"] == 1)[3]
    e = first["residual"][y, x]
    at = _check(ctx, d0, d1, flow, None, T, "e == chi2", chi2=float(e), vote_radius=0, min_known=1)
    beyond = _check(ctx, d0, d1, flow, None, T, "e one ulp beyond chi2", chi2=float(np.nextafter(e, F(0))), vote_radius=0, min_known=1)
    assert at["state"][y, x] == 0 and at["cls"][y, x] == 0 and beyond["state"][y, x] == 1 and beyond["cls"][y, x] == 1
    y, x = np.argwhere(first["state"] != 2)[5]
    px = d0[y, x] / F(UNIT)
    at = _check(ctx, d0, d1, flow, None, T, "d0 == min_disparity", min_disparity=float(px))
    beyond = _check(ctx, d0, d1, flow, None, T, "d0 one ulp below min_disparity", min_disparity=float(np.nextafter(px, F(1e9))))
    assert at["state"][y, x] != 2 and beyond["state"][y, x] == 2
    assert _check(ctx, d0, d1, flow, None, T, "chi2 0", chi2=0.0)["counts"][1] == 0


@pytest.mark.parametrize("r", [0, 1, 2, 7])
def test_vote_parameters(ctx, r):
    W, H = 2 * TW + 2, 2 * TH + 1
    d0, d1, flow = _noise(H, W, 33 + r)
    T = _small_motion()
    full = (2 * r + 1) ** 2
    for num, den in ((0, 1), (1, 2), (2, 3)):
        for min_known in (1, full, full + 1):
            for cv in (1, 255):
                want = _check(ctx, d0, d1, flow, None, T, f"r {r} {num}/{den} min_known {min_known} class {cv}", vote_radius=r, vote_num=num, vote_den=den, min_known=min_known,
                              class_value=cv)
                assert set(np.unique(want["cls"])) <= {0, cv}
                if min_known == full + 1:
                    assert want["counts"][0] == 0                # nothing moves
    if r == 0:                                                   # radius 0, 0/1, min_known 1: the class image is the state
        want = _check(ctx, d0, d1, flow, None, T, "state", vote_radius=0, vote_num=0, vote_den=1, min_known=1)
        assert np.array_equal(want["cls"], (want["state"] == 1).astype(np.uint8))


def test_flow_valid(ctx):
    W, H = 65, 17
    d0, d1, flow = _noise(H, W, 44)
    none = _check(ctx, d0, d1, flow, None, I4, "NULL")
    ones = _check(ctx, d0, d1, flow, np.full((H, W), 1, np.uint8), I4, "all 1")
    assert np.array_equal(none["cls"], ones["cls"]) and none["counts"] == ones["counts"]
    assert _check(ctx, d0, d1, flow, np.zeros((H, W), np.uint8), I4, "all 0")["counts"] == (0, 0, W * H)
    mixed = np.random.default_rng(4).integers(0, 3, (H, W)).astype(np.uint8) * 127        # 0, 127, 254: any non-zero value is valid
    want = _check(ctx, d0, d1, flow, mixed, I4, "mixed")
    assert (want["state"][mixed == 0] == 2).all() and (want["state"][mixed != 0] != 2).any()


# ---- ego-motion -------------------------------------------------------------------------------------------------------------------------------
def _scene_96(noise=False):
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    W, H = 96, 64
    sx, sy = W / synth.KITTI_W, H / synth.KITTI_H
    fx, fy, cx, cy = synth.KITTI_K
    K4 = (fx * sx, fy * sy, cx * sx, cy * sy)
    Ts = SQ.camera_poses(2); objs = SQ.default_objects()
    f0 = SQ.render_frame(0, Ts, objs, w=W, h=H, K4=K4, **(dict(flow_sigma=0.1, invalid_depth=0.02, zero_flow=0.01) if noise else {}))
    return K4, SF.BF * sx, (f0["depth_raw"] * F(sx)).astype(F), f0["flow"], (f0["Tcw_next"] @ np.linalg.inv(f0["Tcw"]))


@pytest.mark.parametrize("step", [1, 3, 16, 97, 200, 1 << 30])
def test_sample_lists_and_ransac(ctx, step):
    from vdo_slam_amd.ransac import pnp_ransac_batch
    K4, bf, d0, flow, T_true = _scene_96(noise=True)
    H, W = d0.shape
    valid = (np.random.default_rng(2).random((H, W)) < 0.9).astype(np.uint8)
    m = _segmenter(ctx, H, W, K4=K4, bf=bf, min_disparity=1.0)
    for fv in (None, valid):
        X, uv = R.samples(d0, flow, fv, tuple(m.params.K), m.params.bf, UNIT, step, min_disparity=1.0)
        T, out = m.egomotion(d0, flow, fv, step=step, max_iterations=200, threshold=0.5, confidence=0.98, min_inliers=5)
        gX, guv = m.samples()
        assert np.array_equal(gX, X) and np.array_equal(guv, uv), step
        assert out[0] == len(X)
        want = pnp_ransac_batch(ctx, [(X, uv)], [float(v) for v in m.params.K], max_iterations=200, thr=0.5, confidence=0.98, refit=True)[0]
        assert out[1:] == (want["n_inliers"], want["iterations_run"])
        if want["n_inliers"] >= 5:
            assert np.array_equal(T, want["T"].astype(F))
        else:
            assert np.array_equal(T, I4)
        if step >= 200:
            assert out == (0, 0, 0) and np.array_equal(T, I4)    # step / 2 beyond the image: no samples (97 leaves one)
        if step == 3:
            assert out[1] > 100 and np.abs(T[:3, 3] - T_true[:3, 3]).max() < 0.05
    # too few inliers: the identity, and the counts still say what was found
    T, out = m.egomotion(d0, flow, None, step=3, max_iterations=200, threshold=0.5, min_inliers=W * H + 1)
    assert np.array_equal(T, I4) and out[1] > 0
    m.close()


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------
def test_padded_strides_and_memory_spaces(ctx):
    import torch
    W, H = 77, 21
    d0, d1, flow = _noise(H, W, 50)
    valid = (np.random.default_rng(3).random((H, W)) < 0.8).astype(np.uint8)
    T = _small_motion()
    m = _segmenter(ctx, H, W)
    want = _ref(m, d0, d1, flow, valid, T)

    def pad(a, extra):
        b = np.full((H, a.shape[1] + extra) + a.shape[2:], 7, a.dtype)
        b[:, : a.shape[1]] = a
        return b
    p0, p1, pf, pv = pad(d0, 3), pad(d1, 5), pad(flow, 2), pad(valid, 9)
    _same(m, p0[:, :W], p1[:, :W], pf[:, :W], pv[:, :W], T, want, "padded host rows")
    for src_dev in (False, True):
        for out_dev in (False, True):
            for padded in (False, True):
                arrs = (p0, p1, pf, pv) if padded else (d0, d1, flow, valid)
                if src_dev:
                    keep = [torch.from_numpy(a).cuda() for a in arrs]
                    ptrs = [t.data_ptr() for t in keep]
                else:
                    ptrs = [a.ctypes.data for a in arrs]
                strides = [arrs[0].shape[1], arrs[1].shape[1], 2 * arrs[2].shape[1], arrs[3].shape[1]]
                out_t = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
                out_h = np.full((H, W), 9, np.uint8)
                torch.cuda.synchronize()
                counts = m.compute_raw(ptrs[0], strides[0], ptrs[1], strides[1], ptrs[2], strides[2], ptrs[3], strides[3], src_dev, T,
                                       out_t.data_ptr() if out_dev else out_h.ctypes.data, out_dev)
                cls = out_t.cpu().numpy() if out_dev else out_h
                what = f"src_dev {src_dev} out_dev {out_dev} padded {padded}"
                assert counts == want["counts"] and np.array_equal(cls, want["cls"]), what
                assert np.array_equal(m.state(), want["state"]) and np.array_equal(m.residual().view(np.uint32), want["residual"].view(np.uint32)), what
    # a packed device flow that is not 8-byte aligned goes through the staging image
    t = torch.zeros(2 * W * H + 1, dtype=torch.float32, device="cuda")
    t[1:] = torch.from_numpy(flow.ravel()).cuda()
    td0, td1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()
    torch.cuda.synchronize()
    assert (t.data_ptr() + 4) % 8 == 4
    out_h = np.zeros((H, W), np.uint8)
    assert m.compute_raw(td0.data_ptr(), W, td1.data_ptr(), W, t.data_ptr() + 4, 2 * W, None, 0, True, T, out_h.ctypes.data, False) == _ref(m, d0, d1, flow, None, T)["counts"]
    m.close()


def test_egomotion_of_strided_host_and_device_sources(ctx):
    """vdo_motionseg_egomotion brings its images to the device as vdo_motionseg_compute does: host rows with a stride, device rows with a stride and
    packed device images (read where they lie) give the sample lists, the pose and the counts of the packed host call, bit for bit"""
    import torch
    W, H = 13, 7
    d0, _, flow = _noise(H, W, 51)
    valid = (np.random.default_rng(4).random((H, W)) < 0.8).astype(np.uint8)
    kw = dict(step=1, max_iterations=20, threshold=1.0, confidence=0.98, min_inliers=5)
    m = _segmenter(ctx, H, W)
    want = m.egomotion(d0, flow, valid, **kw)
    want_X, want_uv = m.samples()
    assert want[1][0] > 0 and len(want_X) == want[1][0]
    p0 =np.full((H, 16), 7, F); p0[:, :W] = d0
    pf = np.full((H, 16, 2), 7, F); pf[:, :W] = flow
    pv = np.full((H, 16), 7, np.uint8); pv[:, :W] = valid
    t0, tf, tv, tp0, tpf, tpv = (torch.from_numpy(a).cuda() for a in (d0, flow, valid, p0, pf, pv))
    torch.cuda.synchronize()
    assert tf.data_ptr() % 8 == 0
    for what, call in [("strided host", lambda: m.egomotion(p0[:, :W], pf[:, :W], pv[:, :W], **kw)),
                       ("strided device", lambda: m.egomotion_raw(tp0.data_ptr(), 16, tpf.data_ptr(), 32, tpv.data_ptr(), 16, True, **kw)),
                       ("packed device", lambda: m.egomotion_raw(t0.data_ptr(), W, tf.data_ptr(), 2 * W, tv.data_ptr(), W, True, **kw))]:
        T, out = call()
        X, uv = m.samples()
        assert np.array_equal(X, want_X) and np.array_equal(uv, want_uv) and out == want[1] and np.array_equal(T, want[0]), what
    m.close()


def test_the_handles_own_device_images_and_no_shared_state(ctx):
    import torch
    W, H = 70, 18
    a = _noise(H, W, 60); b = _noise(H, W, 61)
    T = _small_motion()
    m = _segmenter(ctx, H, W)
    p_disp1, p_right, p_cls = m.device_images()
    assert p_disp1 and p_right and p_cls and len({p_disp1, p_right, p_cls}) == 3
    want_a, want_b = _ref(m, *a, None, T), _ref(m, *b, None, I4)
    # a host disp1 is staged in the handle's disp1 image: passed back as a device source it is read where it lies; the class image goes into the
    # handle's own, from where the labeller reads it as a device source (one label per component of moving pixels)
    _same(m, *a, None, T, want_a, "a")
    t0, tf = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[2]).cuda()
    torch.cuda.synchronize()
    counts = m.compute_raw(t0.data_ptr(), W, p_disp1, W, tf.data_ptr(), 2 * W, None, 0, True, T, p_cls, True)
    assert counts == want_a["counts"]
    from tests import labels_ref as LR
    from vdo_slam_amd.labels import InstanceLabeler
    lab = InstanceLabeler(ctx, W, H, min_area=1, max_disp_diff=-1)
    mask = np.zeros((H, W), np.int32)
    n_labels = lab.compute_raw(p_cls, W, None, 0, True, mask.ctypes.data, False)[0]
    lab.close()
    assert np.array_equal(mask, LR.stages(want_a["cls"], None, 8, -1, 1, 1023)["mask"]) and n_labels == mask.max() > 0
    # two computes (and an ego-motion between them) on one handle: b after a equals b alone, a again equals a
    _same(m, *b, None, I4, want_b, "b after a")
    m.egomotion(a[0], a[2], None, step=4)
    _same(m, *a, None, T, want_a, "a after b")
    _same(m, *b, None, I4, want_b, "b again")
    m.close()


def _last_error():
    from vdo_slam_amd import _capi as K
    return K.lib().vdo_last_error().decode()


def test_every_refusal_writes_nothing(ctx):
    from vdo_slam_amd import _capi as K, motionseg as MS
    W, H = 16, 9
    L = MS._lib()
    K4, bf = _camera(W, H)
    good = dict(K4=K4, bf=bf, disp_unit=UNIT)
    bad = [("K", dict(good, K4=(0.0, 1, 1, 1))), ("K", dict(good, K4=(1.0, 1.0, float("nan"), 1))), ("bf", dict(good, bf=0.0)), ("disp_unit", dict(good, disp_unit=-1.0)),
           ("sigma_flow", dict(good, sigma_flow=0.0)), ("sigma_disp", dict(good, sigma_disp=float("inf"))), ("chi2", dict(good, chi2=-1.0)),
           ("min_disparity", dict(good, min_disparity=-0.5)), ("vote_radius", dict(good, vote_radius=8)), ("vote_radius", dict(good, vote_radius=-1)),
           ("vote_den", dict(good, vote_den=0)), ("vote_num", dict(good, vote_num=2, vote_den=2)), ("vote_num", dict(good, vote_num=-1)), ("min_known", dict(good, min_known=0)),
           ("class_value", dict(good, class_value=0)), ("class_value", dict(good, class_value=256))]
    for word, prm in bad:
        h = C.c_void_p(77)
        p = MS.params(**prm)
        assert L.vdo_motionseg_create(ctx._h, W, H, C.byref(p), C.byref(h)) == -1 and word in _last_error() and h.value == 77, (word, _last_error())
    p = MS.params(**good)
    h = C.c_void_p(77)
    for args, word in (((None, W, H, C.byref(p), C.byref(h)), "ctx"), ((ctx._h, 0, H, C.byref(p), C.byref(h)), "width"), ((ctx._h, W, 0, C.byref(p), C.byref(h)), "height"),
                       ((ctx._h, W, H, None, C.byref(h)), "params"), ((ctx._h, W, H, C.byref(p), None), "out")):
        assert L.vdo_motionseg_create(*args) == -1 and word in _last_error() and h.value == 77
    assert L.vdo_motionseg_create(ctx._h, 1 << 14, 1 << 13, C.byref(p), C.byref(h)) == -4 and "2^26" in _last_error() and h.value == 77      # VDO_ERR_UNSUPPORTED
    m = _segmenter(ctx, H, W)
    for fn in (m.state, m.residual, m.samples):                  # nothing computed yet
        with pytest.raises(K.VdoError, match="no vdo_motionseg_"):
            fn()
    d0, d1, flow = _noise(H, W, 70)
    valid = np.ones((H, W), np.uint8)
    cls = np.full((H, W), 9, np.uint8)
    T = np.ascontiguousarray(I4.ravel())
    out = (C.c_int32 * 3)(-7, -7, -7)
    a = dict(h=m._h, d0=d0.ctypes.data, s0=W, d1=d1.ctypes.data, s1=W, fl=flow.ctypes.data, sf=2 * W, fv=valid.ctypes.data, sv=W, dev=0, T=T.ctypes.data, cls=cls.ctypes.data, od=0, out=out)
    for word, change in (("handle", dict(h=None)), ("disp0 is null", dict(d0=None)), ("disp0_stride", dict(s0=W - 1)), ("disp1 is null", dict(d1=None)), ("disp1_stride", dict(s1=W - 1)),
                         ("flow is null", dict(fl=None)), ("flow_stride", dict(sf=2 * W - 1)), ("flow_valid_stride", dict(sv=W - 1)), ("T is null", dict(T=None)),
                         ("cls is null", dict(cls=None)), ("out is null", dict(out=None))):
        q = dict(a, **change)
        assert L.vdo_motionseg_compute(*q.values()) == -1 and word in _last_error(), (word, _last_error())
        assert (cls == 9).all() and list(out) == [-7] * 3
    Tm = np.full(16, 5, F)
    e = dict(h=m._h, d0=d0.ctypes.data, s0=W, fl=flow.ctypes.data, sf=2 * W, fv=valid.ctypes.data, sv=W, dev=0, step=4, it=100, thr=1.0, conf=0.98, mi=5,
             T=Tm.ctypes.data, out=out)
    for word, change in (("handle", dict(h=None)), ("disp0 is null", dict(d0=None)), ("disp0_stride", dict(s0=W - 1)), ("flow is null", dict(fl=None)), ("flow_stride", dict(sf=W)),
                         ("flow_valid_stride", dict(sv=0)), ("step", dict(step=0)), ("max_iterations", dict(it=-1)), ("reproj_threshold", dict(thr=0.0)),
                         ("confidence", dict(conf=1.0)), ("min_inliers", dict(mi=-1)), ("T is null", dict(T=None)), ("out is null", dict(out=None))):
        q = dict(e, **change)
        assert L.vdo_motionseg_egomotion(*q.values()) == -1 and word in _last_error(), (word, _last_error())
        assert (Tm == 5).all() and list(out) == [-7] * 3
    for fn in (m.state, m.residual, m.samples):                  # none of the refused calls counts
        with pytest.raises(K.VdoError, match="no vdo_motionseg_"):
            fn()
    assert L.vdo_motionseg_get_state(m._h, None) == -1 and L.vdo_motionseg_get_samples(m._h, None, None, None) == -1 and L.vdo_motionseg_last_timing(m._h, None) == -1
    assert L.vdo_motionseg_device_images(None, None, None, None) == -1 and L.vdo_motionseg_destroy(None) == 0
    m.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_motionsegmenter_class_equals_the_c_entry(ctx):
    from vdo_slam_amd import _capi as K, motionseg as MS
    host = K.load_host_lib()
    host.host_motionseg_compute.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    K4, bf, d0, flow, _ = _scene_96()
    H, W = d0.shape
    d1 = np.roll(d0, 1, axis=1)
    valid = (np.random.default_rng(8).random((H, W)) < 0.9).astype(np.uint8)
    p = MS.params(K4, bf, UNIT, vote_radius=1, min_known=3, class_value=26)
    prm = dict(sigma_flow=p.sigma_flow, sigma_disp=p.sigma_disp, chi2=p.chi2, min_disparity=p.min_disparity, vote_radius=1, vote_num=1, vote_den=2, min_known=3, class_value=26)
    pad0 = np.zeros((H, W + 3), F); pad0[:, :W] = d0                                     # (cv::Mat with row steps of their own)
    pad1 = np.zeros((H, W + 1), F); pad1[:, :W] = d1
    padf = np.zeros((H, W + 2, 2), F); padf[:, :W] = flow
    padv = np.zeros((H, W + 7), np.uint8); padv[:, :W] = valid
    T = np.ascontiguousarray(_small_motion().ravel())
    cls = np.full((H, W), 9, np.uint8); counts = np.full(3, -1, np.int32)
    want = R.stages(d0, d1, flow, valid, T, tuple(p.K), p.bf, UNIT, **prm)
    n = host.host_motionseg_compute(_ptr(pad0), W + 3, _ptr(pad1), W + 1, _ptr(padf), 2 * (W + 2), _ptr(padv), W + 7, W, H, C.byref(p), None, None, _ptr(T), _ptr(cls), _ptr(counts), None)
    assert n == want["counts"][0] and np.array_equal(cls, want["cls"]) and tuple(counts) == want["counts"]
    # with the ego-motion: MotionSegmenter::EgoMotion then ::Compute against the two C entries
    m = MS.MotionSegmenter(ctx, W, H, K4, bf, UNIT, vote_radius=1, min_known=3, class_value=26)
    T_c, ego_c = m.egomotion(d0, flow, None, step=4, max_iterations=300, threshold=0.5, confidence=0.98, min_inliers=20)
    cls_c, counts_c = m.compute(d0, d1, flow, None, T_c)
    m.close()
    ego3 = np.array([4, 300, 20], np.int32); ego2 = np.array([0.5, 0.98]); T_h = np.zeros(16, F); ego_counts = np.zeros(3, np.int32)
    n = host.host_motionseg_compute(_ptr(d0), W, _ptr(d1), W, _ptr(flow), 2 * W, None, 0, W, H, C.byref(p), _ptr(ego3), _ptr(ego2), _ptr(T_h), _ptr(cls), _ptr(counts), _ptr(ego_counts))
    assert ego_c[1] >= 20 and tuple(ego_counts) == ego_c and np.array_equal(T_h.reshape(4, 4), T_c)
    assert n == counts_c[0] and np.array_equal(cls, cls_c) and tuple(counts) == counts_c
    p.vote_radius = 9                                                                   # a refusal surfaces as a failure, not as an exit
    assert host.host_motionseg_compute(_ptr(d0), W, _ptr(d1), W, _ptr(flow), 2 * W, None, 0, W, H, C.byref(p), None, None, _ptr(T), _ptr(cls), None, None) == -1
    got = MS.compute(ctx, d0, d1, flow, valid, T, K4, bf, UNIT, **prm)
    assert np.array_equal(got[0], want["cls"]) and got[1] == want["counts"]


# ---- System ------------------------------------------------------------------------------------------------------------------------------------
def _forward_warp(img, flow, seed):
    """The next image of a frame: noise under the forward warp of `img` by its (rounded) flow"""
    H, W = img.shape
    out = np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    xt, yt = xs + np.rint(flow[..., 0]).astype(np.int64), ys + np.rint(flow[..., 1]).astype(np.int64)
    ok = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
    out[yt[ok], xt[ok]] = img[ok]
    return out


def test_trackstereovideo_equals_trackstereopairsemantic_on_the_device_class_image(ctx, tmp_path):
    """System(STEREO).TrackStereoVideo over 3 frames at the KITTI size against TrackStereoPairSemantic fed the class image the stand-alone chain
    (stereo x 2, optflow, vdo_motionseg_egomotion, vdo_motionseg_compute) returns for the same images; then the same through identity Rectify.*
    keys.  Printed per frame: ego-motion inliers, moving pixels, labels, and the recall of the class image on the rendered object pixels (a record,
    not a gate: with the real matchers in the chain the quality is measured nowhere else yet)."""
    from tests import stereo_ref as SR
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.labels import InstanceLabeler
    from vdo_slam_amd.motionseg import MotionSegmenter
    from vdo_slam_amd.optflow import FlowMatcher
    from vdo_slam_amd.stereo import StereoMatcher
    from vdo_slam_amd.system import System, write_settings
    W, H, n_frames = synth.KITTI_W, synth.KITTI_H, 3
    base = (SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    cfg = write_settings(tmp_path / "k.yaml", W, H, synth.KITTI_K, *base)
    I3 = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    cam = dict(K=synth.KITTI_K, D=(0, 0, 0, 0, 0), R=I3)
    keyed = write_settings(tmp_path / "keyed.yaml", W, H, synth.KITTI_K, *base, rectify=dict(left=cam, right=cam))
    Ts = SQ.camera_poses(n_frames + 1); objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs) for k in range(n_frames + 1)]
    disps = [np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64) for fr in frames]
    rights, nexts, next_rights = [], [], []
    for k in range(n_frames):
        fr = frames[k]
        right = np.random.default_rng(500 + k).integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(fr["gray"], disps[k], right)
        rights.append(right)
        nexts.append(_forward_warp(fr["gray"], fr["flow"], 900 + k))
        nr = np.random.default_rng(700 + k).integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(nexts[k], disps[k + 1], nr)                # the next-left picture under frame k + 1's disparity
        next_rights.append(nr)
    # the stand-alone chain with the settings file's defaults (no Stereo.*, Flow.*, Labels.* or Motion.* key)
    sm = StereoMatcher(ctx, W, H)
    sm.set_output_scale(SF.DEPTH_MAP_FACTOR / 256.0)
    fm = FlowMatcher(ctx, W, H)
    ms = MotionSegmenter(ctx, W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, min_disparity=float(F(SF.BF) / F(SF.TH_DEPTH_BG)))
    lab = InstanceLabeler(ctx, W, H)
    classes, found = [], []
    for k in range(n_frames):
        d1 = sm.compute(nexts[k], next_rights[k])[0]
        d0 = sm.compute(frames[k]["gray"], rights[k])[0]
        flow, valid, _ = fm.compute(frames[k]["gray"], nexts[k])
        T, ego = ms.egomotion(d0, flow, valid)
        cls, counts = ms.compute(d0, d1, flow, valid, T)
        _, n_labels, _, _ = lab.compute(cls, d0)
        obj = frames[k]["mask"] > 0
        print(f"frame {k}: {ego[1]} inliers of {ego[0]} samples in {ego[2]} iterations, {counts[0]} moving pixels, {n_labels} labels, "
              f"recall on object pixels {float((cls[obj] > 0).mean()):.4f}, moving among the others {float((cls[~obj] > 0).mean()):.4f}")
        assert ego[1] >= 50 and n_labels >= 1                    # every frame finds a motion and at least one label
        classes.append(cls); found.append((ego[1], counts[0], n_labels))
    sm.close(); fm.close(); ms.close(); lab.close()
    rows = np.array([[0, label, 0, 0, 0, 0, 0, 0, 0, 0] for label in range(1, 40)], np.float32)

    def run(settings, call, counts=None):
        s = System(settings, sensor="stereo")
        try:
            poses = []
            for k in range(n_frames):
                poses.append(call(s, k))
                if counts is not None:
                    counts.append(s.video_counts())
            return poses, s.motions()
        finally:
            s.close()
    video = lambda s, k: s.track_stereo_video(frames[k]["gray"], rights[k], nexts[k], next_rights[k], rows, n_images=n_frames)
    semantic = lambda s, k: s.track_stereo_pair_semantic(frames[k]["gray"], rights[k], nexts[k], classes[k], rows, n_images=n_frames)
    want = run(cfg, semantic)
    for settings in (cfg, keyed):
        seen = []
        poses, motions = run(settings, video, seen)
        assert all(T is not None for T in poses) and all(T is not None for T in want[0])
        for k in range(n_frames):
            assert np.array_equal(poses[k], want[0][k]), (settings, k)
        assert len(motions) == len(want[1])
        for (la, Ha), (lb, Hb) in zip(motions, want[1]):
            assert la == lb and np.array_equal(Ha, Hb)
        assert seen == found                                     # the entry found what the chain found: inliers, moving pixels, labels
        assert not np.array_equal(poses[-1], np.eye(4, dtype=np.float32))
