"""vdo_static_stage (K9 + RenewFrameInfo (static) + Get3DinWorld in one round trip) against vdo_frame_static_filter followed by
vdo_renew_static_world on the same images: every output and both counts, bit for bit.  Sizes: around the 1024 threads of k_static_filter's and
k_carry_select's single workgroup, and none at all; max_num_sta below the carried count (the `m > max` stop), a few above it (the stride-20
top-up, with keypoints within 1 px of carried keys skipped) and large; with and without the 3-D points."""
import numpy as np
import pytest

from vdo_slam_amd import tracking as TR
from vdo_slam_amd.ba import Context
from vdo_slam_amd.frontend import FrameImages

pytestmark = pytest.mark.gpu

W, H = 96, 64           # (any image admits 1025 keypoints: the staging of an image set holds (w/4)(h/4) + 4096 columns, 0.8 of them keypoints)
TH_DEPTH_BG = 40.0
K4 = np.array([70.0, 72.0, 47.5, 31.5], np.float32)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(17)
    depth = rng.uniform(2.0, 38.0, (H, W)).astype(np.float32)
    bad = rng.random((H, W))
    depth[bad < 0.03] = 0.0; depth[(bad >= 0.03) & (bad < 0.06)] = 55.0            # invalid / beyond both depth gates
    flow = rng.uniform(-3.0, 3.0, (H, W, 2)).astype(np.float32)
    flow[rng.random((H, W)) < 0.03] = 0.0
    mask = np.zeros((H, W), np.int32)
    mask[20:30, 30:50] = 2                                                          # an object: its keypoints are no static candidates
    ctx = Context(0)
    im = FrameImages(ctx, W, H)
    im.upload(depth, flow, mask)
    Twc = np.eye(4, dtype=np.float32); Twc[:3, 3] = [0.3, -0.1, 1.5]
    c, s = np.cos(0.1), np.sin(0.1)
    Twc[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    return ctx, im, Twc


def _points(rng, n):
    # distinct pixel centres inside the 2-px inset image, so that no two keypoints coincide by accident
    cells = rng.permutation((W - 4) * (H - 4))[:n]
    x = 2 + cells % (W - 4) + rng.uniform(0.0, 0.9, n)
    y = 2 + cells // (W - 4) + rng.uniform(0.0, 0.9, n)
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("n_carried", [0, 1, 1024, 1025])
@pytest.mark.parametrize("n_orb", [0, 1, 1023, 1024, 1025])
def test_fused_static_stage_equals_the_two_calls(scene, n_orb, n_carried):
    ctx, im, Twc = scene
    rng = np.random.default_rng(1000 * n_orb + n_carried)
    n_stat = n_carried + 37                                   # the carried inliers are a subset of the last frame's static keys, in a shuffled order
    sx, sy = _points(rng, n_stat)
    tm = np.full(n_stat, -1, np.int32)
    tm[rng.permutation(n_stat)[:n_carried]] = 1
    tm = np.where(tm == 1, rng.permutation(n_stat), -1).astype(np.int32)       # TM_sta[i] = index of a static key, or -1
    ox, oy = _points(rng, n_orb)
    k = min(n_orb // 3, n_carried)                            # keypoints within 1 px of carried keys: `used` hits of the top-up
    car = tm[tm != -1][:k]
    ox[:k] = sx[car] + rng.uniform(-0.5, 0.5, k).astype(np.float32); oy[:k] = sy[car] + rng.uniform(-0.5, 0.5, k).astype(np.float32)
    hits = 0
    for max_num in (n_carried // 2, n_carried + 5, 5000):
        for world in (None, (K4, Twc)):
            k9_a = {q: v.copy() for q, v in im.static_filter(ox, oy, TH_DEPTH_BG).items()}
            ren_a = TR.renew_static(im, tm, sx, sy, ox, oy, max_num, world=world) if world is not None else TR.renew_static(im, tm, sx, sy, ox, oy, max_num)
            k9_b, ren_b = TR.static_stage(im, ox, oy, TH_DEPTH_BG, tm, sx, sy, max_num, world=world)
            assert k9_a["keep_idx"].size == k9_b["keep_idx"].size and ren_a["key_x"].size == ren_b["key_x"].size, (max_num, world is not None)
            for q in k9_a:
                assert np.array_equal(k9_a[q], k9_b[q]), (q, max_num, world is not None)
            assert set(ren_a) == set(ren_b) and ("xyz" in ren_b) == (world is not None)
            for q in ren_a:
                assert np.array_equal(ren_a[q], ren_b[q]), (q, max_num, world is not None)
            assert ren_b["key_x"].size <= max_num + 1
            hits += int((ren_b["inlier_id"] == -1).sum())
    if n_orb >= 1023:
        assert hits > 0 and k9_b["keep_idx"].size > 500      # the top-up ran and K9 kept most keypoints: the comparison was not of empty sets
    # the image set's scratch is what it was: the two calls give the same again after the fused one
    assert np.array_equal(im.static_filter(ox, oy, TH_DEPTH_BG)["keep_idx"], k9_b["keep_idx"])


def test_fused_static_stage_refuses_what_k9_refuses(scene):
    from vdo_slam_amd import _capi as K
    ctx, im, Twc = scene
    n = (W // 4) * (H // 4) + 4096                            # more than 0.8 of the staging's columns
    x = np.full(n, 5.0, np.float32)
    with pytest.raises(K.VdoError):
        im.static_filter(x, x, TH_DEPTH_BG)
    with pytest.raises(K.VdoError):
        TR.static_stage(im, x, x, TH_DEPTH_BG, np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32), 100)
    ox, oy = _points(np.random.default_rng(3), 50)            # ... and works afterwards
    k9, ren = TR.static_stage(im, ox, oy, TH_DEPTH_BG, np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32), 100)
    assert np.array_equal(k9["keep_idx"], im.static_filter(ox, oy, TH_DEPTH_BG)["keep_idx"]) and ren["key_x"].size > 0
