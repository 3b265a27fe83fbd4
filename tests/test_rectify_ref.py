"""CPU: the NumPy restatement of the stereo rectifier's contract (tests/rectify_ref.py) checked on its own - on identity and shift maps, against
a long-double evaluation of the same formulas on a real calibration, and on a source ramp.  tests/test_rectify_plan.py compares the library's
planner and tests/test_rectify_gpu.py the device with this restatement array_equal, so both inherit what is shown here."""
import numpy as np
import pytest

from tests import rectify_ref as R


@pytest.mark.parametrize("K4,size", [((60.0, 50.0, 31.5, 8.25), (65, 17)), (R.KITTI_K, R.KITTI_SIZE), (R.EUROC_K, R.EUROC_SIZE)])
def test_identity_map(K4, size):
    W, H = size
    m, v, n = R.plan(K4, (0, 0, 0, 0, 0), R.IDENTITY_R, K4, size, size)
    assert np.array_equal(m[..., 0], 32 * np.arange(W)[None, :].repeat(H, 0))
    assert np.array_equal(m[..., 1], 32 * np.arange(H)[:, None].repeat(W, 1))
    assert v.all() and n == W * H
    src = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
    assert np.array_equal(R.remap(src, m), src) and np.array_equal(R.remap(src, m, nearest=True), src)


def test_principal_point_shift():
    """cx' = cx + 3, cy' = cy - 2 at 65 x 17: destination (u, v) reads source (u - 3, v + 2); 62 x 15 pixels stay inside"""
    K4, size = (60.0, 50.0, 31.5, 8.25), (65, 17)
    P4 = (K4[0], K4[1], K4[2] + 3, K4[3] - 2)
    m, v, n = R.plan(K4, (0,) * 5, R.IDENTITY_R, P4, size, size)
    assert n == 62 * 15
    uu, vv = np.meshgrid(np.arange(65), np.arange(17))
    inside = (uu - 3 >= 0) & (vv + 2 <= 16)
    assert np.array_equal(v.astype(bool), inside)
    assert np.array_equal(m[inside][:, 0], 32 * (uu - 3)[inside]) and np.array_equal(m[inside][:, 1], 32 * (vv + 2)[inside])
    assert (m[~inside] == R.INVALID).all()
    src = np.random.default_rng(2).integers(0, 256, (17, 65), dtype=np.uint8)
    out = R.remap(src, m, border=7)
    assert np.array_equal(out[:15, 3:], src[2:, :62]) and (out[15:] == 7).all() and (out[:, :3] == 7).all()


def test_euroc_against_long_double():
    """The fp64 map of EuRoC cam0 (ORB-SLAM2's Examples/Stereo/EuRoC.yaml) against the same formulas in long double: at most 1 unit anywhere, at
    most 0.1 % of the pixels differing at all (measured: none differs), every pixel valid."""
    a = dict(K4=R.EUROC_K, D=R.EUROC_D, R=R.EUROC_R, P4=R.EUROC_P, src_size=R.EUROC_SIZE, dst_size=R.EUROC_SIZE)
    m, v, n = R.plan(**a)
    ml, vl, nl = R.plan(dtype=np.longdouble, **a)
    assert n == nl == 752 * 480 and v.all()
    d = np.abs(m.astype(np.int64) - ml.astype(np.int64)).max(-1)
    print("max difference", d.max(), "differing pixels", int((d > 0).sum()))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3


def test_euroc_small_reaches_every_fraction():
    m, v, n = R.plan(**R.euroc_small())
    assert n == 94 * 60
    assert set((m[..., 0] & 31).ravel()) == set(range(32)) and set((m[..., 1] & 31).ravel()) == set(range(32))


def test_ramp():
    """A source ramp S = x // 4 through the EuRoC map comes back within 1 grey level of the fixed-point source coordinate over 128,
    qx / 128 = 32 us / 128 = us / 4 (measured: 0.87)."""
    a = dict(K4=R.EUROC_K, D=R.EUROC_D, R=R.EUROC_R, P4=R.EUROC_P, src_size=R.EUROC_SIZE, dst_size=R.EUROC_SIZE)
    m, v, n, us, vs = R.plan(full=True, **a)
    S = (np.arange(752) // 4).astype(np.uint8)[None, :].repeat(480, 0)
    out = R.remap(S, m).astype(np.float64)
    err = np.abs(out - 32 * us / 128).max()
    print("ramp error", err)
    assert err <= 1.0


def test_rounding_of_the_weights():
    """taps of 0 and 255 with every weight pair: the + 512 >> 10 is round-half-up of the exact weighted mean"""
    src = np.array([[0, 255], [255, 0]], np.uint8)
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    m = np.stack([ax, ay], -1).astype(np.int32)
    out = R.remap(src, m)
    exact = (ax * (32 - ay) + (32 - ax) * ay) * 255 / 1024
    assert np.array_equal(out, np.floor(exact + 0.5).astype(np.uint8))


def test_colour_is_gray_then_remap():
    rng = np.random.default_rng(3)
    s = R.euroc_small()
    m, _, _ = R.plan(**s)
    for ch in (3, 4):
        for order in (0, 1):
            src = rng.integers(0, 256, (60, 94, ch), dtype=np.uint8)
            assert np.array_equal(R.remap(src, m, rgb_order=order), R.remap(R.gray(src, order), m))
    g = R.gray(np.array([[[255, 0, 0], [0, 0, 255]]], np.uint8), 1)
    assert g.tolist() == [[76, 29]]


def test_gate():
    valid = np.array([[1, 0, 0, 0, 1]], np.uint8)
    img = np.array([[np.nan, np.nan, 0.0, -0.0, -3.5]], np.float32)
    out, n = R.gate(img, valid)
    assert n == 2
    assert np.array_equal(out.view(np.uint32), np.array([[img.view(np.uint32)[0, 0], 0, 0, 0, img.view(np.uint32)[0, 4]]], np.uint32))
