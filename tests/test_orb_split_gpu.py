"""The split ORB device stage (k_compact + k_angle behind the candidates' event, orb.hip) at the edges it adds: cells near
their capacity, no candidate at all, empty cells and an empty top level, a handle reused from a full frame to an empty one,
_begin / _end called separately, and the descriptor kernel ordered behind the angle kernel.  Every result is bit-exact against
the oracle and against the one-kernel path with its copies (VDO_ORB_FUSED_ANGLE=1, read when the extractor is created: the
fused results come from a second extractor with the same settings)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import frontend_ref as R
from vdo_slam_amd import _capi as K
from vdo_slam_amd import synth_frames as SF
from vdo_slam_amd.frontend import KeypointsC, ORBextractor, OrbParamsC, _fp, _ip, _lib, _u8

pytestmark = pytest.mark.gpu

W, H = 128, 96
SMALL = OrbParamsC(300, 1.2, 3, 20, 7)
KITTI = OrbParamsC(2500, 1.2, 8, 20, 7)
KEYS = ("x", "y", "octave", "response", "size", "angle")


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def noise():
    return np.random.default_rng(11).integers(0, 256, (H, W), dtype=np.uint8)


def flat():
    return np.full((H, W), 90, np.uint8)


def corner():
    """Texture in the top-left 64x26 px only: most cells of levels 0 and 1 are empty (32 and 14 candidates on the oracle), and the
    FAST region of the top level (it starts 19 px inside the level, 27 px of the image) holds no corner at all."""
    g = np.full((H, W), 90, np.uint8)
    g[:26, :64] = np.random.default_rng(12).integers(0, 256, (26, 64), dtype=np.uint8)
    return g


IMAGES = {"noise": noise, "flat": flat, "corner": corner}


def make(ctx, w, h, prm, fused=False):
    if not fused:
        return ORBextractor(ctx, w, h, prm.n_features, prm.scale_factor, prm.n_levels, prm.ini_th, prm.min_th)
    os.environ["VDO_ORB_FUSED_ANGLE"] = "1"
    try:
        return ORBextractor(ctx, w, h, prm.n_features, prm.scale_factor, prm.n_levels, prm.ini_th, prm.min_th)
    finally:
        del os.environ["VDO_ORB_FUSED_ANGLE"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what, keys=KEYS):
    assert got["x"].size == want["x"].size, f"{what}: {got['x'].size} keypoints, want {want['x'].size}"
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k} ({int((bits(got[k]) != bits(want[k])).sum())} differ)"


def assert_candidates_same(a, b, n_levels, what):
    total = 0
    for l in range(n_levels):
        ca, cb = a.candidates(l), b.candidates(l)
        for name, u, v in zip(("x", "y", "resp", "angle"), ca, cb):
            assert u.size == v.size and np.array_equal(bits(u), bits(v)), f"{what}: level {l} candidate {name}"
        total += ca[0].size
    return total


def begin_end(orb, gray):
    """vdo_orb_extract_begin and _end as two calls (what the frame pipeline does around its other work)."""
    L = _lib()
    L.vdo_orb_extract_begin.argtypes = [C.c_void_p, K.c_uint8_p, C.c_int, C.c_int]
    L.vdo_orb_extract_end.argtypes = [C.c_void_p, C.POINTER(KeypointsC)]
    cap = orb.max_keypoints
    a = {k: np.zeros(max(cap, 1), np.float32) for k in ("x", "y", "response", "angle", "size")}
    octave = np.zeros(max(cap, 1), np.int32)
    kp = KeypointsC(cap, 0, _fp(a["x"]), _fp(a["y"]), _fp(a["response"]), _fp(a["angle"]), _fp(a["size"]), _ip(octave))
    K.check(L.vdo_orb_extract_begin(orb._h, _u8(gray), gray.strides[0], 0))
    K.check(L.vdo_orb_extract_end(orb._h, C.byref(kp)))
    out = {k: v[:kp.n].copy() for k, v in a.items()}
    out["octave"] = octave[:kp.n].copy()
    return out


@pytest.fixture(scope="module")
def pair(ctx):
    """One split and one fused extractor at 128x96, shared by the small cases (each case overwrites what the one before left)."""
    a, b = make(ctx, W, H, SMALL), make(ctx, W, H, SMALL, fused=True)
    yield a, b
    a.close(); b.close()


@pytest.mark.parametrize("name", list(IMAGES))
def test_small_images_equal_oracle_and_fused_path(oracle, pair, name):
    split, fused = pair
    gray = IMAGES[name]()
    want = R.extract_desc(oracle, gray, SMALL)
    got = split(gray, descriptors=True)
    assert_same(got, want, f"{name}: oracle", KEYS + ("desc",))
    fk = fused(gray, descriptors=True)
    assert_same(got, fk, f"{name}: fused path", KEYS + ("desc",))      # desc: k_orb_desc ran behind k_angle
    ncand = assert_candidates_same(split, fused, SMALL.n_levels, name)
    per_level = [split.level_info(l)[3] for l in range(SMALL.n_levels)]
    for l in range(SMALL.n_levels):                      # FAST candidates against the oracle, in order
        rx, ry, rr = R.fast_level(oracle, gray, l, SMALL)
        x, y, r, _ = split.candidates(l)
        assert np.array_equal(x, rx) and np.array_equal(y, ry) and np.array_equal(r, rr), f"{name}: FAST level {l}"
    assert_same(begin_end(split, gray), want, f"{name}: _begin / _end")
    if name == "noise":
        # uniform noise: a cell holds about one candidate per 3x3 px, the densest an image gives (the bound is one per 2x2)
        assert ncand > 600 and got["x"].size > 250
    elif name == "flat":
        assert ncand == 0 and got["x"].size == 0 and got["desc"].shape == (0, 32)
    else:
        assert per_level[0] > 0 and per_level[-1] == 0 and 0 < got["x"].size < 100, per_level


def test_noise_then_flat_on_one_handle_leaves_nothing_stale(oracle, pair):
    split, _ = pair
    a = split(noise())
    assert a["x"].size > 250
    b = split(flat())
    assert b["x"].size == 0
    assert all(split.candidates(l)[0].size == 0 for l in range(SMALL.n_levels))
    # and back: the rows are rewritten, not appended to
    assert_same(split(noise()), a, "noise after flat")
    c = split(corner())
    assert_same(c, R.extract(oracle, corner(), SMALL), "corner after noise: oracle")
    for l in range(SMALL.n_levels):
        x, y, r, ang = split.candidates(l)
        assert x.size == split.level_info(l)[3] and ang.size == x.size


def test_kitti_size_equals_oracle_and_fused_path(ctx, oracle):
    w, h = 1242, 375
    gray = SF.make_gray(6, w, h)
    split, fused = make(ctx, w, h, KITTI), make(ctx, w, h, KITTI, fused=True)
    try:
        got = split(gray, descriptors=True)
        want = R.extract_desc(oracle, gray, KITTI)
        assert want["x"].size > 1500
        assert_same(got, want, "oracle", KEYS + ("desc",))
        assert_same(got, fused(gray, descriptors=True), "fused path", KEYS + ("desc",))
        assert assert_candidates_same(split, fused, KITTI.n_levels, "1242x375") > 5000
        assert_same(begin_end(split, gray), want, "_begin / _end")
        # the separate descriptor call after _begin / _end reads the angles of that extraction
        assert np.array_equal(split.descriptors(want["x"].size), want["desc"])
    finally:
        split.close(); fused.close()
