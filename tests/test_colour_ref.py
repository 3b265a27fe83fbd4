"""CPU: the colourer's restatement (tests/colour_ref.py) against an analytic truth.  A plane and a sphere that carry a linear colour ramp per channel
are rendered from a few poses (depth and colour), fused into the TSDF restatement and the colour restatement, and the colours sampled at the
extracted surface points must reproduce the ramp within a bound DERIVED below from the scene, not tuned to the error seen."""
import itertools

import numpy as np
import pytest

from tests import colour_ref as CR
from tests import dense_ref as R

F = np.float32
W, H, K4 = 80, 60, (80.0, 80.0, 39.5, 29.5)
N, ORIGIN, VOXEL = (48, 40, 24), (-24, -20, 12), 0.04
TRUNC, BAND, MIN_D, MAX_D, MAX_W = 0.16, 0.08, 0.0, 3.0, 64
# the ramp: colour_c(p) = BASE_c + SLOPE_c . p, levels and levels per metre; inside 0..255 over the scene (|x| < 1, |y| < 0.8, 0.5 < z < 1.5)
BASE = np.array([128.0, 120.0, 20.0])
SLOPE = np.array([[60.0, 0.0, 0.0], [0.0, 50.0, 30.0], [25.0, -20.0, 110.0]])


def ramp(p):
    return BASE + np.asarray(p, np.float64) @ SLOPE.T


def poses():
    out = []
    for k, (tilt, t) in enumerate(((0.0, (0, 0, 0)), (0.05, (0.06, 0.0, 0.02)), (-0.04, (-0.05, 0.04, 0.0)), (0.03, (0.0, -0.05, -0.03)))):
        c, s = np.cos(tilt), np.sin(tilt)
        T = np.eye(4)
        T[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, c, s], [0, -s, c]])
        T[:3, 3] = t
        out.append(T.astype(F))
    return out


def rays(T):
    """camera centre and the world-frame rays (camera-z component 1) of every pixel centre, float64"""
    T = np.asarray(T, np.float64)
    Rm, t = T[:3, :3], T[:3, 3]
    c = -Rm.T @ t
    ys, xs = np.mgrid[0:H, 0:W]
    dc = np.stack([(xs - K4[2]) / K4[0], (ys - K4[3]) / K4[1], np.ones((H, W))], -1)
    return c, dc @ Rm                                                                 # r = R^T d


def render_plane(T, n=(0.1, -0.05, 1.0), d0=1.0):
    c, r = rays(T)
    n = np.asarray(n)
    lam = (d0 - n @ c) / (r @ n)
    return finish(c, r, lam, np.ones((H, W), bool))


def render_sphere(T, centre=(0.0, 0.0, 1.3), radius=0.4):
    c, r = rays(T)
    oc = c - np.asarray(centre)
    a = (r * r).sum(-1); b = 2 * (r @ oc); cc = oc @ oc - radius * radius
    disc = b * b - 4 * a * cc
    hit = disc > 0
    lam = (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a)
    return finish(c, r, lam, hit)


def finish(c, r, lam, hit):
    p = c + lam[..., None] * r
    depth = np.where(hit & (lam > 0), lam, 0.0).astype(F)                             # the rays have camera-z 1: lam is the z-depth
    image = np.clip(np.floor(ramp(p) + 0.5), 0, 255).astype(np.uint8)
    image[depth == 0] = 0
    return depth, image


def fuse(render):
    V = R.Volume(N, VOXEL, ORIGIN); Cv = CR.ColourVolume(N, VOXEL, ORIGIN)
    for T in poses():
        depth, image = render(T)
        V.integrate(depth, None, T, K4, TRUNC, MIN_D, MAX_D, MAX_W)
        Cv.integrate(depth, None, image, T, K4, MIN_D, MAX_D, BAND, MAX_W)
    return V, Cv


def ramp_bound():
    """Per channel.  A sampled colour is a weighted mean of corner voxels' colours; a corner is at most one voxel diagonal from the sample point; a
    voxel's colour is a mean of pixels whose surface point lies on the pixel's ray within `band` of z-depth of the voxel - band * |r| in space, |r|
    the length of the longest ray with camera-z 1 - and whose ray passes the voxel centre within half a pixel diagonal at the farthest depth in the
    scene.  The ramp is linear: its change over that distance is at most |slope| times it.  Plus 1 for the roundings."""
    rmax = np.sqrt(1 + (max(K4[2], W - 1 - K4[2]) / K4[0]) ** 2 + (max(K4[3], H - 1 - K4[3]) / K4[1]) ** 2)
    diag = np.sqrt(3.0) * VOXEL
    footprint = 0.5 * np.sqrt(K4[0] ** -2 + K4[1] ** -2) * ((ORIGIN[2] + N[2]) * VOXEL) * rmax
    return np.linalg.norm(SLOPE, axis=1) * (BAND * rmax + diag + footprint) + 1.0


@pytest.mark.parametrize("scene", ["plane", "sphere"])
def test_the_ramp_comes_back_at_the_surface(scene):
    V, Cv = fuse(render_plane if scene == "plane" else render_sphere)
    o = list(ORIGIN)
    xyz, _, _ = V.extract(o, [o[a] + N[a] for a in range(3)], 2)
    assert len(xyz) > 200
    rgba = Cv.sample(xyz, 1)
    has = rgba[:, 3] > 0
    err = np.abs(rgba[has, :3].astype(np.float64) - ramp(xyz[has]))
    bound = ramp_bound()
    print(f"{scene}: {has.sum()} of {len(xyz)} surface points coloured, max error per channel {err.max(0)}, bound {bound}")
    assert has.mean() > 0.5
    assert np.all(err.max(0) <= bound), f"{err.max(0)} against {bound}"
    assert np.all(bound < 40)                                                         # the bound says something: far below the ramp's span over the scene


def test_a_constant_volume_samples_to_its_colour():
    rng = np.random.default_rng(0)
    Cv = CR.ColourVolume((9, 7, 5), 0.1, (-4, 3, -2))
    Cv.words[:] = np.uint32(12 | 200 << 8 | 255 << 16 | 5 << 24)
    o, n = np.array([-4, 3, -2]), np.array([9, 7, 5])
    inner = ((o + 0.5) + rng.random((2000, 3)) * (n - 1)) * 0.1                       # between the outermost voxel centres: all eight corners inside
    rgba = Cv.sample(inner.astype(F), 5)
    assert np.all(rgba == np.array([12, 200, 255, 255], np.uint8))
    assert not Cv.sample(inner.astype(F), 6).any()                                    # min_weight above every weight: S == 0
    # anywhere the colour is the constant or nothing, and alpha is below 255 exactly where a corner is outside
    wide = ((o - 1.0) + rng.random((4000, 3)) * (n + 2)) * 0.1
    rgba = Cv.sample(wide.astype(F), 1)
    some = rgba[:, 3] > 0
    assert np.all(rgba[some, :3] == np.array([12, 200, 255], np.uint8)) and 0 < some.sum() < len(wide)
    u = wide.astype(F) / F(0.1) - F(0.5)
    b = np.floor(u)
    all_in = np.all((b >= o) & (b + 1 <= o + n - 1), axis=1)
    assert np.all(rgba[all_in, 3] == 255) and all_in.sum() > 500


def test_alpha_is_the_share_of_the_weight_with_colour():
    Cv = CR.ColourVolume((4, 4, 4), 1.0, (0, 0, 0))
    Cv.words[1, 1, 1] = np.uint32(50 | 60 << 8 | 70 << 16 | 1 << 24)
    # at the voxel's centre all the weight is its own; midway to a neighbour on one axis half of it, on two a quarter, on three an eighth
    for p, alpha in (((1.5, 1.5, 1.5), 255), ((2.0, 1.5, 1.5), 128), ((2.0, 2.0, 1.5), 64), ((2.0, 2.0, 2.0), 32), ((2.49, 2.49, 2.49), 1), ((2.5, 2.5, 2.5), 0)):
        got = Cv.sample(np.array([p], F), 1)[0]
        assert got[3] == alpha and tuple(got[:3]) == ((50, 60, 70) if alpha else (0, 0, 0)), (p, got)


def test_the_running_mean_rounds_to_nearest_and_saturates():
    Cv = CR.ColourVolume((1, 1, 1), 1.0, (0, 0, 0))
    T = np.eye(4, dtype=F); T[2, 3] = 1.0                                             # the one voxel centre lies 1.5 ahead
    depth = np.full((3, 3), 1.5, F)
    seen = []
    for v in (0, 255, 1, 1, 1):
        assert Cv.integrate(depth, None, np.full((3, 3), v, np.uint8), T, (2.0, 2.0, 1.0, 1.0), 0.0, 5.0, 0.25, 3) == (1, 0, 0)
        seen.append((int(Cv.words[0, 0, 0]) & 255, int(Cv.words[0, 0, 0]) >> 24))
    assert seen == [(0, 1), (128, 2), (86, 3), (65, 3), (49, 3)]


def test_follow_against_a_relabelling():
    rng = np.random.default_rng(1)
    n = (7, 5, 4)
    for o, q in itertools.product(((0, 0, 0), (-9, 13, -2)), ((5, -3, 2), (0, 0, 1), (-6, 4, -3), (7, 0, 0), (0, -5, 0), (1, 1, -4), (-20, 30, 9), (0, 0, 0))):
        Cv = CR.ColourVolume(n, 0.1, o)
        Cv.words = rng.integers(1, 1 << 32, n[::-1], dtype=np.uint64).astype(np.uint32)
        before = {}
        for g in itertools.product(*[range(o[a], o[a] + n[a]) for a in range(3)]):
            before[g] = int(Cv.words[g[2] % n[2], g[1] % n[1], g[0] % n[0]])
        new = [o[a] + q[a] for a in range(3)]
        Cv.follow(new)
        assert tuple(Cv.origin) == tuple(new)
        for g in itertools.product(*[range(new[a], new[a] + n[a]) for a in range(3)]):
            assert int(Cv.words[g[2] % n[2], g[1] % n[1], g[0] % n[0]]) == before.get(g, 0), (o, q, g)
        if any(abs(q[a]) >= n[a] for a in range(3)):
            assert not Cv.words.any()


def test_pack():
    im = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    assert CR.pack(im, 0)[1, 2] == 20 | 21 << 8 | 22 << 16 and CR.pack(im, 1)[1, 2] == 22 | 21 << 8 | 20 << 16
    assert np.array_equal(CR.pack(im[:, :, :3], 1), CR.pack(im, 1))                   # the fourth channel is ignored
    assert np.array_equal(CR.pack(im[:, :, 0]), CR.pack(im[:, :, :1])) and CR.pack(im[:, :, 0])[0, 1] == 4 * 0x010101
