"""CPU: the NumPy restatement of the dense mapper (tests/dense_ref.py) against hand cases that are exact in fp32, against the analytic surfaces of
rendered scenes, and its recentring against a from-scratch model keyed by global voxel."""
import numpy as np
import pytest

from tests import dense_ref as R

F = np.float32
I4 = np.eye(4, dtype=F)


def _pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    """world -> camera: a rotation about y and a translation"""
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = [tx, ty, tz]
    return T


def render(T, K4, W, H, plane_z, sphere=None):
    """Depth (float64 [H, W]) of the world plane z = plane_z and an optional sphere (centre, radius) seen from the world -> camera pose T, and the
    image of what was hit (0 plane, 1 sphere)"""
    fx, fy, cx, cy = K4
    Rm, t = T[:3, :3], T[:3, 3]
    ys, xs = np.mgrid[0:H, 0:W]
    r = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))], -1)
    d = (plane_z + Rm[:, 2] @ t) / (r @ Rm[:, 2])
    hit = np.zeros((H, W), np.int32)
    if sphere is not None:
        C, rad = sphere
        Cc = Rm @ np.asarray(C, float) + t
        a = (r * r).sum(-1); b = r @ Cc; c = Cc @ Cc - rad * rad
        disc = b * b - a * c
        ds = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
        hit = (ds < d).astype(np.int32)
        d = np.minimum(d, ds)
    return d, hit


def depth_term(depths, hits):
    """The largest depth difference between 4-neighbour pixels that hit the same surface and have no silhouette pixel beside them"""
    worst = 0.0
    for d, h in zip(depths, hits):
        edge = np.zeros_like(h, bool)
        edge[:, 1:] |= h[:, 1:] != h[:, :-1]; edge[:, :-1] |= h[:, 1:] != h[:, :-1]
        edge[1:, :] |= h[1:, :] != h[:-1, :]; edge[:-1, :] |= h[1:, :] != h[:-1, :]
        near = edge.copy()
        near[:, 1:] |= edge[:, :-1]; near[:, :-1] |= edge[:, 1:]; near[1:, :] |= edge[:-1, :]; near[:-1, :] |= edge[1:, :]
        for ax in (0, 1):
            dd = np.abs(np.diff(d, axis=ax))
            a = near[1:, :] | near[:-1, :] if ax == 0 else near[:, 1:] | near[:, :-1]
            if (~a).any():
                worst = max(worst, float(dd[~a].max()))
    return worst


# ---- hand cases, exact in fp32 ----------------------------------------------------------------------------------------------------------------
def _axis_volume():
    """One voxel whose centre (0.5, 0.5, 0.5) * 0.5 = (0.25, 0.25, 0.25) is moved onto the optical axis by T; a 1 x 1 image"""
    T = I4.copy(); T[0, 3] = -0.25; T[1, 3] = -0.25; T[2, 3] = 1.75          # camera coordinates (0, 0, 2)
    return R.Volume((1, 1, 1), 0.5), T, (8.0, 8.0, 0.0, 0.0)


@pytest.mark.parametrize("s,q", [(0.0, 0), (0.25, 16384), (0.5, 32767), (-0.25, -16383), (-0.5, -32767), (0.125, 8192), (3.0, 32767)])
def test_known_q_on_the_optical_axis(s, q):
    """d - Zc a power-of-two fraction of trunc = 0.5: q = floor(s / trunc * 32767 + 0.5) (0.25 -> 16383.5 + 0.5, -0.25 -> -16383.5 + 0.5 = -16383)"""
    V, T, K4 = _axis_volume()
    counts = V.integrate(np.full((1, 1), 2.0 + s, F), None, T, K4, 0.5, 0.0, 10.0, 255)
    assert counts == (1, 0, 0)
    assert int(V.t()[0, 0, 0]) == q and int(V.w()[0, 0, 0]) == 1


def test_running_mean_of_a_constant_and_weight_saturation():
    V, T, K4 = _axis_volume()
    for k in range(1, 301):
        assert V.integrate(np.full((1, 1), 2.125, F), None, T, K4, 0.5, 0.0, 10.0, 40) == (1, 0, 0)
        assert int(V.t()[0, 0, 0]) == 8192 and int(V.w()[0, 0, 0]) == min(k, 40)
    # at the cap the mean keeps moving: w / (w + 1) of the old value
    V.integrate(np.full((1, 1), 1.875, F), None, T, K4, 0.5, 0.0, 10.0, 40)
    assert int(V.t()[0, 0, 0]) == int(np.floor((8192 * 40 - 8191) / 41 + 0.5)) and int(V.w()[0, 0, 0]) == 40


def test_floor_div_rounds_towards_minus_infinity():
    a = np.array([-7, -6, -5, -1, 0, 1, 5, 6, 7, -65534 * 255 * 2 - 3])
    for d in (1, 2, 3, 6, 512):
        assert np.array_equal(R.floor_div(a, d), np.floor_divide(a, d))
    # the mean of -3 (w = 1) and -4: (-7 + 0.5 * 2) / 2 -> floor(-3.0) = -3; of -3 and -6: floor(-4.5 + 0.5) = -4
    assert int(R.floor_div(2 * (-3 * 1 + -4) + 2, 4)) == -3 and int(R.floor_div(2 * (-3 * 1 + -6) + 2, 4)) == -4


def test_skips_keep_the_word_and_are_counted():
    V, T, K4 = _axis_volume()
    V.integrate(np.full((1, 1), 2.0, F), None, T, K4, 0.5, 0.0, 10.0, 255)
    before = V.words.copy()
    assert V.integrate(np.full((1, 1), 2.0, F), np.ones((1, 1), np.int32), T, K4, 0.5, 0.0, 10.0, 255) == (0, 1, 0)
    assert V.integrate(np.full((1, 1), 1.25, F), None, T, K4, 0.5, 0.0, 10.0, 255) == (0, 0, 1)                  # s = -0.75 < -trunc
    for d in (0.0, -1.0, np.nan, np.inf, 10.5):
        assert V.integrate(np.full((1, 1), d, F), None, T, K4, 0.5, 0.0, 10.0, 255) == (0, 0, 0)
    assert np.array_equal(V.words, before)


# ---- accuracy on rendered scenes --------------------------------------------------------------------------------------------------------------
W, H = 80, 60
K4 = (70.0, 70.0, 39.5, 29.5)
VOXEL, TRUNC = 0.06, 0.24
PLANE_Z = 3.017
SPHERE = ((0.1, -0.05, 2.2), 0.45)
N = (56, 44, 40)
ORIGIN = (-28, -22, 28)                                                      # x, y around the axis; z from 1.68 m to 4.08 m
POSES = [_pose(), _pose(0.12, 0.0, 0.0, 0.02), _pose(-0.1, 0.06, 0.05, -0.03), _pose(0.05, -0.08, -0.04, 0.01), _pose(-0.15, -0.03, 0.0, 0.04)]


def _fuse(poses, sphere, masked=False, n=N, origin=ORIGIN):
    V = R.Volume(n, VOXEL, origin)
    depths, hits = [], []
    for T in poses:
        d, hit = render(T, K4, W, H, PLANE_Z, sphere)
        depths.append(d); hits.append(hit)
        V.integrate(d.astype(F), hit if masked else None, T.astype(F), K4, TRUNC, 0.0, 10.0, 64)
    return V, depths, hits


def _distance(xyz, sphere):
    p = xyz.astype(np.float64)
    dist = np.abs(p[:, 2] - PLANE_Z)
    if sphere is not None:
        C, rad = sphere
        dist = np.minimum(dist, np.abs(np.linalg.norm(p - np.asarray(C), axis=1) - rad))
    return dist


@pytest.mark.parametrize("n_poses", [3, 5])
def test_plane_accuracy(n_poses):
    V, depths, hits = _fuse(POSES[:n_poses], None)
    xyz, grad, wgt = V.extract(V.origin, V.origin + V.n, 2)
    bound = VOXEL + depth_term(depths, hits)
    dist = _distance(xyz, None)
    print(f"plane, {n_poses} poses: {len(xyz)} points, worst distance {dist.max():.4f} m, bound {bound:.4f} m")
    assert len(xyz) > 500 and dist.max() <= bound
    assert (wgt >= 2).all() and (wgt <= n_poses).all()
    inner = (np.abs(grad).sum(1) > 0)
    assert inner.mean() > 0.8 and (grad[inner, 2] < 0).all()                  # the distance falls along +z, towards the plane and through it


def test_fronto_parallel_crossing_is_exact_to_the_quantum():
    """Translations in x and y only: d - Zc is the same number in every view, the crossing on z lies within 2 * trunc / 32767 and a few ulp of the depth"""
    poses = [_pose(), _pose(0.12, 0.03), _pose(-0.09, 0.06), _pose(0.04, -0.07)]
    V, _, _ = _fuse(poses, None)
    xyz, grad, wgt = V.extract(V.origin, V.origin + V.n, 2)
    assert len(xyz) > 500
    err = np.abs(xyz[:, 2].astype(np.float64) - PLANE_Z)
    tol = 2 * TRUNC / 32767 + 8 * float(np.spacing(F(PLANE_Z)))
    print(f"fronto-parallel crossing: worst {err.max():.3e} m, tolerance {tol:.3e} m")
    assert err.max() <= tol
    centres = (np.floor(xyz[:, :2] / F(VOXEL)) + 0.5) * VOXEL               # every point is a z crossing: x and y are voxel centres
    assert np.abs(xyz[:, :2] - centres).max() < 1e-5


@pytest.mark.parametrize("n_poses", [3, 5])
def test_sphere_in_front_of_a_plane_accuracy(n_poses):
    V, depths, hits = _fuse(POSES[:n_poses], SPHERE)
    xyz, grad, wgt = V.extract(V.origin, V.origin + V.n, 2)
    bound = VOXEL + depth_term(depths, hits)
    dist = _distance(xyz, SPHERE)
    C, rad = SPHERE
    on_sphere = np.abs(np.linalg.norm(xyz.astype(np.float64) - np.asarray(C), axis=1) - rad) <= bound
    print(f"sphere + plane, {n_poses} poses: {len(xyz)} points ({int(on_sphere.sum())} on the sphere), worst distance {dist.max():.4f} m, bound {bound:.4f} m")
    assert on_sphere.sum() > 200 and dist.max() <= bound


def test_masked_sphere_leaves_no_point_and_no_carving():
    V, depths, hits = _fuse(POSES, SPHERE, masked=True)
    xyz, grad, wgt = V.extract(V.origin, V.origin + V.n, 2)
    bound = VOXEL + depth_term(depths, hits)
    assert len(xyz) > 500 and (np.abs(xyz[:, 2].astype(np.float64) - PLANE_Z) <= bound).all()       # every point lies on the plane, none on the sphere
    # the plane is not carved: a seen voxel clearly in front of the plane holds a positive distance, one clearly behind it a negative one
    gz = V.globals_of_slots(2)
    pz = ((gz + 0.5) * VOXEL)[:, None, None] * np.ones(V.words.shape)
    seen = V.w() > 0
    front = seen & (PLANE_Z - pz >= VOXEL); back = seen & (pz - PLANE_Z >= VOXEL)
    assert front.sum() > 1000 and back.sum() > 1000
    assert (V.t()[front] > 0).all() and (V.t()[back] < 0).all()
    # and the unmasked fusion of the same frames does put points on the sphere
    U, _, _ = _fuse(POSES, SPHERE)
    uxyz = U.extract(U.origin, U.origin + U.n, 2)[0]
    C, rad = SPHERE
    assert (np.abs(np.linalg.norm(uxyz.astype(np.float64) - np.asarray(C), axis=1) - rad) <= bound).sum() > 200


# ---- recentring against a from-scratch model keyed by global voxel -----------------------------------------------------------------------------
def _as_dict(V):
    out = {}
    g = [V.globals_of_slots(a) for a in range(3)]
    for sz in range(V.n[2]):
        for sy in range(V.n[1]):
            for sx in range(V.n[0]):
                if V.words[sz, sy, sx]:
                    out[(int(g[0][sx]), int(g[1][sy]), int(g[2][sz]))] = int(V.words[sz, sy, sx])
    return out


@pytest.mark.parametrize("shift", [(1, 0, 0), (-3, 2, -1), (0, 0, 0), (9, 0, 0), (0, -7, 0), (2, 3, 11), (12, -20, 40), (8, 6, 10)])
def test_recenter_equals_a_model_keyed_by_global_voxel(shift):
    n, o = (9, 7, 10), (-4, 3, -12)
    rng = np.random.default_rng(5)
    V = R.Volume(n, 0.1, o)
    V.words = rng.integers(1, 1 << 32, V.words.shape, dtype=np.uint64).astype(np.uint32)
    model = _as_dict(V)
    assert len(model) == 9 * 7 * 10
    q = tuple(o[a] + shift[a] for a in range(3))
    V.recenter(q)
    want = {g: w for g, w in model.items() if all(q[a] <= g[a] < q[a] + n[a] for a in range(3))}
    assert _as_dict(V) == want and tuple(V.origin) == q
    if any(abs(shift[a]) >= n[a] for a in range(3)):
        assert not V.words.any()
    # a voxel is found again at its slot
    for g, w in list(want.items())[:20]:
        assert int(V.at(g)) == w


def test_extract_order_and_neighbour_rules():
    """Two crossings made by hand: order z, y, x then axis; the neighbour may lie outside the box but not outside the volume; min_weight on both"""
    V = R.Volume((3, 2, 2), 0.5, (-1, 0, 0))

    def put(g, t, w):
        V.words[g[2] % 2, g[1] % 2, g[0] % 3] = (w << 16) | (t & 0xFFFF)
    put((-1, 0, 0), 100, 3); put((0, 0, 0), -300, 2); put((0, 1, 0), 50, 5); put((1, 0, 0), -10, 1)
    xyz, grad, wgt = V.extract((-1, 0, 0), (2, 2, 2), 2)
    # voxel (-1,0,0): x crossing with (0,0,0), frac = 100 / 400; voxel (0,0,0): y crossing with (0,1,0), frac = -300 / -350; its x neighbour has w = 1
    assert np.array_equal(xyz, np.array([[(-0.5 + 0.25) * 0.5, 0.25, 0.25], [0.25, (0.5 + F(-300) / F(-350)) * F(0.5), 0.25]], F))
    assert np.array_equal(wgt, [2, 2]) and not grad.any()
    assert len(V.extract((-1, 0, 0), (0, 1, 1), 2)[0]) == 1                  # the neighbour outside the box still counts
    assert len(V.extract((-1, 0, 0), (2, 2, 2), 3)[0]) == 0
    assert len(V.extract((5, 0, 0), (9, 2, 2), 1)[0]) == 0
