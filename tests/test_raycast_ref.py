"""CPU: the NumPy restatement of the raycaster (tests/raycast_ref.py) against hand cases that are exact in fp32, against the analytic depth and
normal of planes and a sphere fused with tests/dense_ref.py, its coverage from the fusing pose, and its independence of the cyclic layout."""
import numpy as np
import pytest

from tests import dense_ref as R
from tests import raycast_ref as RC
from tests import test_dense_ref as D

F = np.float32
I4 = np.eye(4, dtype=F)


def _words(t, w):
    return ((np.asarray(w, np.int64) << 16) | (np.asarray(t, np.int64) & 0xFFFF)).astype(np.uint32)


# ---- hand cases, exact in fp32 ----------------------------------------------------------------------------------------------------------------
def _axis_pose(cx, cy, cz):
    T = I4.copy(); T[0, 3] = -cx; T[1, 3] = -cy; T[2, 3] = -cz               # the camera centre is (cx, cy, cz), looking along +z
    return T


def test_two_slabs_give_the_depth_in_closed_form():
    """2 x 2 x 2, voxel 1: +1000 at the centres z = 0.5, -1000 at z = 1.5.  The ray x = y = 1 from z = -1 samples z = 0.25 (b = -1: invalid), 0.75
    (f = 0.25: F = 500), 1.25 (F = -500): depth = 1.75 + 0.5 * (500 / 1000) = 2, the plane z = 1 between the centres.  No gradient: n < 4."""
    V = R.Volume((2, 2, 2), 1.0)
    V.words[0] = _words(1000, 2); V.words[1] = _words(-1000, 3)
    depth, grad, wgt, counts = RC.render(V, 1, 1, (8.0, 8.0, 0.0, 0.0), 1.25, 0.5, 3, 2, _axis_pose(1.0, 1.0, -1.0))
    assert depth[0, 0] == F(2.0) and wgt[0, 0] == 2 and not grad.any() and counts == (1, 0, 0)
    # two samples are not enough to reach the crossing, a larger min_weight leaves no valid sample, and the reversed signs are no hit
    assert RC.render(V, 1, 1, (8.0, 8.0, 0.0, 0.0), 1.25, 0.5, 2, 2, _axis_pose(1.0, 1.0, -1.0))[3] == (0, 1, 0)
    assert RC.render(V, 1, 1, (8.0, 8.0, 0.0, 0.0), 1.25, 0.5, 3, 3, _axis_pose(1.0, 1.0, -1.0))[3] == (0, 0, 1)
    V.words[0] = _words(-1000, 2); V.words[1] = _words(1000, 3)
    depth, grad, wgt, counts = RC.render(V, 1, 1, (8.0, 8.0, 0.0, 0.0), 1.25, 0.5, 3, 2, _axis_pose(1.0, 1.0, -1.0))
    assert depth[0, 0] == 0 and wgt[0, 0] == 0 and counts == (0, 1, 0)


@pytest.mark.parametrize("origin", [(0, 0, 0), (-2, 5, -1), (1, 1, 1)])
def test_a_linear_field_gives_depth_and_gradient_in_closed_form(origin):
    """4 x 4 x 4, voxel 1, t = 300 - 200 * (gz - oz): zero at the plane z = oz + 2.  From z = oz - 1 with near 1 and step 0.5 the samples read
    300, 200, 100, 0: the hit lies between the last two, depth = 2.5 + 0.5 * (100 / 100) = 3; the gradient is two cells of -200 along z."""
    o = np.array(origin)
    V = R.Volume((4, 4, 4), 1.0, origin)
    gz = V.globals_of_slots(2)
    V.words[:] = _words(300 - 200 * (gz - o[2]), 4 + (gz - o[2]))[:, None, None]
    T = _axis_pose(o[0] + 2.0, o[1] + 2.0, o[2] - 1.0)
    depth, grad, wgt, counts = RC.render(V, 1, 1, (8.0, 8.0, 0.0, 0.0), 1.0, 0.5, 8, 1, T)
    assert depth[0, 0] == F(3.0) and wgt[0, 0] == 5 and counts == (1, 0, 0)
    assert np.array_equal(grad[0, 0], np.array([0, 0, -400], F))
    assert np.array_equal(RC.normals(grad)[0, 0], np.array([0, 0, -1], F))
    # one cell off the axis in x the cell b - e_x would lie outside: the depth stays, the gradient is 0
    T = _axis_pose(o[0] + 1.0, o[1] + 2.0, o[2] - 1.0)
    depth, grad, wgt, counts = RC.render(V, 1, 1, (8.0, 8.0, 0.0, 0.0), 1.0, 0.5, 8, 1, T)
    assert depth[0, 0] == F(3.0) and not grad.any()


def test_non_finite_poses_have_no_valid_sample():
    V = R.Volume((4, 4, 4), 1.0)
    V.words[:] = _words(100, 5)
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 3), (2, 2), (1, 0)):
            T = _axis_pose(2.0, 2.0, -1.0); T[at] = bad
            depth, grad, wgt, counts = RC.render(V, 3, 2, (8.0, 8.0, 1.0, 0.5), 1.0, 0.5, 8, 1, T)
            assert counts == (0, 0, 6) and not depth.any() and not grad.any() and not wgt.any()


# ---- accuracy on fused planes ------------------------------------------------------------------------------------------------------------------
W, H = 48, 32
K4 = (40.0, 40.0, 23.5, 15.5)
VOXEL, TRUNC = 0.1, 0.4
N, ORIGIN = (64, 48, 40), (-32, -24, 30)                                     # x from -3.2 m, y from -2.4 m, z from 3 m to 7 m
NEAR, STEP, STEPS = 3.0, 0.2, 25
PLANES = {"fronto": (np.array([0.0, 0.0, 1.0]), 5.0), "tilted": (np.array([-0.2, 0.0, 1.0]), 5.0)}      # n . X = d: z = 5, z = 5 + 0.2 x


def _pose(yaw_deg, shift):
    T = np.eye(4)
    a = np.deg2rad(yaw_deg); c, s = np.cos(a), np.sin(a)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = shift
    return T


VIEWS = {"fusing": np.eye(4), "rotated": _pose(10.0, (0.3, 0.0, 0.0))}


def analytic(T, plane):
    """float64 [H, W]: the z-depth at which the ray of every pixel meets the plane n . X = d, and the rays (world) and the camera centre"""
    n, d = plane
    Rm, t = T[:3, :3], T[:3, 3]
    c = -Rm.T @ t
    ys, xs = np.mgrid[0:H, 0:W]
    rc = np.stack([(xs - K4[2]) / K4[0], (ys - K4[3]) / K4[1], np.ones((H, W))], -1)
    rw = rc @ Rm                                                              # R^T r per pixel
    return (d - n @ c) / (rw @ n), rw, c


_fused = {}


def fused(name):
    """The plane fused 4 times from the fusing pose (computed once, never changed)"""
    if name not in _fused:
        V = R.Volume(N, VOXEL, ORIGIN)
        d = analytic(np.eye(4), PLANES[name])[0].astype(F)
        for _ in range(4):
            V.integrate(d, None, I4, K4, TRUNC, 0.0, 10.0, 64)
        V.words.setflags(write=False)
        _fused[name] = V
    return _fused[name]


_rendered = {}


def rendered(name, view):
    if (name, view) not in _rendered:
        _rendered[name, view] = RC.render(fused(name), W, H, K4, NEAR, STEP, STEPS, 2, VIEWS[view].astype(F))
    return _rendered[name, view]


@pytest.mark.parametrize("view", ["fusing", "rotated"])
@pytest.mark.parametrize("name", ["fronto", "tilted"])
def test_plane_depth_within_one_voxel_edge(name, view):
    """Every hit within one voxel edge (100 mm) of the analytic ray / plane depth.  Measured largest error: fronto below 0.01 mm from both
    poses, tilted 6.79 mm (fusing) and 7.91 mm (rotated)."""
    depth, grad, wgt, counts = rendered(name, view)
    exact = analytic(VIEWS[view], PLANES[name])[0]
    hit = depth > 0
    err = np.abs(depth.astype(np.float64) - exact)[hit]
    print(f"{name} plane, {view} pose: {int(hit.sum())} of {W * H} rays hit, largest depth error {1e3 * err.max():.2f} mm, bound {1e3 * VOXEL:.0f} mm")
    assert counts[0] == hit.sum() and sum(counts) == W * H
    assert hit.sum() > 1000 and err.max() <= VOXEL
    assert ((wgt >= 2) & (wgt <= 4))[hit].all() and not wgt[~hit].any()


@pytest.mark.parametrize("name", ["fronto", "tilted"])
def test_coverage_from_the_fusing_pose(name):
    """Every pixel at least 3 px inside the image whose surface point lies at least 2 voxels inside the volume is hit (measured: 0 missed)"""
    depth = rendered(name, "fusing")[0]
    exact, rw, c = analytic(np.eye(4), PLANES[name])
    P = c + exact[..., None] * rw
    lo = (np.array(ORIGIN) + 2) * VOXEL; hi = (np.array(ORIGIN) + np.array(N) - 2) * VOXEL
    inside = ((P >= lo) & (P <= hi)).all(-1)
    inner = np.zeros((H, W), bool); inner[3:H - 3, 3:W - 3] = True
    must = inside & inner
    print(f"{name} plane: {int(must.sum())} pixels must hit, {int((must & ~(depth > 0)).sum())} missed")
    assert must.sum() > 800 and (depth > 0)[must].all()


@pytest.mark.parametrize("view", ["fusing", "rotated"])
@pytest.mark.parametrize("name", ["fronto", "tilted"])
def test_plane_normals_within_five_degrees(name, view):
    """normals(grad) within 5 degrees of the plane's normal towards free space, off the border of what was hit.  Measured largest angle: fronto 0.000 deg
    from both poses, tilted 4.705 deg (fusing) and 4.798 deg (rotated)."""
    depth, grad, wgt, counts = rendered(name, view)
    nrm = RC.normals(grad).astype(np.float64)
    have = np.abs(nrm).sum(-1) > 0
    hit = depth > 0
    off = hit.copy()                                                          # off the border: the 3 x 3 neighbourhood is hit as well
    off[1:, :] &= hit[:-1, :]; off[:-1, :] &= hit[1:, :]; off[:, 1:] &= hit[:, :-1]; off[:, :-1] &= hit[:, 1:]
    off[0, :] = off[-1, :] = False; off[:, 0] = off[:, -1] = False
    n = -PLANES[name][0] / np.linalg.norm(PLANES[name][0])
    sel = off & have
    ang = np.degrees(np.arccos(np.clip(nrm[sel] @ n, -1, 1)))
    print(f"{name} plane, {view} pose: {int(sel.sum())} normals of {int(off.sum())} pixels off the border, largest angle {ang.max():.3f} deg")
    assert sel.sum() > 0.8 * off.sum() and sel.sum() > 700 and ang.max() <= 5.0


# ---- a sphere in front of a plane (the scene of test_dense_ref.py) -------------------------------------------------------------------------------
def test_sphere_in_front_of_a_plane():
    """Every hit point within one voxel edge plus the local depth step off the silhouette of the nearer surface - the condition test_dense_ref.py puts on
    the extracted points.  Measured: worst 16.5 mm against 94.4 mm, 631 of 4309 hits on the sphere."""
    V, depths, hits = D._fuse(D.POSES, D.SPHERE)
    T = D.POSES[0]
    depth, grad, wgt, counts = RC.render(V, D.W, D.H, D.K4, 1.5, D.TRUNC / 2, 23, 2, T.astype(F))
    bound = D.VOXEL + D.depth_term(depths[:1], hits[:1])
    ys, xs = np.mgrid[0:D.H, 0:D.W]
    r = np.stack([(xs - D.K4[2]) / D.K4[0], (ys - D.K4[3]) / D.K4[1], np.ones((D.H, D.W))], -1)
    hit = depth > 0
    P = (depth.astype(np.float64)[..., None] * r)[hit]                        # POSES[0] is the identity
    dist = D._distance(P, D.SPHERE)
    C, rad = D.SPHERE
    on_sphere = np.abs(np.linalg.norm(P - np.asarray(C), axis=1) - rad) <= bound
    print(f"sphere + plane: {int(hit.sum())} rays hit ({int(on_sphere.sum())} on the sphere), worst distance {1e3 * dist.max():.1f} mm, bound {1e3 * bound:.1f} mm")
    assert hit.sum() > 2000 and on_sphere.sum() > 500 and dist.max() <= bound


# ---- the cyclic layout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(3, 0, 0), (0, -2, 0), (0, 0, 5), (-5, 3, -4), (7, 7, 7)])
def test_recenter_leaves_the_render_of_the_surviving_region_unchanged(shift):
    """After Volume.recenter the render equals, bit for bit, the render of a volume built from scratch at the new origin from the surviving voxels (another
    slot layout, the same global voxels); and every ray that still hits keeps the depth, gradient-or-zero and weight bits it had before."""
    V0 = fused("tilted")
    T = VIEWS["rotated"].astype(F)
    before = rendered("tilted", "rotated")
    V = R.Volume(N, VOXEL, ORIGIN); V.words = V0.words.copy()
    q = tuple(ORIGIN[a] + shift[a] for a in range(3))
    V.recenter(q)
    Vs = R.Volume(N, VOXEL, q)
    g0 = [V0.globals_of_slots(a) for a in range(3)]
    for a in range(3):
        assert set(Vs.globals_of_slots(a)) == set(range(q[a], q[a] + N[a]))
    G = np.meshgrid(g0[2], g0[1], g0[0], indexing="ij")
    stay = np.ones(V0.words.shape, bool)
    for a, g in zip((2, 1, 0), G):
        stay &= (g >= q[a]) & (g < q[a] + N[a])
    Vs.words[G[0][stay] % N[2], G[1][stay] % N[1], G[2][stay] % N[0]] = V0.words[stay]
    assert np.array_equal(Vs.words, V.words)
    after = RC.render(V, W, H, K4, NEAR, STEP, STEPS, 2, T)
    hit = after[0] > 0
    assert hit.sum() > 500 and after[3][0] == hit.sum()
    assert np.array_equal(after[0].view(np.uint32)[hit], before[0].view(np.uint32)[hit]) and np.array_equal(after[2][hit], before[2][hit])
    both = hit & (np.abs(after[1]).sum(-1) > 0)
    assert both.sum() > 300 and np.array_equal(after[1].view(np.uint32)[both], before[1].view(np.uint32)[both])
