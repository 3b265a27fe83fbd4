"""CPU: the NumPy restatement of the distance field (tests/distance_ref.py) against an all-pairs brute force over the site list, against SciPy's
Euclidean transform where it is installed, its site set against the crossings the dense restatement extracts, the R^2 edge, and the metric
distance on fused analytic surfaces."""
import numpy as np
import pytest

from tests import dense_ref as R
from tests import distance_ref as D
from tests import test_dense_ref as TD

FAR = D.FAR


def _whole(V):
    return V.origin, V.origin + np.array(V.n)


def _brute(site, radius):
    """d2 by all pairs: every voxel of the box against every site of the box, in int64"""
    zyx = np.argwhere(site).astype(np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in site.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    if len(zyx) == 0:
        return np.full(site.shape, FAR, np.uint32)
    best = np.full(len(grid), np.iinfo(np.int64).max, np.int64)
    for c in range(0, len(zyx), 64):
        d = grid[:, None, :] - zyx[None, c:c + 64, :]
        best = np.minimum(best, (d * d).sum(-1).min(1))
    return np.where(best <= radius * radius, best, FAR).astype(np.uint32).reshape(site.shape)


def _volumes():
    for n, k, radius in D.CASES:
        for origin in D.ORIGINS:
            yield D.sparse_volume(R, n, k, origin, seed=sum(n)), radius
    rng = np.random.default_rng(5)                          # the all-sites case: random signs
    V = R.Volume((9, 8, 7), 0.05, (3, -4, 5))
    t = rng.integers(-3000, 3000, V.words.shape)
    V.words = ((np.uint32(3) << 16) | t.astype(np.int16).view(np.uint16).astype(np.uint32)).astype(np.uint32)
    yield V, 4


def test_separable_minima_equal_the_brute_force():
    some_far = some_site = 0
    for V, radius in _volumes():
        lo, hi = _whole(V)
        for mw in (1, 2):
            for rr in sorted({1, 2, radius}):
                words, blo, bhi = D.field(V, lo, hi, mw, rr)
                site = D.sites(V, lo, hi, mw)
                assert np.array_equal(words & FAR, _brute(site, rr)), (V.n, mw, rr)
                assert np.array_equal((words & FAR) == 0, site)
                assert np.array_equal(words >> 28, D.state(V, lo, hi, mw)) and np.array_equal(blo, lo) and np.array_equal(bhi, hi)
                some_far += int(((words & FAR) == FAR).sum()); some_site += int(site.sum())
    assert some_far > 1000 and some_site > 100


def test_a_sub_box_ignores_sites_outside_it_but_keeps_sites_made_by_neighbours_outside_it():
    V = R.Volume((8, 6, 5), 0.05, (-3, 2, 7))
    V.words[:] = (2 << 16) | 3000
    V.words[9 % 5, 4 % 6, (-1) % 8] = (2 << 16) | (-3000 & 0xFFFF)      # the one negative voxel g = (-1, 4, 9)
    lo, hi = (0, 2, 7), (5, 8, 12)                           # g is one voxel outside the box on x; its neighbour (0, 4, 9) is inside
    words, blo, bhi = D.field(V, lo, hi, 1, 3)
    site = D.sites(V, lo, hi, 1)
    assert site.sum() == 1 and site[9 - 7, 4 - 2, 0]          # made a site by a neighbour outside the box but inside the volume
    assert np.array_equal(words & FAR, _brute(site, 3))
    assert (words & FAR)[2, 2, 1] == 1                       # measured to the site inside the box (1 voxel), not to g's other neighbours outside it


def test_scipy_agrees():
    ndi = pytest.importorskip("scipy.ndimage")
    for V, _ in _volumes():
        lo, hi = _whole(V)
        site = D.sites(V, lo, hi, 1)
        if not site.any():
            continue
        want = np.rint(ndi.distance_transform_edt(~site) ** 2).astype(np.uint32)
        words, _, _ = D.field(V, lo, hi, 1, 8191)
        assert np.array_equal(words & FAR, want), V.n


def test_sites_are_the_ends_of_the_crossings_extract_reports():
    for V, _ in _volumes():
        lo, hi = _whole(V)
        for mw in (1, 2):
            xyz, grad, wgt = V.extract(lo, hi, mw)
            ends = set()
            for p in xyz.astype(np.float64) / float(V.voxel) - 0.5:     # a crossing lies between the centres a and a + e_k, on the axis k alone
                k = int(np.argmax(np.abs(p - np.rint(p))))
                a = np.rint(p).astype(np.int64); a[k] = int(np.floor(p[k] + 1e-6))
                b = a.copy(); b[k] += 1
                ends.add(tuple(a)); ends.add(tuple(b))
            site = D.sites(V, lo, hi, mw)
            got = {tuple(int(v) for v in (np.array(z[::-1]) + lo)) for z in np.argwhere(site)}
            assert got == ends, (V.n, mw)


def test_the_radius_edge():
    """One site at a corner of 5^3 with R = 3: (3, 0, 0) and (2, 2, 1) hold 9, (3, 1, 0) holds 10 > 9: FAR"""
    V, lo, hi = D.corner_box()
    words, _, _ = D.field(V, lo, hi, 1, 3)
    d2 = words & FAR
    assert D.sites(V, lo, hi, 1).sum() == 1 and d2[0, 0, 0] == 0
    assert d2[0, 0, 3] == 9 and d2[1, 2, 2] == 9 and d2[0, 1, 3] == FAR
    assert (d2 != FAR).sum() == (_brute(D.sites(V, lo, hi, 1), 3) != FAR).sum()


@pytest.mark.parametrize("sphere", [None, TD.SPHERE])
def test_metric_distance_on_fused_surfaces(sphere):
    """Free voxels in front of a fused plane (and sphere): sqrt(d2) * voxel is within one voxel diagonal of the analytic distance up to the radius.  A
    site is a voxel centre at an end of a crossing edge, so within one voxel of the fused surface, which itself lies within the dense mapper's bound
    of the true one; only voxels whose nearest surface point was seen by the cameras can be asked, so the test keeps to the middle of the volume."""
    V, depths, hits = TD._fuse(TD.POSES, sphere)
    lo, hi = _whole(V)
    radius = 10
    words, _, _ = D.field(V, lo, hi, 2, radius)
    d2, st = (words & FAR).astype(np.int64), words >> 28
    gz, gy, gx = np.meshgrid(*[np.arange(lo[a], hi[a]) for a in (2, 1, 0)], indexing="ij")
    P = (np.stack([gx, gy, gz], -1) + 0.5) * float(V.voxel)
    true = TD._distance(P.reshape(-1, 3), sphere).reshape(d2.shape)
    mid = (np.abs(P[..., 0]) < 0.5) & (np.abs(P[..., 1]) < 0.4) & (P[..., 2] < TD.PLANE_Z)
    ask = mid & (st == 1) & (true <= (radius - 2) * float(V.voxel))
    if sphere is not None:                                  # the cameras saw the front of the sphere: its nearest point must lie well inside that cap
        C, rad = np.asarray(sphere[0]), sphere[1]
        r = np.linalg.norm(P - C, axis=-1)
        foot_z = C[2] + rad * (P[..., 2] - C[2]) / r
        ask &= (np.abs(P[..., 2] - TD.PLANE_Z) <= np.abs(r - rad)) | (foot_z < C[2] - 0.5 * rad)
    assert ask.sum() > 500
    assert np.all(d2[ask] != FAR)
    err = np.abs(np.sqrt(d2[ask]) * float(V.voxel) - true[ask])
    diag = np.sqrt(3.0) * float(V.voxel)
    print(f"{'sphere + plane' if sphere else 'plane'}: {int(ask.sum())} free voxels, worst error {err.max():.4f} m, voxel diagonal {diag:.4f} m")
    assert err.max() <= diag


def test_sample_names_the_voxel_of_a_point():
    V = D.sparse_volume(R, (17, 5, 9), 3, (-37, 5, -101), seed=31)
    lo, hi = _whole(V)
    words, lo, hi = D.field(V, lo, hi, 1, 3)
    vx = np.float32(V.voxel)
    g = np.array([[-37, 5, -101], [-21, 9, -93], [-38, 5, -101], [-20, 9, -93]], np.float32)
    pts = np.concatenate([g * vx, (g + np.float32(0.5)) * vx, [[np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [1e30, 0, 0], [-1e30, 0, 0]]]).astype(np.float32)
    got = D.sample(words, lo, hi, vx, pts)
    assert np.all(got[8:] == D.OUTSIDE) and got[6] == D.OUTSIDE and got[7] == D.OUTSIDE
    assert got[4] == words[0, 0, 0] and got[5] == words[8, 4, 16]
