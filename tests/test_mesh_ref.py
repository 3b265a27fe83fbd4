"""CPU: the NumPy restatement of the mesher's contract (tests/mesh_ref.py) has the properties a surface-nets mesh must have - closed and oriented
on a closed surface, close to a plane, open only next to unseen voxels, and an exact partition of the quads by the two box modes."""
import collections
import time

import numpy as np
import pytest

from tests import mesh_ref as M

F = np.float32
VOXEL = 0.1


def _edges(tri):
    und, dire = collections.Counter(), collections.Counter()
    for a, b, c in np.asarray(tri).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            und[(min(p, q), max(p, q))] += 1; dire[(p, q)] += 1
    return und, dire


def _sphere(n=20, r=6.2, centre=(10.3, 9.8, 10.1)):
    return M.sdf_words((n, n, n), lambda g: np.linalg.norm(g - np.array(centre), axis=-1) - r)


def _whole(V, outside=0, min_weight=1, info=None):
    o = [int(v) for v in V.origin]
    return M.mesh(V, o, [o[a] + V.n[a] for a in range(3)], outside, min_weight, info)


def _signed_volume(xyz, tri):
    P = xyz.astype(np.float64) / VOXEL
    return float(np.einsum("ij,ij->i", P[tri[:, 0]], np.cross(P[tri[:, 1]], P[tri[:, 2]])).sum() / 6)


@pytest.mark.parametrize("centre", [(10.3, 9.8, 10.1), (10.0, 10.0, 10.0), (9.55, 10.45, 10.25)])
def test_sphere_is_closed_oriented_and_of_the_right_volume(centre):
    r = 6.2
    V = M.make_volume((20, 20, 20), (0, 0, 0), _sphere(20, r, centre), np.full((20, 20, 20), 2), VOXEL)
    xyz, grad, wgt, tri = _whole(V, min_weight=2)
    if centre == (10.3, 9.8, 10.1):
        assert (len(xyz), len(tri)) == (714, 1424)
    und, dire = _edges(tri)
    assert set(und.values()) == {2} and set(dire.values()) == {1}              # every edge shared by two triangles, once per direction
    assert len(xyz) - len(und) + len(tri) == 2
    vol, want = _signed_volume(xyz, tri), 4 / 3 * np.pi * r ** 3
    print(f"sphere at {centre}: signed volume {vol:.1f} voxel^3 against {want:.1f} ({100 * (vol / want - 1):+.2f} %)")
    assert vol > 0 and abs(vol / want - 1) < 0.05
    assert np.all(wgt == 2)
    # the gradient points towards free space: away from the centre
    out = xyz.astype(np.float64) / VOXEL - np.array(centre)
    assert np.all(np.einsum("ij,ij->i", out, grad.astype(np.float64)) > 0)


def test_tilted_plane():
    """Surface nets put a vertex at the mean of crossings that all lie ON the plane up to the rounding of t and the linear interpolation, which is
    exact for a plane: the restatement gives a largest distance of 5.6e-5 voxels and a largest angle of 0.003 degrees here (printed below); the bounds
    are the contract's half voxel and 2 degrees."""
    nrm = np.array([0.35, -0.5, 0.79]); nrm /= np.linalg.norm(nrm)
    d0 = float(nrm @ np.array([8.2, 7.7, 8.4]))
    n = (17, 16, 18)
    t = M.sdf_words(n, lambda g: g @ nrm - d0)
    V = M.make_volume(n, (-5, 3, -40), t, np.full(n[::-1], 3), VOXEL)
    xyz, grad, wgt, tri = _whole(V)
    assert len(xyz) > 200 and len(tri) > 300
    P = xyz.astype(np.float64) / VOXEL - np.array([-5, 3, -40])
    dist = np.abs(P @ nrm - d0)
    g = grad.astype(np.float64); g /= np.linalg.norm(g, axis=1)[:, None]
    ang = np.degrees(np.arccos(np.clip(g @ nrm, -1, 1)))
    print(f"plane: largest distance {dist.max():.2e} voxels, largest angle {ang.max():.3f} degrees")
    assert dist.max() < 0.5 and ang.max() < 2.0
    und, dire = _edges(tri)
    assert set(und.values()) <= {1, 2} and set(dire.values()) == {1}


def test_unseen_voxels_open_the_mesh_only_beside_them():
    w = np.full((20, 20, 20), 2)
    w[14:, 10:13, 10:13] = 0                                                   # [z, y, x]: a block of unseen voxels through the surface
    V = M.make_volume((20, 20, 20), (0, 0, 0), _sphere(), w, VOXEL)
    info = {}
    xyz, grad, wgt, tri = _whole(V, min_weight=2, info=info)
    und, dire = _edges(tri)
    assert set(und.values()) == {1, 2} and set(dire.values()) == {1}
    valid, cell = info["valid"], info["cell"]
    pad = np.pad(valid, 1, constant_values=True)                               # (cells outside the volume do not count: the sphere does not reach them)
    near_invalid = np.zeros(valid.shape, bool)
    for dz in (0, 1, 2):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                near_invalid |= ~pad[dz:dz + valid.shape[0], dy:dy + valid.shape[1], dx:dx + valid.shape[2]]
    n1 = 0
    for (p, q), cnt in und.items():
        if cnt == 1:
            n1 += 1
            assert any(near_invalid[cell[v][2], cell[v][1], cell[v][0]] for v in (p, q))
    assert n1 > 0


BOXES = [((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (20, 20, 20)), ((-9, -9, -9), (99, 99, 99)), ((9, 0, 0), (10, 20, 20)), ((0, 0, 11), (20, 20, 12)), ((3, 4, 5), (15, 13, 17)),
         ((0, 0, 0), (20, 9, 20)), ((5, 0, 0), (20, 20, 20)), ((50, 50, 50), (60, 60, 60)), ((8, 8, 8), (11, 11, 11))]


@pytest.mark.parametrize("origin", [(0, 0, 0), (-7, 13, -26)])
def test_the_two_modes_partition_the_quads(origin):
    rng = np.random.default_rng(3)
    t = _sphere() + rng.integers(-300, 300, (20, 20, 20))
    w = np.full((20, 20, 20), 2); w[rng.random((20, 20, 20)) < 0.01] = 0
    V = M.make_volume((20, 20, 20), origin, t, w, VOXEL)
    xyz, _, _, tri = _whole(V, min_weight=2)
    whole = M.sorted_rows(M.quads_of(xyz, tri))
    assert len(whole) > 500
    for lo, hi in BOXES:
        lo = [lo[a] + origin[a] for a in range(3)]; hi = [hi[a] + origin[a] for a in range(3)]
        xi, _, _, ti = M.mesh(V, lo, hi, 0, 2)
        xo, _, _, to = M.mesh(V, lo, hi, 1, 2)
        for x, tr in ((xi, ti), (xo, to)):
            assert len(tr) == 0 or (tr.min() >= 0 and tr.max() < len(x))
        both = M.sorted_rows(np.concatenate([M.quads_of(xi, ti), M.quads_of(xo, to)]))
        assert np.array_equal(both, whole), f"box {lo} .. {hi}"
    xo, _, _, to = M.mesh(V, (0, 0, 0), (0, 0, 0), 1, 2)                        # an empty box with `outside`: the whole volume, the same numbering
    assert np.array_equal(xo.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(to, tri)


def _ambiguous_cells(t):
    """cells [z, y, x] with a face whose diagonal corners agree in sign and whose neighbours differ"""
    neg = t < 0
    c = {d: M._corner(neg, d) for d in [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]}
    amb = np.zeros(c[(0, 0, 0)].shape, bool)
    for axis in range(3):
        i, j = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            def at(di, dj):
                d = [0, 0, 0]; d[axis] = side; d[i] = di; d[j] = dj
                return c[tuple(d)]
            amb |= (at(0, 0) == at(1, 1)) & (at(0, 1) == at(1, 0)) & (at(0, 0) != at(0, 1))
    return amb


def test_random_words_keep_the_index_and_order_invariants():
    rng = np.random.default_rng(11)
    n = (13, 7, 9)
    t = rng.integers(-32767, 32768, n[::-1]); t[rng.random(n[::-1]) < 0.05] = 0
    w = rng.integers(1, 256, n[::-1]); w[rng.random(n[::-1]) < 0.03] = 0
    V = M.make_volume(n, (4, -9, 100), t, w, VOXEL)
    info = {}
    xyz, grad, wgt, tri = _whole(V, info=info)
    cell = info["cell"]
    assert len(xyz) > 300 and len(tri) % 2 == 0 and tri.min() >= 0 and tri.max() < len(xyz)
    lin = (cell[:, 2] * (n[1] - 1) + cell[:, 1]) * (n[0] - 1) + cell[:, 0]
    assert np.all(np.diff(lin) > 0)                                             # vertices in the order z, y, x of their cells, none twice
    q = tri.reshape(-1, 2, 3)
    assert np.array_equal(q[:, 0, 0], q[:, 1, 0]) and np.array_equal(q[:, 0, 2], q[:, 1, 1])      # (v0, v1, v2), (v0, v2, v3)
    # the lattice edge of a quad from its four cells: a = the componentwise largest lower corner, k the one axis on which the four agree; the
    # quads come in the order of (a, k)
    cq = cell[np.concatenate([q[:, 0, :], q[:, 1, 2:3]], 1)]                     # [quads, 4, 3]
    same = np.all(cq == cq[:, :1, :], 1)
    assert np.all(same.sum(1) == 1)
    a = cq.max(1); k = np.argmax(same, 1)
    key = ((a[:, 2] * n[1] + a[:, 1]) * n[0] + a[:, 0]) * 3 + k
    assert np.all(np.diff(key) > 0)
    amb = _ambiguous_cells(t)
    assert amb.any()
    und, dire = _edges(tri)
    for (p, r), cnt in dire.items():
        if cnt > 1:
            assert amb[cell[p][2], cell[p][1], cell[p][0]] and amb[cell[r][2], cell[r][1], cell[r][0]]
    assert np.all(wgt >= 1) and np.all(wgt <= 255)


def test_the_restatement_is_vectorised():
    rng = np.random.default_rng(5)
    n = (65, 9, 9)
    V = M.make_volume(n, (0, 0, 0), rng.integers(-2000, 2000, n[::-1]), np.full(n[::-1], 1), VOXEL)
    t0 = time.perf_counter()
    xyz, _, _, tri = _whole(V)
    assert len(tri) > 1000 and time.perf_counter() - t0 < 1.0
