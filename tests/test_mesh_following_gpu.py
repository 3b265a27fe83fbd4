"""GPU: the mesh of a volume that follows the camera (vdo_slam_amd/mesh.py, FollowingMesh).  Before every move the quads that will not be wholly
inside the staying box are kept (`outside` mode); the kept pieces and the last volume must hold every quad of the scene exactly once - checked
against the restatement of the same flow (bit for bit) and against a twin volume that never moves."""
import numpy as np
import pytest

from tests import dense_ref as R
from tests import mesh_ref as M

pytestmark = pytest.mark.gpu

F = np.float32
W, H, N, VOXEL, K4 = 48, 32, (24, 16, 20), 0.1, (40.0, 40.0, 23.5, 15.5)
ANCHOR, MARGIN, MIN_WEIGHT, MAX_DEPTH = (0.5, 0.5, 0.25), 2, 1, 10.0


def _frames():
    """A noisy, slightly tilted wall 1 m ahead, seen by a camera that walks along +x (four moves of the volume), then towards -y (two moves towards a
    negative axis).  The view (+-0.6 m by +-0.4 m on the wall, the camera within MARGIN voxels of the volume's middle) never reaches the volume's
    outer 2 voxels in x and y: a voxel at a seam is not fused again after the call that kept its quads, and the twin sees nothing outside the
    moving volume."""
    rng = np.random.default_rng(0)
    poses, depths = [], []
    ys, xs = np.mgrid[0:H, 0:W]
    for k in range(8):
        T = np.eye(4, dtype=F)
        T[0, 3] = -0.35 * min(k, 4); T[1, 3] = 0.3 * max(k - 5, 0)               # world -> camera: the camera centre is at -t
        poses.append(T)
        depths.append((1.0 + 0.002 * (xs - W / 2) + rng.normal(0, 0.01, (H, W))).astype(F))
    return poses, depths


@pytest.fixture(scope="module")
def flow():
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.dense import DenseMapper
    from vdo_slam_amd.mesh import FollowingMesh, Mesher
    ctx = Context(0)
    poses, depths = _frames()
    fm = FollowingMesh(ctx, W, H, N, VOXEL, K4, anchor=ANCHOR, margin=MARGIN, min_weight=MIN_WEIGHT, max_depth=MAX_DEPTH)
    origins = []
    for T, d in zip(poses, depths):
        fm.fuse(d, None, T)
        origins.append(fm.mapper.origin())
    got = fm.mesh()
    # the twin: one volume over every place the moving one has been, never moved
    lo = [min(o[a] for o in origins) for a in range(3)]; hi = [max(o[a] for o in origins) + N[a] for a in range(3)]
    n2 = [hi[a] - lo[a] for a in range(3)]
    twin = DenseMapper(ctx, W, H, n2, VOXEL, K4, origin=lo, max_depth=MAX_DEPTH)
    for T, d in zip(poses, depths):
        twin.integrate(d, None, T)
    ms = Mesher(ctx, n2)
    tw = ms.extract_all(twin, MIN_WEIGHT)
    out = dict(got=got, origins=origins, recenters=fm.recenters, twin=tw, pieces=len(fm.m_tri), poses=poses, depths=depths)
    ms.close(); twin.close(); fm.close(); ctx.close()
    return out


def test_the_volume_moved_towards_both_signs(flow):
    o = flow["origins"]
    assert flow["recenters"] >= 3 and flow["pieces"] == flow["recenters"]
    assert any(b[0] > a[0] for a, b in zip(o, o[1:])) and any(b[1] < a[1] for a, b in zip(o, o[1:]))


def test_no_quad_is_lost_or_doubled_at_a_seam(flow):
    X, Nn, Wt, T = flow["got"]
    xyz, grad, wgt, tri, counts = flow["twin"]
    assert len(T) > 300 and T.min() >= 0 and T.max() < len(X)
    mine = M.sorted_rows(M.quads_of(X, T)); twin = M.sorted_rows(M.quads_of(xyz, tri))
    assert len(mine) == len(twin) and np.array_equal(mine, twin)


def test_the_flow_equals_its_restatement(flow):
    """the same flow on the restatement's volume: the pieces, their order and the rebased indices, bit for bit"""
    import math

    def camera_voxel(T, voxel):                                 # the voxel of the camera centre -R^T t, in float64 (as host/DenseMapper.cc states it)
        T = np.asarray(T, F).reshape(4, 4).astype(np.float64)
        return [int(math.floor(-(T[0, a] * T[0, 3] + T[1, a] * T[1, 3] + T[2, a] * T[2, 3]) / float(F(voxel)))) for a in range(3)]

    def staying_box(o, q, n):                                   # what both the old and the new volume cover; empty: all zeros
        lo = [max(o[a], q[a]) for a in range(3)]; hi = [min(o[a], q[a]) + n[a] for a in range(3)]
        return ([0, 0, 0], [0, 0, 0]) if any(hi[a] <= lo[a] for a in range(3)) else (lo, hi)
    V = R.Volume(N, VOXEL, (0, 0, 0))
    target = [int(np.floor(ANCHOR[a] * N[a])) for a in range(3)]
    started, base, px, pg, pw, pt = False, 0, [], [], [], []
    for T, d in zip(flow["poses"], flow["depths"]):
        c = camera_voxel(T, VOXEL)
        o = [int(v) for v in V.origin]
        want = [c[a] - target[a] for a in range(3)]
        if not started or any(abs(c[a] - (o[a] + target[a])) > MARGIN for a in range(3)):
            if started:
                lo, hi = staying_box(o, want, N)
                x, g, w, t = M.mesh(V, lo, hi, 1, MIN_WEIGHT)
                px.append(x); pg.append(g); pw.append(w); pt.append(t + np.int32(base)); base += len(x)
            V.recenter(want); started = True
        V.integrate(d, None, T, K4, F(4.0 * float(F(VOXEL))), 0.0, MAX_DEPTH, 64)
    x, g, w, t = M.mesh_all(V, MIN_WEIGHT)
    X, Nn, Wt, T = flow["got"]
    assert np.array_equal(X.view(np.uint32), np.concatenate(px + [x]).view(np.uint32))
    assert np.array_equal(Nn.view(np.uint32), R.normals(np.concatenate(pg + [g])).view(np.uint32)) and np.array_equal(Wt, np.concatenate(pw + [w]))
    assert np.array_equal(T, np.concatenate(pt + [t + np.int32(base)]))


def test_a_saved_mesh_reads_back(flow, tmp_path):
    from vdo_slam_amd.mesh import read_ply, write_ply
    X, Nn, Wt, T = flow["got"]
    write_ply(tmp_path / "mesh.ply", X, Nn, Wt, T)
    x, n, w, t = read_ply(tmp_path / "mesh.ply")
    assert np.array_equal(x.view(np.uint32), X.view(np.uint32)) and np.array_equal(n.view(np.uint32), Nn.view(np.uint32)) and np.array_equal(w, Wt) and np.array_equal(t, T)
    head = open(tmp_path / "mesh.ply", "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
