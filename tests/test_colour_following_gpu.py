"""GPU: the coloured mesh of a volume that follows the camera (vdo_slam_amd/colour.py, FollowingColourMesh) over a path that moves the volume on
every axis.  What is kept before a move is coloured BEFORE the move, while its voxels are still in the volume; vertices, triangles and colours
equal the same flow on the restatements (tests/dense_ref.py, tests/mesh_ref.py, tests/colour_ref.py) bit for bit."""
import math

import numpy as np
import pytest

from tests import colour_ref as CR
from tests import dense_ref as R
from tests import mesh_ref as M

pytestmark = pytest.mark.gpu

F = np.float32
W, H, N, VOXEL, K4 = 48, 32, (24, 16, 20), 0.1, (40.0, 40.0, 23.5, 15.5)
ANCHOR, MARGIN, MIN_WEIGHT, MAX_DEPTH = (0.5, 0.5, 0.25), 2, 1, 10.0
TRUNC = F(4.0 * float(F(VOXEL)))
BAND = float(TRUNC / F(2))


def _frames():
    """A noisy wall 1 m ahead of a camera that walks along +x (moves of the volume towards +x), then towards -y, then forward (+z); the wall keeps
    its distance.  The image is a ramp over the pixels that changes from frame to frame."""
    rng = np.random.default_rng(0)
    poses, depths, images = [], [], []
    ys, xs = np.mgrid[0:H, 0:W]
    for k in range(11):
        T = np.eye(4, dtype=F)
        T[0, 3] = -0.35 * min(k, 4); T[1, 3] = 0.3 * min(max(k - 4, 0), 3); T[2, 3] = -0.35 * max(k - 7, 0)      # world -> camera: the centre is at -t
        poses.append(T)
        depths.append((1.0 + 0.002 * (xs - W / 2) + rng.normal(0, 0.01, (H, W))).astype(F))
        images.append(np.stack([5 * xs + k, 7 * ys + 2 * k, 250 - 4 * xs - 3 * k], -1).astype(np.uint8))
    return poses, depths, images


@pytest.fixture(scope="module")
def flow():
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.colour import FollowingColourMesh
    ctx = Context(0)
    poses, depths, images = _frames()
    fm = FollowingColourMesh(ctx, W, H, N, VOXEL, K4, anchor=ANCHOR, margin=MARGIN, min_weight=MIN_WEIGHT, max_depth=MAX_DEPTH)
    try:
        origins = []
        for T, d, im in zip(poses, depths, images):
            fm.fuse(d, None, im, T)
            origins.append(fm.mapper.origin())
        mesh = fm.coloured_mesh()
        points = fm.coloured_points()
        kept = np.concatenate(fm.m_xyz) if fm.m_xyz else np.zeros((0, 3), F)
        after = fm.colourer.sample(kept, 1)[0]                  # the kept vertices sampled in the LAST volume: most of their voxels are gone
        out = dict(mesh=mesh, points=points, origins=origins, recenters=fm.recenters, kept=len(kept), after=after, poses=poses, depths=depths, images=images)
    finally:
        fm.close(); ctx.close()
    return out


@pytest.fixture(scope="module")
def restated(flow):
    return _restate(flow["poses"], flow["depths"], flow["images"])


def _restate(poses, depths, images):
    """the same flow on the restatements"""
    from vdo_slam_amd.dense import leaving_boxes
    from vdo_slam_amd.mesh import staying_box

    def camera_voxel(T, voxel):                                 # the voxel of the camera centre -R^T t, in float64 (as host/DenseMapper.cc states it)
        T = np.asarray(T, F).reshape(4, 4).astype(np.float64)
        return [int(math.floor(-(T[0, a] * T[0, 3] + T[1, a] * T[1, 3] + T[2, a] * T[2, 3]) / float(F(voxel)))) for a in range(3)]
    V = R.Volume(N, VOXEL, (0, 0, 0)); Cv = CR.ColourVolume(N, VOXEL, (0, 0, 0))
    target = [int(np.floor(ANCHOR[a] * N[a])) for a in range(3)]
    started, base = False, 0
    mx, mg, mw, mt, mc, px, pg, pw, pc = [], [], [], [], [], [], [], [], []
    for T, d, im in zip(poses, depths, images):
        c = camera_voxel(T, VOXEL)
        o = [int(v) for v in V.origin]
        want = [c[a] - target[a] for a in range(3)]
        if not started or any(abs(c[a] - (o[a] + target[a])) > MARGIN for a in range(3)):
            if started:
                assert tuple(Cv.origin) == tuple(V.origin)      # the colour volume stands where the map stands: it followed at the last frame
                lo, hi = staying_box(o, want, N)
                x, g, w, t = M.mesh(V, lo, hi, 1, MIN_WEIGHT)
                mx.append(x); mg.append(g); mw.append(w); mt.append(t + np.int32(base)); mc.append(Cv.sample(x, 1)); base += len(x)
                for blo, bhi in leaving_boxes(o, want, N):
                    x, g, w = V.extract(blo, bhi, MIN_WEIGHT)
                    px.append(x); pg.append(g); pw.append(w); pc.append(Cv.sample(x, 1))
            V.recenter(want); started = True
        V.integrate(d, None, T, K4, TRUNC, 0.0, MAX_DEPTH, 64)
        Cv.integrate(d, None, im, T, K4, 0.0, MAX_DEPTH, BAND, 64, 0, 0, map_origin=V.origin)
    x, g, w, t = M.mesh_all(V, MIN_WEIGHT)
    o = [int(v) for v in V.origin]
    ex, eg, ew = V.extract(o, [o[a] + N[a] for a in range(3)], MIN_WEIGHT)
    return dict(X=np.concatenate(mx + [x]), G=np.concatenate(mg + [g]), Wt=np.concatenate(mw + [w]), T=np.concatenate(mt + [t + np.int32(base)]),
                C=np.concatenate(mc + [Cv.sample(x, 1)]), kept=base, after=Cv.sample(np.concatenate(mx), 1), PX=np.concatenate(px + [ex]), PC=np.concatenate(pc + [Cv.sample(ex, 1)]))


def test_the_volume_moved_on_every_axis(flow):
    o = flow["origins"]
    moves = [(a, b) for a, b in zip(o, o[1:]) if a != b]
    assert flow["recenters"] == len(moves) >= 3
    assert any(b[0] > a[0] for a, b in moves) and any(b[1] < a[1] for a, b in moves) and any(b[2] > a[2] for a, b in moves)


def test_vertices_triangles_and_colours_equal_the_restatement(flow, restated):
    X, Nn, Wt, T, C = flow["mesh"]
    assert len(T) > 300 and flow["kept"] == restated["kept"] > 100
    assert np.array_equal(X.view(np.uint32), restated["X"].view(np.uint32)) and np.array_equal(T, restated["T"])
    assert np.array_equal(Nn.view(np.uint32), R.normals(restated["G"]).view(np.uint32)) and np.array_equal(Wt, restated["Wt"])
    assert C.shape == (len(X), 4) and np.array_equal(C, restated["C"])
    PX, _, _, PC = flow["points"]
    assert np.array_equal(PX.view(np.uint32), restated["PX"].view(np.uint32)) and np.array_equal(PC, restated["PC"])


def test_what_left_kept_its_colour(flow, restated):
    """Every kept vertex that had a coloured neighbourhood before its move has alpha > 0 - and would have lost it had it been sampled after."""
    C = flow["mesh"][4][:flow["kept"]]
    before = restated["C"][:restated["kept"]]
    assert np.array_equal(C[:, 3] > 0, before[:, 3] > 0) and (C[:, 3] > 0).mean() > 0.9
    assert np.array_equal(flow["after"], restated["after"])
    gone = (C[:, 3] > 0) & (flow["after"][:, 3] == 0)
    print(f"{flow['kept']} kept vertices, {(C[:, 3] > 0).sum()} coloured, {gone.sum()} of them have no colour in the last volume")
    assert gone.sum() > 50


def test_a_coloured_mesh_reads_back_and_an_uncoloured_one_keeps_its_bytes(flow, tmp_path):
    from vdo_slam_amd import colour as CL, mesh as MS
    X, Nn, Wt, T, C = flow["mesh"]
    CL.write_ply(tmp_path / "c.ply", X, Nn, Wt, T, C)
    x, n, w, t, c = CL.read_ply(tmp_path / "c.ply")
    assert np.array_equal(x.view(np.uint32), X.view(np.uint32)) and np.array_equal(n.view(np.uint32), Nn.view(np.uint32)) and np.array_equal(w, Wt)
    assert np.array_equal(t, T) and np.array_equal(c, C)
    head = open(tmp_path / "c.ply", "rb").read(600)
    assert b"property int weight\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face" in head
    CL.write_ply(tmp_path / "plain.ply", X, Nn, Wt, T); MS.write_ply(tmp_path / "mesh.ply", X, Nn, Wt, T)
    assert open(tmp_path / "plain.ply", "rb").read() == open(tmp_path / "mesh.ply", "rb").read()
    assert CL.read_ply(tmp_path / "plain.ply")[4] is None and np.array_equal(CL.read_ply(tmp_path / "plain.ply")[3], T)
