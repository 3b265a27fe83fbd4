"""GPU: the device mesher (vdo_mesh_*, csrc/mesh.hip) against the NumPy restatement of its contract (tests/mesh_ref.py).  Every comparison is
array_equal: the vertices with their float bits, the gradients, the weights and the triangle indices."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_ref as R
from tests import mesh_ref as M

pytestmark = pytest.mark.gpu

F = np.float32
VOXEL = 0.1
K4 = (50.0, 50.0, 0.0, 0.0)
SENT_F, SENT_I = F(-777.25), np.int32(-777)


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mesher(ctx):
    """one mesher for (nearly) every map of this module: 64^3 voxels, staging windows larger than any mesh here"""
    from vdo_slam_amd.mesh import Mesher
    m = Mesher(ctx, (64, 64, 64), stage_vertices=1 << 16, stage_triangles=1 << 17)
    yield m
    m.close()


@pytest.fixture(scope="module")
def small_windows(ctx):
    """staging windows of 7 vertices and 7 triangles: every host output of more goes through several"""
    from vdo_slam_amd.mesh import Mesher
    m = Mesher(ctx, (17, 5, 9), stage_vertices=7, stage_triangles=7)
    yield m
    m.close()


def device_map(ctx, V, voxel=VOXEL):
    """a device mapper holding the restatement's volume V (same origin, so the same slot alignment)"""
    from vdo_slam_amd.dense import DenseMapper
    m = DenseMapper(ctx, 1, 1, V.n, voxel, K4, origin=[int(v) for v in V.origin], stage_points=16)
    m.set_volume(V.words)
    return m


def whole(V):
    o = [int(v) for v in V.origin]
    return o, [o[a] + V.n[a] for a in range(3)]


def same(got, want, what):
    xyz, grad, wgt, tri, counts = got
    rx, rg, rw, rt = want
    assert counts == (len(rx), len(rt)), f"{what}: counts {counts} against {(len(rx), len(rt))}"
    assert np.array_equal(xyz.view(np.uint32), rx.view(np.uint32)), f"{what}: xyz bits"
    assert np.array_equal(grad, rg) and np.array_equal(wgt, rw), f"{what}: gradients or weights"
    assert np.array_equal(tri, rt), f"{what}: triangles"


def check(mesher, m, V, lo, hi, outside, min_weight, what):
    want = M.mesh(V, lo, hi, outside, min_weight)
    same(mesher.extract(m, lo, hi, outside, min_weight), want, what)
    return want


def random_volume(n, origin, seed, unseen=0.04, amp=3000):
    rng = np.random.default_rng(seed)
    t = rng.integers(-amp, amp + 1, n[::-1]); t[rng.random(n[::-1]) < 0.05] = 0
    w = rng.integers(1, 6, n[::-1]); w[rng.random(n[::-1]) < unseen] = 0
    return M.make_volume(n, origin, t, w, VOXEL)


SIZES = [(1, 1, 1), (2, 1, 1), (2, 2, 2), (3, 2, 2), (17, 5, 9), (65, 3, 3), (257, 2, 2)]


@pytest.mark.parametrize("n", SIZES, ids=lambda n: "x".join(map(str, n)))
def test_volume_sizes(ctx, mesher, small_windows, n):
    for origin in ((0, 0, 0), (-3 * n[0] - 2, 5, -(n[2] // 2) - 1)):
        V = random_volume(n, origin, 7 * n[0] + n[2], unseen=0.02 if n[0] * n[1] * n[2] > 12 else 0.0)
        m = device_map(ctx, V)
        lo, hi = whole(V)
        for mw in (2, 1):
            want = check(mesher, m, V, lo, hi, 0, mw, f"{n} at {origin}, min_weight {mw}")
            check(mesher, m, V, [0, 0, 0], [0, 0, 0], 1, mw, f"{n} at {origin}, outside an empty box, min_weight {mw}")
            if n[0] * n[1] * n[2] <= 17 * 5 * 9:
                check(small_windows, m, V, lo, hi, 0, mw, f"{n} at {origin}, windows of 7")
        if min(n) < 2:
            assert len(want[0]) == 0 and len(want[3]) == 0
        elif n == (17, 5, 9):
            assert len(want[0]) > 7 * 20 and len(want[3]) > 7 * 20                # cells across several ballot words, workgroups and windows
        else:
            assert len(want[0]) > 0
        m.close()


def test_recentred_origins(ctx, mesher):
    """the device clears what leaves; what stays keeps its slots, so the alignment is that of the new origin"""
    n = (17, 5, 9)
    V = random_volume(n, (0, 0, 0), 5, unseen=0.0)
    m = device_map(ctx, V)
    for q in ((3, 0, 0), (3, -2, 4), (-20, -9, -5), (-8, -7, -1), (-8 - 17, -7, -1)):
        m.recenter(q); V.recenter(q)
        words, origin = m.volume()
        assert tuple(origin) == q and np.array_equal(words, V.words)
        fresh = random_volume(n, q, 100 + abs(q[0]), unseen=0.0)                # fill what came in (zero words) with new content, keep the rest
        V.words = np.where(V.words == 0, fresh.words, V.words); m.set_volume(V.words)
        lo, hi = whole(V)
        want = check(mesher, m, V, lo, hi, 0, 1, f"after recentring to {q}")
        assert len(want[3]) > 100
        check(mesher, m, V, [lo[0] + 2, lo[1], lo[2] + 1], [hi[0] - 3, hi[1], hi[2] - 2], 1, 1, f"after recentring to {q}, outside a box")
    m.close()


def test_slot_alignment_does_not_matter(ctx, mesher):
    n = (17, 5, 9)
    rng = np.random.default_rng(21)
    t = rng.integers(-900, 900, n[::-1]); w = rng.integers(1, 4, n[::-1]); w[rng.random(n[::-1]) < 0.03] = 0
    meshes = []
    for origin in ((0, 0, 0), (17 * 3 + 5, -5 * 2 + 3, 9 * 4 + 8)):               # slots (0, 0, 0) and (5, 3, 8) for the same content
        V = M.make_volume(n, origin, t, w, VOXEL)
        m = device_map(ctx, V)
        lo, hi = whole(V)
        meshes.append(check(mesher, m, V, lo, hi, 0, 1, f"origin {origin}"))
        m.close()
    assert len(meshes[0][3]) > 50
    for k in (1, 2, 3):
        assert np.array_equal(meshes[0][k], meshes[1][k])                        # gradients, weights and triangles; the vertices differ by the shift


BOXES = [((0, 0, 0), (0, 0, 0)), ((100, 100, 100), (120, 120, 120)), ((-50, -50, -50), (-40, 60, 60)), ((-99, -99, -99), (99, 99, 99)), ((2, -9, 1), (99, 4, 8)),
         ((8, 0, 0), (9, 5, 9)), ((0, 2, 0), (17, 3, 9)), ((0, 0, 4), (17, 5, 5)), ((3, 1, 2), (12, 5, 7)), ((0, 0, 0), (17, 5, 9)), ((1, 1, 1), (16, 4, 8)), ((5, 0, 0), (7, 5, 9))]


def test_boxes_in_both_modes(ctx, mesher, small_windows):
    n, origin = (17, 5, 9), (-6, 40, -3)
    V = random_volume(n, origin, 33)
    m = device_map(ctx, V)
    lo, hi = whole(V)
    all_quads = M.sorted_rows(M.quads_of(*[M.mesh(V, lo, hi, 0, 1)[k] for k in (0, 3)]))
    for blo, bhi in BOXES:
        blo = [blo[a] + origin[a] for a in range(3)]; bhi = [bhi[a] + origin[a] for a in range(3)]
        parts = []
        for outside in (0, 1):
            got = mesher.extract(m, blo, bhi, outside, 1)
            same(got, M.mesh(V, blo, bhi, outside, 1), f"box {blo} .. {bhi}, outside {outside}")
            parts.append(M.quads_of(got[0], got[3]))
        assert np.array_equal(M.sorted_rows(np.concatenate(parts)), all_quads), f"box {blo} .. {bhi}: the two modes do not partition the quads"
    check(small_windows, m, V, [origin[0] + 3, origin[1] + 1, origin[2] + 2], [origin[0] + 12, origin[1] + 5, origin[2] + 7], 1, 1, "outside a box, windows of 7")
    m.close()


def raw(mesher, m, lo, hi, outside, mw, cv, ct, device=False):
    """vdo_mesh_extract into sentinel-filled buffers two rows longer than the capacities -> (xyz, grad, weight, tri, counts)"""
    xyz = np.full((cv + 2, 3), SENT_F, F); grad = np.full((cv + 2, 3), SENT_I, np.int32); wgt = np.full(cv + 2, SENT_I, np.int32); tri = np.full((ct + 2, 3), SENT_I, np.int32)
    if not device:
        counts = mesher.extract_raw(m, lo, hi, outside, mw, cv, xyz.ctypes.data, grad.ctypes.data, wgt.ctypes.data, ct, tri.ctypes.data, False)
        return xyz, grad, wgt, tri, counts
    import torch
    d = [torch.from_numpy(a).cuda() for a in (xyz, grad, wgt, tri)]
    torch.cuda.synchronize()
    counts = mesher.extract_raw(m, lo, hi, outside, mw, cv, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), ct, d[3].data_ptr(), True)
    return tuple(a.cpu().numpy() for a in d) + (counts,)


def check_raw(got, want, cv, ct, what):
    xyz, grad, wgt, tri, counts = got
    rx, rg, rw, rt = want
    assert counts == (len(rx), len(rt)), f"{what}: counts"
    v, t = min(cv, len(rx)), min(ct, len(rt))
    assert np.array_equal(xyz[:v].view(np.uint32), rx[:v].view(np.uint32)) and np.array_equal(grad[:v], rg[:v]) and np.array_equal(wgt[:v], rw[:v]), f"{what}: vertices"
    assert np.array_equal(tri[:t], rt[:t]), f"{what}: triangles"                 # indices of the FULL numbering, whatever the vertex capacity
    assert np.all(xyz[v:] == SENT_F) and np.all(grad[v:] == SENT_I) and np.all(wgt[v:] == SENT_I) and np.all(tri[t:] == SENT_I), f"{what}: written past min(capacity, count)"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_capacities(ctx, mesher, small_windows, device):
    n, origin = (17, 5, 9), (2, -3, 7)
    V = random_volume(n, origin, 44)
    m = device_map(ctx, V)
    lo, hi = whole(V)
    want = M.mesh(V, lo, hi, 0, 1)
    nv, nt = len(want[0]), len(want[3])
    assert nv > 20 and nt > 20
    for ms in (mesher, small_windows):
        for cv in (0, nv - 1, nv, nv + 1):
            for ct in (0, nt - 1, nt, nt + 1):
                check_raw(raw(ms, m, lo, hi, 0, 1, cv, ct, device), want, cv, ct, f"capacities {cv}, {ct} of {nv}, {nt}")
    m.close()


def _hand(ctx, mesher, n, t, w, mw=1, origin=(0, 0, 0)):
    V = M.make_volume(n, origin, np.asarray(t).reshape(n[::-1]), np.asarray(w).reshape(n[::-1]) if np.ndim(w) else np.full(n[::-1], w), VOXEL)
    m = device_map(ctx, V)
    lo, hi = whole(V)
    want = check(mesher, m, V, lo, hi, 0, mw, f"hand-made {n}")
    m.close()
    return want


def test_hand_made_zero_corners(ctx, mesher):
    """t = 0 is positive: with (-7, 0, -7) along x, frac is 1 in the first cell and 0 in the second - both vertices on the middle voxel's centre"""
    t = np.tile(np.array([-7, 0, -7]), (3, 3, 1))
    xyz, grad, wgt, tri = _hand(ctx, mesher, (3, 3, 3), t, 1)
    assert len(xyz) == 8 and np.all(xyz[:, 0] == F(1.5) * F(VOXEL))
    assert np.array_equal(grad[:, 0], np.tile([28, -28], 4)) and np.all(grad[:, 1:] == 0)
    assert len(tri) == 4                                                         # the two x edges through the middle of the volume, a quad each


def test_hand_made_checkerboard_and_ambiguous_faces(ctx, mesher):
    z, y, x = np.mgrid[0:4, 0:4, 0:4]
    t = np.where((x + y + z) % 2 == 0, 1, -1) * (100 + 37 * x + 11 * y + 5 * z)
    xyz, grad, wgt, tri = _hand(ctx, mesher, (4, 4, 4), t, 9)
    assert len(xyz) == 27 and len(tri) == 2 * 3 * 3 * 4                          # every cell active; every inner lattice edge (2 x 2 x 3 per axis) a quad
    t2 = np.full((3, 3, 3), 50); t2[0, 0, 0] = -50; t2[0, 1, 1] = -50; t2[1, 1, 1] = -30    # one ambiguous face in the z = 0 layer
    _hand(ctx, mesher, (3, 3, 3), t2, 2)


def test_hand_made_extremes(ctx, mesher):
    rng = np.random.default_rng(8)
    t = rng.choice([-32767, 32767], (5, 6, 7))
    xyz, grad, wgt, tri = _hand(ctx, mesher, (7, 6, 5), t, 255, mw=255, origin=((1 << 22) - 7, -(1 << 22) + 1, 0))
    assert len(tri) > 50 and np.all(wgt == 255) and 2 * 65534 <= np.abs(grad).max() <= 4 * 65534


def test_min_weight_gates_exactly_the_cells_of_the_corner(ctx, mesher):
    n = (6, 5, 6)
    t = M.sdf_words(n, lambda g: g @ np.array([0.3, 0.5, 0.81]) - 4.3)
    w = np.full(n[::-1], 3); corner = (2, 2, 3); w[corner[2], corner[1], corner[0]] = 1
    V = M.make_volume(n, (0, 0, 0), t, w, VOXEL)
    m = device_map(ctx, V)
    lo, hi = whole(V)
    info = {}
    full = M.mesh(V, lo, hi, 0, 1, info)
    same(mesher.extract(m, lo, hi, 0, 1), full, "min_weight 1")
    gated = mesher.extract(m, lo, hi, 0, 2)
    same(gated, M.mesh(V, lo, hi, 0, 2), "min_weight 2")
    # a cell loses validity iff the corner is one of its 8: the quads left are those of the full mesh with no such cell
    cell = info["cell"]
    touches = np.all((cell <= np.array(corner)) & (cell + 1 >= np.array(corner)), 1)
    q = full[3].reshape(-1, 2, 3); q4 = np.concatenate([q[:, 0, :], q[:, 1, 2:3]], 1)
    keep = ~touches[q4].any(1)
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(M.sorted_rows(M.quads_of(gated[0], gated[3])), M.sorted_rows(M.quads_of(full[0], full[3])[keep]))
    m.close()


def test_fused_sphere_and_plane(ctx, mesher):
    """depth rendered from a plane and a sphere in front of it, fused on the device through vdo_dense_integrate"""
    from tests import test_dense_ref as D
    from vdo_slam_amd.dense import DenseMapper
    m = DenseMapper(ctx, D.W, D.H, D.N, D.VOXEL, D.K4, origin=D.ORIGIN, trunc=D.TRUNC, min_depth=0.0, max_depth=10.0, max_weight=64, stage_points=16)
    depths, hits = [], []
    for T in D.POSES[:3]:
        d, hit = D.render(T, D.K4, D.W, D.H, D.PLANE_Z, D.SPHERE)
        depths.append(d); hits.append(hit)
        m.integrate(d.astype(F), None, T.astype(F))
    V = R.Volume(D.N, D.VOXEL, D.ORIGIN)
    V.words, _ = m.volume()
    lo, hi = whole(V)
    xyz, grad, wgt, tri = check(mesher, m, V, lo, hi, 0, 2, "fused sphere and plane")
    assert len(xyz) > 2000 and len(tri) > 4000
    # the surface is where it was rendered: a crossing lies within VOXEL + depth_term of a surface (tests/test_dense_ref.py), and a vertex is the
    # mean of its cell's crossings, so within the cell's diagonal of each of them
    assert D._distance(xyz, D.SPHERE).max() <= D.VOXEL + D.depth_term(depths, hits) + np.sqrt(3) * D.VOXEL
    check(mesher, m, V, [-10, -8, 30], [9, 12, 50], 1, 2, "fused, outside a box")
    m.close()


def test_an_object_volume(ctx, mesher):
    """a volume fused by the object stage (label-selecting) is a plain vdo_dense: the same mesher takes it"""
    from tests import test_dense_ref as D
    from vdo_slam_amd.dense import DenseMapper
    from vdo_slam_amd.objects import ObjectStage
    stage = ObjectStage(ctx, D.W, D.H, D.K4, min_depth=0.0, max_depth=10.0)
    n = (24, 24, 24)
    m = DenseMapper(ctx, D.W, D.H, n, D.VOXEL, D.K4, origin=(-12, -12, -12), trunc=D.TRUNC, min_depth=0.0, max_depth=10.0, max_weight=64, stage_points=16)
    Two = np.eye(4); Two[:3, 3] = D.SPHERE[0]                                     # the object frame sits on the sphere's centre
    depths, hits = [], []
    for T in D.POSES[:3]:
        d, hit = D.render(T, D.K4, D.W, D.H, D.PLANE_Z, D.SPHERE)
        depths.append(d); hits.append(hit)
        stage.integrate(d.astype(F), (hit * 5).astype(np.int32), [m], [5], [(T @ Two).astype(F)])
    V = R.Volume(n, D.VOXEL, (-12, -12, -12))
    V.words, _ = m.volume()
    lo, hi = whole(V)
    xyz, grad, wgt, tri = check(mesher, m, V, lo, hi, 0, 2, "object volume")
    assert len(tri) > 300
    bound = D.VOXEL + D.depth_term(depths, hits) + np.sqrt(3) * D.VOXEL            # as above, around the object frame's origin
    assert np.abs(np.linalg.norm(xyz.astype(np.float64), axis=1) - D.SPHERE[1]).max() <= bound
    m.close(); stage.close()


def test_one_mesher_serves_maps_of_different_sizes_in_turn(ctx, mesher):
    A = random_volume((33, 7, 5), (0, 0, 0), 1); B = random_volume((6, 4, 3), (9, 9, 9), 2)
    ma, mb = device_map(ctx, A), device_map(ctx, B)
    for V, m in ((A, ma), (B, mb), (A, ma), (B, mb)):
        lo, hi = whole(V)
        check(mesher, m, V, lo, hi, 0, 1, f"shared mesher, {V.n}")
    ma.close(); mb.close()


def test_refusals_write_nothing(ctx, mesher):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.mesh import Mesher, MeshParamsC
    V = random_volume((17, 5, 9), (0, 0, 0), 3)
    m = device_map(ctx, V)
    big = device_map(ctx, random_volume((65, 64, 64), (0, 0, 0), 4))             # one x slab more than the mesher's 64^3
    ctx2 = Context(0)
    other = device_map(ctx2, V)
    L = mesher._L
    L.vdo_last_error.restype = C.c_char_p
    lo = (C.c_int32 * 3)(0, 0, 0); hi = (C.c_int32 * 3)(17, 5, 9)
    cap = 4096
    xyz = np.full((cap, 3), SENT_F, F); grad = np.full((cap, 3), SENT_I, np.int32); wgt = np.full(cap, SENT_I, np.int32); tri = np.full((cap, 3), SENT_I, np.int32)
    counts = (C.c_int64 * 2)(-5, -6)
    good = dict(h=mesher._h, map=m._h, lo=lo, hi=hi, mw=1, cv=cap, xyz=xyz.ctypes.data, grad=grad.ctypes.data, weight=wgt.ctypes.data, ct=cap, tri=tri.ctypes.data, counts=counts)

    def call(**kw):
        a = dict(good, **kw)
        return L.vdo_mesh_extract(a["h"], a["map"], a["lo"], a["hi"], 0, a["mw"], a["cv"], C.c_void_p(a["xyz"]), C.c_void_p(a["grad"]), C.c_void_p(a["weight"]), a["ct"],
                                  C.c_void_p(a["tri"]), 0, a["counts"])
    cases = [(dict(h=None), "handle"), (dict(map=None), "map"), (dict(lo=None), "lo"), (dict(hi=None), "hi"), (dict(counts=None), "counts"), (dict(mw=0), "min_weight"),
             (dict(cv=-1), "vertex_capacity"), (dict(ct=-1), "triangle_capacity"), (dict(xyz=None), "xyz"), (dict(grad=None), "grad"), (dict(weight=None), "weight"),
             (dict(tri=None), "tri"), (dict(map=other._h), "context"), (dict(map=big._h), "larger")]
    for kw, name in cases:
        assert call(**kw) == K.VDO_ERR_INVALID, name
        assert name.encode() in L.vdo_last_error(), (name, L.vdo_last_error())
        assert np.all(xyz == SENT_F) and np.all(grad == SENT_I) and np.all(wgt == SENT_I) and np.all(tri == SENT_I) and tuple(counts) == (-5, -6), name
    assert call() == 0 and counts[0] > 0 and counts[1] > 0                       # and the same arguments, all good, are served
    # create
    h = C.c_void_p()
    for n, sv, st, code in (((0, 4, 4), 8, 8, -1), ((4, 4, 4), 0, 8, -1), ((4, 4, 4), 8, 0, -1), ((4097, 1, 1), 8, 8, -4), ((4096, 4096, 256), 8, 8, -4)):
        p = MeshParamsC((C.c_int32 * 3)(*n), sv, st)
        assert L.vdo_mesh_create(ctx._h, C.byref(p), C.byref(h)) == code and not h.value
    p = MeshParamsC((C.c_int32 * 3)(4, 4, 4), 8, 8)
    assert L.vdo_mesh_create(None, C.byref(p), C.byref(h)) == -1 and L.vdo_mesh_create(ctx._h, None, C.byref(h)) == -1 and L.vdo_mesh_create(ctx._h, C.byref(p), None) == -1
    assert L.vdo_mesh_last_timing(None, (C.c_double * 2)()) == -1
    m.close(); big.close(); other.close(); ctx2.close()


def test_timing_is_reported(ctx, mesher):
    V = random_volume((17, 5, 9), (0, 0, 0), 3)
    m = device_map(ctx, V)
    lo, hi = whole(V)
    mesher.extract(m, lo, hi)
    wall, dev = mesher.timing()
    assert wall > 0 and dev > 0 and dev <= wall * 1.5
    m.close()
