"""GPU: the device raycaster (vdo_raycast_*, csrc/raycast.hip) against the NumPy restatement of its contract (tests/raycast_ref.py).  Every comparison
is array_equal: depth and gradient as uint32 views, weights and counts, with the empty-space skipping on and off."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_ref as R
from tests import raycast_ref as RC

pytestmark = pytest.mark.gpu

F = np.float32
VOXEL = 0.1


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _mapper(ctx, n, origin, W=8, H=8, K4=(8.0, 8.0, 3.5, 3.5), **prm):
    from vdo_slam_amd.dense import DenseMapper
    return DenseMapper(ctx, W, H, n, VOXEL, K4, origin=origin, stage_points=4096, **prm)


def _same(got, want, what):
    assert tuple(got[3]) == tuple(want[3]), f"{what}: counts {tuple(got[3])} against {tuple(want[3])}"
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: {int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum())} depth bits differ"
    assert np.array_equal(got[2], want[2]), f"{what}: weights"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), f"{what}: gradient bits"


def _check(m, V, W, H, K4, near, step, n_steps, min_weight, T, what):
    """A view of the mapper m against the restatement on V, skipping on and off; returns the restatement's render"""
    from vdo_slam_amd.raycast import Raycaster
    want = RC.render(V, W, H, K4, near, step, n_steps, min_weight, T)
    assert sum(want[3]) == W * H
    rc = Raycaster(m, W, H, K4, near, step, n_steps, min_weight)
    for skip in (True, False):
        rc.set_skip(skip)
        _same(rc.render(T), want, f"{what}, skipping {'on' if skip else 'off'}")
    rc.close()
    return want


def _dense_words(n, seed, p_light=0.05):
    """Random well-formed words: crossings everywhere, weights 1 (a few) .. 5 straddling min_weight 2"""
    rng = np.random.default_rng(seed)
    shape = tuple(n)[::-1]
    t = rng.integers(-32767, 32768, shape)
    w = np.where(rng.random(shape) < p_light, 1, rng.integers(2, 6, shape))
    return ((w << 16) | (t & 0xFFFF)).astype(np.uint32)


def _sparse_words(n, seed):
    """Mostly zero: small blocks of seen voxels and lone voxels on brick faces, brick corners and the cyclic seam (slots 7 | 8, n - 1 | 0)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    words = np.zeros((nz, ny, nx), np.uint32)

    def put(x, y, z, size):
        for k in range(size):
            for j in range(size):
                for i in range(size):
                    t = int(rng.integers(-32767, 32768)); w = int(rng.integers(2, 6))
                    words[(z + k) % nz, (y + j) % ny, (x + i) % nx] = (w << 16) | (t & 0xFFFF)
    marks = [(7, 7, 7), (8, 8, 8), (nx - 1, 3, 5), (3, ny - 1, 5), (3, 5, nz - 1), (nx - 1, ny - 1, nz - 1), (0, 0, 0), (15, 7, 23), (16, 8, 24), (nx // 2, ny // 2, nz // 2)]
    for x, y, z in marks:
        put(x % nx, y % ny, z % nz, int(rng.integers(2, 5)))
    for x, y, z in [(7, 0, 0), (8, 0, 0), (0, 7, 8), (nx - 1, 0, 8), (0, ny - 1, 7), (8, 8, nz - 1), (nx // 3, ny // 3, nz // 3)]:
        put(x % nx, y % ny, z % nz, 1)
    return words


FRONT = 0.8


def _view(n, origin, W, yaw=0.03, shift=(0.013, -0.007, 0.0), f_scale=1.3):
    """A camera 0.8 m in front of the volume's front face looking along +z (turned by yaw), whose image the face overfills; the march covers the volume"""
    n = np.array(n); o = np.array(origin)
    centre = (o + 0.5 * n) * VOXEL
    dist = FRONT + 0.5 * n[2] * VOXEL
    c, s = np.cos(yaw), np.sin(yaw)
    Rm = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    T = np.eye(4)
    T[:3, :3] = Rm
    T[:3, 3] = -Rm @ centre + np.array(shift) + [0, 0, dist]
    f = f_scale * max(W, 16) * FRONT / max(n[0] * VOXEL, 0.3)
    return T.astype(F), f


def _setup(ctx, n, o, W, H, words, **view):
    T, f = _view(n, o, W, **view)
    K4 = (f, 0.9 * f, 0.5 * W - 0.25, 0.5 * H + 0.1)
    m = _mapper(ctx, n, o)
    V = R.Volume(n, VOXEL, o)
    V.words = words
    m.set_volume(words)
    near, step = 0.5, 0.07
    n_steps = int(np.ceil((FRONT + n[2] * VOXEL + 0.3 - near) / step)) + 1
    return m, V, T, K4, near, step, n_steps


# ---- sizes --------------------------------------------------------------------------------------------------------------------------------
VOLUMES = [(1, 1, 1), (2, 1, 2), (2, 2, 2)] + [(x, y, z) for x in (7, 8, 9) for y in (3, 4, 5) for z in (15, 16, 17)] + [(65, 2, 3), (64, 32, 64)]
BIG = ((1, 1, 1), (2, 1, 2), (2, 2, 2), (65, 2, 3), (64, 32, 64))
ORIGINS = {"negative": lambda n: tuple(-3 * v - 2 for v in n), "zero": lambda n: (0, 0, 0), "straddling": lambda n: tuple(-(v // 2) - (v > 1) for v in n)}


@pytest.mark.parametrize("n", VOLUMES, ids=lambda n: "x".join(map(str, n)))
def test_volume_sizes_and_origins(ctx, n):
    images = [(1, 1), (96, 48)] if n in BIG else [(32, 8)]
    for W, H in images:
        for name, fo in ORIGINS.items():
            o = fo(n)
            m, V, T, K4, near, step, n_steps = _setup(ctx, n, o, W, H, _dense_words(n, 31 * W + n[0] + n[2]))
            want = _check(m, V, W, H, K4, near, step, n_steps, 2, T, f"{n} at {o} ({name}), image {W}x{H}")
            if min(n) == 1:
                assert want[3] == (0, 0, W * H)                                # a one-voxel axis has no base cell: no sample can be valid
            if n == (64, 32, 64) and (W, H) == (96, 48):
                assert min(want[3][:2]) > 200 and (np.abs(want[1]).sum(-1) > 0).sum() > 200      # hits, misses and gradients all occur
            m.close()


@pytest.mark.parametrize("W,H", [(w, h) for w in (31, 32, 33) for h in (7, 8, 9)])
def test_image_sizes(ctx, W, H):
    n, o = (9, 5, 17), (-4, -2, 3)
    m, V, T, K4, near, step, n_steps = _setup(ctx, n, o, W, H, _dense_words(n, 100 * W + H))
    want = _check(m, V, W, H, K4, near, step, n_steps, 2, T, f"image {W}x{H}")
    assert want[3][0] > 0
    m.close()


@pytest.mark.parametrize("n,o", [((64, 32, 64), (-32, -16, 5)), ((64, 32, 64), (-37, -11, 3)), ((17, 9, 16), (-8, -4, 0)), ((23, 16, 40), (5, -21, -9))], ids=str)
def test_sparse_volumes_with_voxels_on_brick_faces_corners_and_the_seam(ctx, n, o):
    W, H = 96, 48
    words = _sparse_words(n, n[0] + o[0])
    m, V, T, K4, near, step, n_steps = _setup(ctx, n, o, W, H, words)
    want = _check(m, V, W, H, K4, near, step, n_steps, 2, T, f"sparse {n} at {o}")
    assert want[3][0] + want[3][1] > 0 and want[3][2] > 0
    # straight down each axis through the seam, from outside
    for yaw in (0.5, -0.9):
        T2, _ = _view(n, o, W, yaw=yaw)
        _check(m, V, W, H, K4, near, step, n_steps, 2, T2, f"sparse {n} at {o}, yaw {yaw}")
    m.close()


# ---- volumes made by integrating planes, recentring ------------------------------------------------------------------------------------------------
PW, PH, PK4 = 48, 32, (40.0, 40.0, 23.5, 15.5)
PN, PO = (64, 48, 40), (-32, -24, 30)
NEAR, STEP, STEPS = 3.0, 0.2, 25


def _plane_depth(normal, d):
    ys, xs = np.mgrid[0:PH, 0:PW]
    r = np.stack([(xs - PK4[2]) / PK4[0], (ys - PK4[3]) / PK4[1], np.ones((PH, PW))], -1)
    return (d / (r @ np.asarray(normal))).astype(F)


def _yaw(deg, shift):
    T = np.eye(4)
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = shift
    return T.astype(F)


def _fused_plane(ctx, normal):
    m = _mapper(ctx, PN, PO, PW, PH, PK4, trunc=0.4, max_depth=10.0)
    V = R.Volume(PN, VOXEL, PO)
    depth = _plane_depth(normal, 5.0)
    I4 = np.eye(4, dtype=F)
    for _ in range(4):
        assert m.integrate(depth, None, I4) == V.integrate(depth, None, I4, PK4, 0.4, 0.0, 10.0, 64)
    assert np.array_equal(m.volume()[0], V.words)
    return m, V


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (-0.2, 0.0, 1.0)], ids=["fronto", "tilted"])
def test_integrated_planes_and_recentring(ctx, normal):
    m, V = _fused_plane(ctx, normal)
    views = [np.eye(4, dtype=F), _yaw(10.0, (0.3, 0.0, 0.0)), _yaw(-25.0, (-1.0, 0.2, 0.5))]
    for i, T in enumerate(views):
        want = _check(m, V, PW, PH, PK4, NEAR, STEP, STEPS, 2, T, f"plane {normal}, view {i}")
        if i < 2:
            assert want[3][0] > 1000 and (np.abs(want[1]).sum(-1) > 0).sum() > 900
    # the seam inside the view on each axis, then on all three
    for q in [(-32 + 29, -24, 30), (-32, -24 - 20, 30), (-32, -24, 30 + 17), (-32 - 9, -24 + 11, 30 + 13)]:
        m.recenter(PO); V.recenter(PO)
        depth = _plane_depth(normal, 5.0)
        m2, V2 = m, V
        V2.words = np.zeros_like(V2.words); m2.set_volume(V2.words)
        for _ in range(2):
            assert m2.integrate(depth, None, np.eye(4, dtype=F)) == V2.integrate(depth, None, np.eye(4, dtype=F), PK4, 0.4, 0.0, 10.0, 64)
        m2.recenter(q); V2.recenter(q)
        assert np.array_equal(m2.volume()[0], V2.words)
        for i, T in enumerate(views[:2]):
            want = _check(m2, V2, PW, PH, PK4, NEAR, STEP, STEPS, 2, T, f"plane {normal}, recentred to {q}, view {i}")
            assert want[3][0] > 150
    m.close()


# ---- parameters -------------------------------------------------------------------------------------------------------------------------------
def test_parameters(ctx):
    n, o, W, H = (16, 9, 17), (-8, -4, 2), 33, 9
    m, V, T, K4, near, step, n_steps = _setup(ctx, n, o, W, H, _dense_words(n, 3, p_light=0.02))
    assert _check(m, V, W, H, K4, near, step, 1, 2, T, "n_steps 1")[3][0] == 0                      # one sample: no pair, no hit
    _check(m, V, W, H, K4, 0.9, 0.05, 2, 2, T, "n_steps 2")
    assert _check(m, V, W, H, K4, 0.0, 0.01, 300, 2, T, "n_steps 300, near 0")[3][0] > 0
    assert _check(m, V, W, H, K4, 0.0, 0.01, 300, 1, T, "min_weight 1")[3][0] > 0
    assert _check(m, V, W, H, K4, near, step, n_steps, 255, T, "min_weight 255")[3] == (0, 0, W * H)
    _check(m, V, W, H, K4, 0.0, 7.5, 5, 1, T, "a step larger than the volume")
    _check(m, V, W, H, K4, 1.0, 1.0e30, 4, 1, T, "a step that overflows")
    V.words = (V.words & np.uint32(0xFFFF)) | np.uint32(255 << 16); m.set_volume(V.words)
    assert _check(m, V, W, H, K4, near, step, n_steps, 255, T, "min_weight 255 on full weights")[3][0] > 0
    m.close()


# ---- poses and intrinsics ------------------------------------------------------------------------------------------------------------------------
def test_poses_and_intrinsics(ctx):
    n, o, W, H = (24, 16, 20), (-12, -8, 4), 33, 9
    m, V, T, K4, near, step, n_steps = _setup(ctx, n, o, W, H, _dense_words(n, 9, p_light=0.01))
    centre = (np.array(o) + 0.5 * np.array(n)) * VOXEL
    I4 = np.eye(4, dtype=F)
    inside = I4.copy(); inside[:3, 3] = -centre
    behind = I4.copy(); behind[:3, 3] = -centre - [0, 0, 3.0]                  # the volume lies behind the camera
    far = I4.copy(); far[:3, 3] = -centre + [0, 0, 500.0]
    up = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F); up[:3, 3] = -(up[:3, :3] @ centre) + [0, 0, 1.5]
    for name, pose in [("identity", I4), ("front", T), ("turned", _view(n, o, W, yaw=0.6)[0]), ("inside", inside), ("behind", behind), ("far", far), ("about x", up)]:
        want = _check(m, V, W, H, K4, 0.0, 0.05, 80, 2, pose, name)
        if name in ("front", "inside", "about x"):
            assert want[3][0] > 0, name
        if name in ("behind", "far"):
            assert want[3] == (0, 0, W * H), name
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 3, 5, 10, 11):
            Tb = T.copy(); Tb.reshape(16)[at] = bad
            want = _check(m, V, W, H, K4, near, step, n_steps, 2, Tb, f"T[{at}] = {bad}")
            if at in (3, 11):                                                 # the centre is not finite: nothing can be valid
                assert want[3] == (0, 0, W * H) and not want[0].any() and not want[1].any() and not want[2].any()
    allnan = np.full((4, 4), np.nan, F)
    assert _check(m, V, W, H, K4, near, step, n_steps, 2, allnan, "T all NaN")[3] == (0, 0, W * H)
    for fx, fy in [(1e30, 1e30), (1e-30, 1e-30), (1e-3, 5e4), (3.0e38, 2.0e-38)]:
        _check(m, V, W, H, (fx, fy, K4[2], K4[3]), near, step, n_steps, 2, T, f"fx {fx}, fy {fy}")
    _check(m, V, W, H, (K4[0], K4[1], -1e6, 1e6), near, step, n_steps, 2, T, "principal point far outside")
    m.close()


# ---- outputs -----------------------------------------------------------------------------------------------------------------------------------
def test_host_and_device_outputs_each_null_in_turn(ctx):
    import torch
    from vdo_slam_amd.raycast import Raycaster
    n, o, W, H = (16, 9, 17), (-8, -4, 2), 33, 9
    m, V, T, K4, near, step, n_steps = _setup(ctx, n, o, W, H, _dense_words(n, 4, p_light=0.02))
    want = RC.render(V, W, H, K4, near, step, n_steps, 2, T)
    assert want[3][0] > 0
    rc = Raycaster(m, W, H, K4, near, step, n_steps, 2)
    for skip in (True, False):
        rc.set_skip(skip)
        for drop in (None, 0, 1, 2, (0, 1, 2)):
            drop = (drop,) if isinstance(drop, int) else (drop or ())
            host = [np.full((H, W), -7.0, F), np.full((H, W, 3), -7.0, F), np.full((H, W), -7, np.int32)]
            dev = [torch.from_numpy(a.copy()).cuda() for a in host]
            torch.cuda.synchronize()
            got = rc.render_raw(T, *[None if k in drop else host[k].ctypes.data for k in range(3)], False)
            assert tuple(got) == want[3]
            got = rc.render_device(T, *[None if k in drop else dev[k].data_ptr() for k in range(3)])
            assert tuple(got) == want[3]
            for k in range(3):
                back = dev[k].cpu().numpy()
                for arr, where in ((host[k], "host"), (back, "device")):
                    if k in drop:
                        assert (arr == -7).all(), f"output {k} ({where}) was written though NULL"
                    else:
                        assert np.array_equal(arr.view(np.uint32), want[k].view(np.uint32)), f"output {k} ({where}), dropped {drop}, skipping {skip}"
    wall, dev_ms, grid_ms = rc.timing()
    assert wall > 0 and dev_ms >= 0 and grid_ms == 0                          # the last render ran with skipping off
    rc.close(); m.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(ctx):
    from vdo_slam_amd import raycast as RY
    L = RY._lib()
    L.vdo_last_error.restype = C.c_char_p
    m = _mapper(ctx, (4, 4, 4), (0, 0, 0))
    h = C.c_void_p()

    def create(W=8, H=8, mapper=m._h, **kw):
        prm = dict(K4=(4.0, 4.0, 4.0, 4.0), near=0.5, step=0.1, n_steps=10, min_weight=2)
        prm.update(kw)
        pc = RY.params(**prm)
        return L.vdo_raycast_create(mapper, W, H, C.byref(pc), C.byref(h)), L.vdo_last_error().decode()

    nan, inf = float("nan"), float("inf")
    for kw, word in [(dict(W=0), "width"), (dict(H=0), "height"), (dict(W=-3), "width"), (dict(K4=(0.0, 4.0, 4.0, 4.0)), "fx"), (dict(K4=(4.0, -1.0, 4.0, 4.0)), "fy"),
                     (dict(K4=(4.0, 4.0, nan, 4.0)), "K[2]"), (dict(K4=(inf, 4.0, 4.0, 4.0)), "K[0]"), (dict(K4=(4.0, 4.0, 4.0, -inf)), "K[3]"), (dict(near=-0.1), "near"),
                     (dict(near=nan), "near"), (dict(near=inf), "near"), (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=nan), "step"), (dict(step=inf), "step"),
                     (dict(n_steps=0), "n_steps"), (dict(n_steps=65537), "n_steps"), (dict(min_weight=0), "min_weight"), (dict(min_weight=256), "min_weight"),
                     (dict(mapper=None), "map is null")]:
        rc, msg = create(**kw)
        assert rc == -1 and word in msg and not h.value, (kw, rc, msg)
    for W, H in (((1 << 24) + 1, 1), (1 << 14, 1 << 13)):
        rc, msg = create(W=W, H=H)
        assert rc == -4 and not h.value, (W, H, rc, msg)
    pc = RY.params((4.0, 4.0, 4.0, 4.0), 0.5, 0.1, 10)
    assert L.vdo_raycast_create(m._h, 8, 8, None, C.byref(h)) == -1 and "params is null" in L.vdo_last_error().decode()
    assert L.vdo_raycast_create(m._h, 8, 8, C.byref(pc), None) == -1 and "out is null" in L.vdo_last_error().decode()
    assert L.vdo_raycast_create(m._h, 8, 8, C.byref(pc), C.byref(h)) == 0 and h.value
    W = H = 8
    d = np.full((H, W), -7.0, F); g = np.full((H, W, 3), -7.0, F); w = np.full((H, W), -7, np.int32)
    out = (C.c_int64 * 3)(-5, -5, -5)
    T = np.ascontiguousarray(np.eye(4, dtype=F).reshape(16))
    for args, word in [((None, T.ctypes.data, d.ctypes.data, g.ctypes.data, w.ctypes.data, 0, out), "handle is null"),
                       ((h, None, d.ctypes.data, g.ctypes.data, w.ctypes.data, 0, out), "T is null"), ((h, T.ctypes.data, d.ctypes.data, g.ctypes.data, w.ctypes.data, 0, None), "out is null")]:
        assert L.vdo_raycast_render(*args) == -1 and word in L.vdo_last_error().decode(), word
    assert list(out) == [-5, -5, -5] and (d == -7).all() and (g == -7).all() and (w == -7).all()
    ms = (C.c_double * 2)()
    assert L.vdo_raycast_set_skip(None, 1) == -1 and L.vdo_raycast_last_timing(h, None) == -1 and L.vdo_raycast_last_timing(None, ms) == -1
    assert L.vdo_raycast_grid_timing(h, None) == -1 and L.vdo_raycast_destroy(None) == 0
    assert L.vdo_raycast_render(h, T.ctypes.data, d.ctypes.data, g.ctypes.data, w.ctypes.data, 0, out) == 0 and list(out) == [0, 0, 64]      # an empty volume
    assert not d.any() and not g.any() and not w.any()
    assert L.vdo_raycast_destroy(h) == 0
    m.close()


# ---- two views, and the view follows the map ----------------------------------------------------------------------------------------------------
def test_a_second_view_and_a_view_sees_the_new_volume(ctx):
    from vdo_slam_amd.raycast import Raycaster
    m, V = _fused_plane(ctx, (-0.2, 0.0, 1.0))
    T = _yaw(10.0, (0.3, 0.0, 0.0))
    a = Raycaster(m, PW, PH, PK4, NEAR, STEP, STEPS, 2)
    K2 = (55.0, 50.0, 30.2, 9.9)
    b = Raycaster(m, 61, 21, K2, 2.5, 0.15, 40, 3)
    _same(a.render(T), RC.render(V, PW, PH, PK4, NEAR, STEP, STEPS, 2, T), "first view")
    _same(b.render(T), RC.render(V, 61, 21, K2, 2.5, 0.15, 40, 3, T), "second view")
    # one more frame, of a nearer plane from another pose: both views see the new volume
    depth = _plane_depth((0.1, 0.05, 1.0), 4.6)
    T2 = _yaw(-4.0, (0.1, 0.05, 0.0))
    assert m.integrate(depth, None, T2) == V.integrate(depth, None, T2, PK4, 0.4, 0.0, 10.0, 64)
    wa = RC.render(V, PW, PH, PK4, NEAR, STEP, STEPS, 2, T); wb = RC.render(V, 61, 21, K2, 2.5, 0.15, 40, 3, T)
    _same(a.render(T), wa, "first view, new volume")
    _same(b.render(T), wb, "second view, new volume")
    b.close()
    _same(a.render(T), wa, "first view after the second closed")
    a.close(); m.close()
