"""GPU: the device instance labeller (vdo_labels_*, csrc/labels.hip) against the NumPy restatement of its contract (tests/labels_ref.py).
Integer results throughout: every comparison is array_equal of roots, areas, mask and the three counts."""
import ctypes as C

import numpy as np
import pytest

from tests import labels_ref as R

pytestmark = pytest.mark.gpu

TW, TH = 64, 16                                                  # the local-labelling tile of csrc/labels.hip


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _labeler(ctx, H, W, **prm):
    from vdo_slam_amd.labels import InstanceLabeler
    prm.setdefault("min_area", 1)
    prm.setdefault("max_disp_diff", -1)
    return InstanceLabeler(ctx, W, H, **prm)


def _ref(m, cls, disp=None):
    p = m.params
    return R.stages(cls, disp, p.connectivity, p.max_disp_diff, p.min_area, p.max_labels)


def _same(m, cls, disp, want, what=""):
    mask, n, nc, A = m.compute(cls, disp)
    assert np.array_equal(m.roots(), want["roots"]), f"{what}: roots"
    assert np.array_equal(m.areas(), want["areas"]), f"{what}: areas"
    assert mask.dtype == np.int32 and np.array_equal(mask, want["mask"]), f"{what}: mask"
    assert (n, nc, A) == want["counts"], f"{what}: counts {(n, nc, A)} against {want['counts']}"
    assert mask.max(initial=0) < 1024


def _check(ctx, cls, disp=None, what="", **prm):
    H, W = cls.shape
    m = _labeler(ctx, H, W, **prm)
    want = _ref(m, cls, disp)
    _same(m, cls, disp, want, what)
    m.close()
    return want


def _last_error():
    from vdo_slam_amd import _capi as K
    return K.lib().vdo_last_error().decode()


def _ramp(H, W, step=1.0):
    return (np.float32(10) + np.float32(step) * np.arange(W, dtype=np.float32))[None, :].repeat(H, 0).copy()


# ---- sizes: one pixel, one row / column, around the tile in both axes, several tiles with a remainder ----------------------------------
SIZES = [(1, 1), (1, 7), (7, 1)] + [(w, h) for w in (TW - 1, TW, TW + 1) for h in (TH - 1, TH, TH + 1)] + [(96, 64), (200, 37)]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes(ctx, W, H, connectivity):
    cls = R.noise(H, W, 0.59, seed=1000 * H + W, classes=2)
    disp = np.random.default_rng(W + H).integers(0, 5, (H, W)).astype(np.float32) * np.float32(100)
    _check(ctx, cls, None, f"{W}x{H}", connectivity=connectivity)
    _check(ctx, cls, disp, f"{W}x{H} gated", connectivity=connectivity, max_disp_diff=100, min_area=2, max_labels=5)
    _check(ctx, np.ones((H, W), np.uint8), None, f"{W}x{H} constant", connectivity=connectivity)


# ---- patterns at several tiles and at two tiles with a remainder --------------------------------------------------------------------------
PATTERN_SIZES = [(96, 64), (65, 17)]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("W,H", PATTERN_SIZES)
def test_background_and_one_component(ctx, W, H, connectivity):
    want = _check(ctx, np.zeros((H, W), np.uint8), None, "background", connectivity=connectivity)
    assert want["counts"] == (0, 0, 1) and (want["roots"] == -1).all()
    want = _check(ctx, np.full((H, W), 7, np.uint8), None, "constant", connectivity=connectivity)
    assert want["counts"] == (1, 1, 1) and (want["roots"] == 0).all() and want["areas"][0, 0] == W * H


@pytest.mark.parametrize("W,H", PATTERN_SIZES)
def test_checkerboard(ctx, W, H):
    cb = R.checkerboard(H, W)
    want = _check(ctx, cb, None, "checkerboard 4", connectivity=4)
    assert want["counts"][1] == W * H // 2
    if (W, H) == (96, 64):                                       # 3072 singletons overflow the 1023 labels: the threshold rises past every area
        assert want["counts"] == (0, 3072, 2) and (want["mask"] == 0).all()
    want = _check(ctx, cb, None, "checkerboard 8", connectivity=8)
    assert want["counts"] == (1, 1, 1)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("W,H", PATTERN_SIZES)
def test_long_chains(ctx, W, H, connectivity):
    """a spiral, serpentines and combs: one component each, found through parent chains that cross every tile edge many times"""
    for name, a in (("spiral", R.spiral(H, W)), ("serpentine", R.serpentine(H, W)), ("serpentine^T", R.serpentine(W, H).T.copy()),
                    ("comb |", R.comb(H, W, True)), ("comb -", R.comb(H, W, False))):
        want = _check(ctx, a, None, name, connectivity=connectivity)
        assert want["counts"][:2] == (1, 1), name
    inv = (1 - R.spiral(H, W)).astype(np.uint8)                  # the free arm between the spiral's arms
    _check(ctx, inv, None, "inverse spiral", connectivity=connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("density", [0.5, 0.59, 0.7])
def test_noise(ctx, density, seed, connectivity):
    """around the percolation threshold: ragged components over many tiles, the hardest input for races in the border merge"""
    for W, H in PATTERN_SIZES:
        want = _check(ctx, R.noise(H, W, density, seed), None, f"noise {density} seed {seed} {W}x{H}", connectivity=connectivity)
        print(f"{W}x{H} density {density} seed {seed} connectivity {connectivity}: {want['counts'][1]} components")


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("W,H", PATTERN_SIZES)
def test_many_classes(ctx, W, H, connectivity):
    ys, xs = np.mgrid[0:H, 0:W]
    two = (1 + ((xs // 3 + ys // 2) & 1)).astype(np.uint8)       # two classes interleaved, no background
    _check(ctx, two, None, "two classes", connectivity=connectivity)
    many = (1 + (xs // 2 + 33 * ys) % 255).astype(np.uint8)      # 255 classes in cells of two pixels
    want = _check(ctx, many, None, "255 classes", connectivity=connectivity, max_labels=1023)
    assert len(np.unique(many)) == 255 and want["mask"].max() < 1024
    _check(ctx, R.noise(H, W, 0.8, 3, classes=255), None, "255 classes, noise", connectivity=connectivity)


# ---- the disparity gate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_edge", [TW, TW // 2])                # the two rectangles meet on a tile edge / inside a tile
def test_gate_at_the_limit_and_one_beyond(ctx, x_edge):
    H, W, tau = TH + 4, TW + 20, 6
    cls = np.full((H, W), 3, np.uint8)
    for jump, n_comp in ((tau, 1), (tau + 1, 2)):
        disp = np.full((H, W), 50.0, np.float32)
        disp[:, x_edge:] = 50.0 + jump
        want = _check(ctx, cls, disp, f"vertical edge, jump {jump}", connectivity=4, max_disp_diff=tau)
        assert want["counts"][1] == n_comp
        disp = np.full((H, W), 50.0, np.float32)
        disp[TH:, :] = 50.0 + jump                               # and along a horizontal tile edge
        want = _check(ctx, cls, disp, f"horizontal edge, jump {jump}", connectivity=8, max_disp_diff=tau)
        assert want["counts"][1] == n_comp
    disp = np.full((H, W), 50.0, np.float32)
    disp[:, x_edge:] = 50.0 + tau + 1
    disp[5, x_edge - 1] = 0.0                                    # a hole of unknown disparity bridges the jump
    want = _check(ctx, cls, disp, "hole", connectivity=4, max_disp_diff=tau)
    assert want["counts"][1] == 1


def test_gate_unknown_and_fractional_disparities(ctx):
    W, H = 96, 64
    rng = np.random.default_rng(11)
    cls = R.noise(H, W, 0.85, 4, classes=2)
    disp = (rng.integers(1, 40, (H, W)) * 0.37).astype(np.float32) * np.float32(256.0 / 7)      # a scaled disparity with a fractional part
    special = rng.random((H, W))
    disp[special < 0.05] = np.nan
    disp[(special >= 0.05) & (special < 0.10)] = -3.5
    disp[(special >= 0.10) & (special < 0.15)] = np.float32(2.0 ** 24)
    disp[(special >= 0.15) & (special < 0.20)] = np.float32(2.0 ** 24 - 1)
    disp[(special >= 0.20) & (special < 0.25)] = 0.0
    disp[(special >= 0.25) & (special < 0.27)] = np.inf
    for conn in (4, 8):
        for tau in (0, 100, 300):
            _check(ctx, cls, disp, f"special disparities tau {tau}", connectivity=conn, max_disp_diff=tau)
    a = np.ones((1, 4), np.uint8)
    d = np.array([[7.99, 7.0, 8.0, 8.99]], np.float32)           # truncation: 7, 7, 8, 8
    assert _check(ctx, a, d, "truncation", connectivity=4, max_disp_diff=0)["counts"][1] == 2


# ---- selection ------------------------------------------------------------------------------------------------------------------------------
def test_min_area_at_the_area_and_one_above(ctx):
    cls = R.blobs(40, 96, [(20, 10), (7, 3), (1, 1), (5, 5)])    # areas 200, 21, 1, 25
    for min_area, n in ((200, 1), (201, 0), (21, 3), (22, 2), (1, 4), (2, 3)):
        want = _check(ctx, cls, None, f"min_area {min_area}", connectivity=4, min_area=min_area)
        assert want["counts"] == (n, 4, min_area)


@pytest.mark.parametrize("max_labels,A,n", [(1, 10, 0), (3, 9, 2), (5, 1, 5), (1023, 1, 5), (4, 4, 4), (2, 9, 2)])
def test_max_labels_with_ties(ctx, max_labels, A, n):
    cls = R.blobs(TH + 8, TW + 30, [3, 3, 2, 2, 1] * 1)          # areas 9, 9, 4, 4, 1
    want = _check(ctx, cls, None, f"max_labels {max_labels}", connectivity=8, max_labels=max_labels)
    assert want["counts"] == (n, 5, A)


def test_threshold_raise_over_a_wide_range_of_areas(ctx):
    """areas from 1 to several thousand: every radix pass of the threshold search has something to decide"""
    W, H = 200, 37
    cls = np.zeros((H, W), np.uint8)
    cls[0:30, 0:150] = 1                                         # 4500
    cls[0:30, 152:170] = 1                                       # 540
    cls[0:30, 172:189] = 1                                       # 510
    cls[32:35, 0:171] = 1                                        # 513
    cls[32:36:2, 173:199:2] = 1                                  # 26 singletons
    for max_labels in (1, 2, 3, 4, 5, 29, 30):
        want = _check(ctx, cls, None, f"max_labels {max_labels}", connectivity=4, max_labels=max_labels)
        assert want["counts"][1] == 30 and want["counts"][0] == min(max_labels, 4) + (26 if max_labels == 30 else 0)


def test_labels_never_reach_1024(ctx):
    W, H = 96, 64
    cls = np.zeros((H, W), np.uint8)
    cls[::2, ::2] = 1                                            # 1536 singletons
    cls[1, 0:5] = 1                                              # and one larger component that joins three of them
    want = _check(ctx, cls, None, "1536 singletons", connectivity=4, max_labels=1023)
    assert want["counts"][1] > 1023 and want["counts"][0] == 1 and want["mask"].max() == 1
    cls = np.zeros((H, W), np.uint8)
    cls[::2, ::3] = 1                                            # 32 x 32 = 1024 singletons: one too many
    assert _check(ctx, cls, None, "1024 singletons", connectivity=4)["counts"] == (0, 1024, 2)
    cls[0, 0] = 0                                                # 1023: all of them fit
    want = _check(ctx, cls, None, "1023 singletons", connectivity=4)
    assert want["counts"] == (1023, 1023, 1) and want["mask"].max() == 1023


# ---- the speckle filter ---------------------------------------------------------------------------------------------------------------------
def _speckle_image(H, W, sizes):
    disp = _ramp(H, W, 0.25) * np.float32(16)
    keep = R.blobs(H, W, sizes) != 0
    disp[~keep] = 0
    return disp


def _same_filter(m, disp, max_diff, max_size, what=""):
    want = R.filter_speckles(disp, max_diff, max_size)
    got, n = m.filter_speckles(disp, max_diff, max_size)
    assert np.array_equal(m.roots(), want["roots"]) and np.array_equal(m.areas(), want["areas"]), what
    assert np.array_equal(got.view(np.uint32), want["disp"].view(np.uint32)), what      # zeroed or bit for bit as it was
    assert n == want["n_removed"], what
    return want


def test_speckle_filter_around_max_size(ctx):
    W, H = TW + 36, TH + 24
    disp = _speckle_image(H, W, [(3, 3), (5, 2), (11, 1), (4, 3), (30, 12), (70, 3), 1, 1, 2])       # areas 9, 10, 11, 12, 360, 210, 1, 1, 4
    m = _labeler(ctx, H, W)
    for max_size, removed in ((0, 0), (1, 2), (9, 15), (10, 25), (11, 36), (12, 48), (359, 258), (360, 618)):
        want = _same_filter(m, disp, 8, max_size, f"max_size {max_size}")
        assert want["n_removed"] == removed
    want = _same_filter(m, disp, 0, 12, "max_diff 0")            # the ramp now cuts the wide blobs into columns of equal disparity
    assert want["n_removed"] > 48
    disp[3, 2] = np.nan; disp[20, 50] = -1.0                     # unknown values belong to no component and stay as they are
    _same_filter(m, disp, 8, 10, "unknown values")
    m.close()


@pytest.mark.parametrize("W,H", [(1, 1), (TW + 1, TH + 1), (200, 37)])
def test_speckle_filter_noise(ctx, W, H):
    rng = np.random.default_rng(W)
    disp = (rng.integers(1, 6, (H, W)) * (rng.random((H, W)) < 0.6)).astype(np.float32) * np.float32(256.7)
    m = _labeler(ctx, H, W)
    for max_diff, max_size in ((0, 3), (257, 10), (600, 40), (10 ** 6, 10 ** 6)):
        _same_filter(m, disp, max_diff, max_size, f"{W}x{H} {max_diff} {max_size}")
    m.close()


def test_filter_and_compute_on_one_handle_share_no_state(ctx):
    import torch
    W, H = 96, 64
    cls = R.noise(H, W, 0.59, 21, classes=2)
    disp = _speckle_image(H, W, [(3, 3), (40, 20), 2, (30, 30)])
    m = _labeler(ctx, H, W, connectivity=8, max_disp_diff=40, min_area=3, max_labels=6)
    want = _ref(m, cls, disp)
    _same(m, cls, disp, want, "compute")
    _same_filter(m, disp, 8, 9, "filter after compute")
    _same(m, cls, disp, want, "compute after filter")
    t = torch.from_numpy(disp).cuda()                            # in place on a device image
    torch.cuda.synchronize()
    ref = R.filter_speckles(disp, 8, 9)
    assert m.filter_speckles_raw(t.data_ptr(), True, 8, 9) == ref["n_removed"]
    assert np.array_equal(t.cpu().numpy().view(np.uint32), ref["disp"].view(np.uint32))
    _same(m, cls, disp, want, "compute after a device filter")
    m.close()


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dev", [False, True])
@pytest.mark.parametrize("src_dev", [False, True])
def test_padded_strides_and_memory_spaces(ctx, src_dev, out_dev):
    import torch
    W, H = 65, 17
    cls = R.noise(H, W, 0.7, 8, classes=3)
    disp = np.random.default_rng(2).integers(0, 4, (H, W)).astype(np.float32) * np.float32(10)
    sc, sd = W + 13, W + 3
    bufc = np.full((H, sc), 255, np.uint8); bufc[:, :W] = cls
    bufd = np.full((H, sd), 10.0, np.float32); bufd[:, :W] = disp
    m = _labeler(ctx, H, W, connectivity=8, max_disp_diff=10, min_area=2, max_labels=9)
    want = _ref(m, cls, disp)
    keep = []
    if src_dev:
        tc, td = torch.from_numpy(bufc).cuda(), torch.from_numpy(bufd).cuda()
        keep += [tc, td]
        pc, pd = tc.data_ptr(), td.data_ptr()
    else:
        pc, pd = bufc.ctypes.data, bufd.ctypes.data
    if out_dev:
        tm = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
        pm = tm.data_ptr()
    else:
        hm = np.full((H, W), -7, np.int32)
        pm = hm.ctypes.data
    torch.cuda.synchronize()
    counts = m.compute_raw(pc, sc, pd, sd, src_dev, pm, out_dev)
    mask = tm.cpu().numpy() if out_dev else hm
    assert np.array_equal(mask, want["mask"]) and counts == want["counts"]
    assert np.array_equal(m.roots(), want["roots"]) and np.array_equal(m.areas(), want["areas"])
    if src_dev:                                                  # packed device images are read where they lie
        tc2, td2 = torch.from_numpy(cls).cuda(), torch.from_numpy(disp).cuda()
        torch.cuda.synchronize()
        assert m.compute_raw(tc2.data_ptr(), W, td2.data_ptr(), W, True, pm, out_dev) == want["counts"]
        assert np.array_equal(tm.cpu().numpy() if out_dev else hm, want["mask"])
    m.close()


def test_the_handles_own_device_images(ctx):
    W, H = 65, 17
    cls = R.noise(H, W, 0.59, 9, classes=2)
    m = _labeler(ctx, H, W, connectivity=4)
    want = _ref(m, cls)
    d_cls, d_mask = m.device_images()
    assert d_cls and d_mask and d_cls != d_mask
    assert m.stage_classes(cls) == d_cls
    assert m.compute_raw(d_cls, W, None, 0, True, d_mask, True) == want["counts"]
    assert np.array_equal(m.roots(), want["roots"]) and np.array_equal(m.areas(), want["areas"])
    import torch
    out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert m.compute_raw(d_cls, W, None, 0, True, out.data_ptr(), True) == want["counts"]
    assert np.array_equal(out.cpu().numpy(), want["mask"])
    wall, dev = m.timing()
    assert wall > 0 and dev > 0
    m.close()


def test_two_computes_on_one_handle_share_no_state(ctx):
    W, H = 96, 64
    a, b = R.noise(H, W, 0.59, 31), R.checkerboard(H, W)
    m = _labeler(ctx, H, W, connectivity=4)
    wa, wb = _ref(m, a), _ref(m, b)
    _same(m, a, None, wa, "first")
    _same(m, b, None, wb, "second (the threshold rises)")
    _same(m, a, None, wa, "first again")
    m.close()


@pytest.mark.parametrize("kw,word,code", [
    (dict(W=0), "width", -1), (dict(H=0), "height", -1), (dict(W=-5), "width", -1),
    (dict(connectivity=6), "connectivity", -1), (dict(connectivity=0), "connectivity", -1), (dict(max_disp_diff=-2), "max_disp_diff", -1),
    (dict(min_area=0), "min_area", -1), (dict(max_labels=0), "max_labels", -1), (dict(max_labels=1024), "max_labels", -1),
    (dict(W=8192, H=8193), "2^26", -4),
])
def test_create_refusals(ctx, kw, word, code):
    from vdo_slam_amd import _capi as K
    kw = dict(kw)
    W, H = kw.pop("W", 32), kw.pop("H", 16)
    with pytest.raises(K.VdoError, match=word.replace("^", r"\^")) as e:
        _labeler(ctx, H, W, **kw)
    assert e.value.code == code


def test_compute_and_filter_refusals_write_nothing(ctx):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd import labels
    H, W = 16, 32
    m = _labeler(ctx, H, W, max_disp_diff=5)
    cls = np.ones((H, W), np.uint8); disp = np.ones((H, W), np.float32)
    mask = np.full((H, W), -7, np.int32)
    pc, pd, pm = cls.ctypes.data, disp.ctypes.data, mask.ctypes.data
    for fn in (m.roots, m.areas):                                # inspection before the first compute or filter
        with pytest.raises(K.VdoError, match="no vdo_labels_compute"):
            fn()
    for args, word in (((0, W, pd, W), "cls"), ((pc, W - 1, pd, W), "cls_stride"), ((pc, 0, pd, W), "cls_stride"), ((pc, W, 0, W), "disp"),
                       ((pc, W, pd, W - 1), "disp_stride_floats")):
        with pytest.raises(K.VdoError, match=word) as e:
            m.compute_raw(*args, False, pm, False)
        assert e.value.code == -1 and (mask == -7).all()
    with pytest.raises(K.VdoError, match="mask"):
        m.compute_raw(pc, W, pd, W, False, 0, False)
    L = labels._lib()
    out = (C.c_int32 * 3)(-7, -7, -7)
    assert L.vdo_labels_compute(m._h, pc, W, pd, W, 0, pm, 0, None) == -1 and "out" in _last_error() and (mask == -7).all()
    assert L.vdo_labels_compute(None, pc, W, pd, W, 0, pm, 0, out) == -1 and "handle" in _last_error() and (mask == -7).all() and list(out) == [-7] * 3
    before = disp.copy()
    n = C.c_int32(-7)
    for args, word in (((pd, 0, -1, 3), "max_diff"), ((pd, 0, 3, -1), "max_size"), ((0, 0, 3, 3), "disparity256")):
        with pytest.raises(K.VdoError, match=word) as e:
            m.filter_speckles_raw(*args)
        assert e.value.code == -1 and np.array_equal(disp, before)
    assert L.vdo_labels_filter_speckles(m._h, pd, 0, 3, 3, None) == -1 and "n_removed" in _last_error() and np.array_equal(disp, before)
    assert L.vdo_labels_create(ctx._h, W, H, None, C.byref(C.c_void_p())) == -1 and "params" in _last_error()
    for fn in (m.roots, m.areas):                                # none of the refused calls counts as a compute
        with pytest.raises(K.VdoError, match="no vdo_labels_compute"):
            fn()
    m.close()
    m = _labeler(ctx, H, W)                                      # gate off: no disparity is needed, and none is read
    assert m.compute_raw(pc, W, 0, 0, False, pm, False) == (1, 1, 1) and (mask == 1).all()
    m.close()


# ---- host classes ---------------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_instancelabeler_class_equals_the_c_entry(ctx):
    from vdo_slam_amd import _capi as K
    host = K.load_host_lib()
    host.host_labels_compute.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    W, H = 131, 37
    cls = R.noise(H, W, 0.65, 41, classes=3)
    disp = np.random.default_rng(3).integers(0, 5, (H, W)).astype(np.float32) * np.float32(64)
    want = R.stages(cls, disp, 8, 64, 4, 7)
    prm = np.array([8, 64, 4, 7], np.int32)
    padded = np.zeros((H, W + 5), np.uint8); padded[:, :W] = cls                       # (cv::Mat with row steps of their own)
    dpad = np.zeros((H, W + 2), np.float32); dpad[:, :W] = disp
    mask = np.full((H, W), -1, np.int32); counts = np.full(3, -1, np.int32)
    assert host.host_labels_compute(_ptr(padded), W + 5, _ptr(dpad), W + 2, W, H, _ptr(prm), _ptr(mask), _ptr(counts)) == want["counts"][0]
    assert np.array_equal(mask, want["mask"]) and tuple(counts) == want["counts"]
    prm[1] = -1                                                                         # gate off: no disparity image
    want = R.stages(cls, None, 8, -1, 4, 7)
    assert host.host_labels_compute(_ptr(padded), W + 5, None, 0, W, H, _ptr(prm), _ptr(mask), None) == want["counts"][0]
    assert np.array_equal(mask, want["mask"])
    prm[0] = 5                                                                          # a refusal surfaces as a failure, not as an exit
    assert host.host_labels_compute(_ptr(cls), W, None, 0, W, H, _ptr(prm), _ptr(mask), None) == -1
    from vdo_slam_amd import labels
    got = labels.compute(ctx, cls, connectivity=4, min_area=3)
    ref = R.stages(cls, None, 4, -1, 3, 1023)
    assert np.array_equal(got[0], ref["mask"]) and got[1:] == ref["counts"]
    d2, n = labels.filter_speckles(ctx, disp, 64, 5)
    ref = R.filter_speckles(disp, 64, 5)
    assert np.array_equal(d2.view(np.uint32), ref["disp"].view(np.uint32)) and n == ref["n_removed"]


def _forward_warp(img, flow, seed):
    """The next image of a frame: noise under the forward warp of `img` by its (rounded) flow"""
    H, W = img.shape
    out = np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    xt, yt = xs + np.rint(flow[..., 0]).astype(np.int64), ys + np.rint(flow[..., 1]).astype(np.int64)
    ok = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
    out[yt[ok], xt[ok]] = img[ok]
    return out


def test_trackstereopairsemantic_equals_trackstereopair_on_the_device_mask(ctx, tmp_path):
    """System(STEREO).TrackStereoPairSemantic over 3 frames against TrackStereoPair fed the mask vdo_labels_compute returned for the same
    disparity and class image"""
    from tests import stereo_ref as SR
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.labels import InstanceLabeler
    from vdo_slam_amd.stereo import StereoMatcher
    from vdo_slam_amd.system import System, write_settings
    W, H, n_frames = synth.KITTI_W, synth.KITTI_H, 3
    cfg = write_settings(tmp_path / "k.yaml", W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    Ts = SQ.camera_poses(n_frames); objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs) for k in range(n_frames)]
    rights, nexts, classes = [], [], []
    for k, fr in enumerate(frames):
        disp = np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64)
        right = np.random.default_rng(500 + k).integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(fr["gray"], disp, right)
        rights.append(right)
        nexts.append(_forward_warp(fr["gray"], fr["flow"], 900 + k))
        classes.append((fr["mask"] > 0).astype(np.uint8) * 26)   # one class for every object: the instances are gone
    # the masks the labeller makes from the matcher's disparity (the settings file has no Stereo.* or Labels.* key: the defaults; the depth image
    # is the disparity x DepthMapFactor / 256)
    sm = StereoMatcher(ctx, W, H)
    sm.set_output_scale(SF.DEPTH_MAP_FACTOR / 256.0)
    lab = InstanceLabeler(ctx, W, H)
    unit = SF.DEPTH_MAP_FACTOR / 256.0
    assert lab.params.max_disp_diff * unit == 512 and lab.params.min_area == 200
    masks = []
    for k, fr in enumerate(frames):
        d = sm.compute(fr["gray"], rights[k])
        d = d[0] if isinstance(d, tuple) else d
        mask, n, nc, A = lab.compute(classes[k], d)
        print(f"frame {k}: {n} labels of {nc} components, threshold {A}")
        assert n >= 1
        masks.append(mask)
    sm.close(); lab.close()
    n_max = max(int(m.max()) for m in masks)
    rows = np.array([[0, label, 0, 0, 0, 0, 0, 0, 0, 0] for label in range(1, n_max + 1)], np.float32)
    s = System(cfg, sensor="stereo")
    poses = [s.track_stereo_pair_semantic(fr["gray"], rights[k], nexts[k], classes[k], rows, n_images=n_frames) for k, fr in enumerate(frames)]
    motions = s.motions()
    s.close()
    assert all(T is not None for T in poses)
    s = System(cfg, sensor="stereo")
    want = [s.track_stereo_pair(fr["gray"], rights[k], nexts[k], masks[k].copy(), rows, n_images=n_frames) for k, fr in enumerate(frames)]
    want_motions = s.motions()
    s.close()
    for k in range(n_frames):
        assert np.array_equal(poses[k], want[k]), k
    assert len(motions) == len(want_motions)
    for (la, Ha), (lb, Hb) in zip(motions, want_motions):
        assert la == lb and np.array_equal(Ha, Hb)
    assert not np.array_equal(poses[-1], np.eye(4, dtype=np.float32))
