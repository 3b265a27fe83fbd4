"""The Frame-side image kernels across sizes and edge cases: k_ingest (vdo_frame_images_ingest_device), K1 / K2 on their own
(vdo_depth_preprocess, vdo_rgb2gray), K10 (vdo_frame_object_sample: three launches and the host collection) and K9
(vdo_frame_static_filter, both branches).  Every output is an integer or an fp32 value that both sides compute with the same IEEE
operations, so everything is array_equal.  References: the CPU oracle and the NumPy restatements of tests/image_kernels_ref.py;
where both exist the GPU tests assert oracle == NumPy == GPU, and the ``not gpu`` tests below assert oracle == NumPy on the same
inputs.  Every case asserts the counts that put it where it says (kept counts, workgroup counts, which path ran)."""
import ctypes as C

import numpy as np
import pytest

from tests import frontend_ref as R
from tests import image_kernels_ref as N
from vdo_slam_amd import _capi as K
from vdo_slam_amd.synth_frames import BF, DEPTH_MAP_FACTOR, TH_DEPTH_BG, TH_DEPTH_OBJ

gpu = pytest.mark.gpu
K9_KEYS = ("keep_idx", "corr_x", "corr_y", "flow_x", "flow_y", "depth")
K10_KEYS = ("key_x", "key_y", "corr_x", "corr_y", "flow_x", "flow_y", "depth", "label")
K_OBJ_SPEC = 8192                       # kObjSpec of csrc/frame.hip: result columns that come back with the count
SCALES = [(BF, DEPTH_MAP_FACTOR), (386.1448, 5000.0 / 3.0)]          # synth_frames' pair (factor a power of two) and one that is not


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _same_bits(a, b, keys, what=""):
    """array_equal on the bit patterns (a denormal or a signed zero must not pass as its neighbour)."""
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k}"


def oracle_depth(o, d, bf, factor):
    out = np.array(d, np.float32)
    o.vdo_oracle_depth_preprocess(R._fp(out), out.size, bf, factor)
    return out


def oracle_gray(o, img, rgb_order):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(img.shape[:2], np.uint8)
    o.vdo_oracle_rgb2gray(R._u8(img), out.size, img.shape[2], 1 if rgb_order else 0, R._u8(out))
    return out


def oracle_static_filter(o, kx, ky, mask, depth, flow, th, sampled):
    if not sampled:
        return R.static_filter(o, kx, ky, np.zeros(kx.size, np.int32), mask, depth, flow, th)
    n = kx.size
    h, w = mask.shape
    idx = np.zeros(n, np.int32); f = [np.zeros(n, np.float32) for _ in range(5)]
    o.vdo_oracle_frame_static_filter_sampled.argtypes = [C.c_int, K.c_float_p, K.c_float_p, K.c_int32_p, K.c_float_p, K.c_float_p, C.c_int, C.c_int, C.c_float,
                                                         K.c_int32_p] + [K.c_float_p] * 5
    m = o.vdo_oracle_frame_static_filter_sampled(n, R._fp(kx), R._fp(ky), R._ip(mask), R._fp(depth), R._fp(flow), w, h, th, R._ip(idx), *[R._fp(a) for a in f])
    return dict(keep_idx=idx[:m], corr_x=f[0][:m], corr_y=f[1][:m], flow_x=f[2][:m], flow_y=f[3][:m], depth=f[4][:m])


def _gray_images():
    """(name, [h, w, 4] RGBA image): 1, 255 and 257 pixels and 64 x 96, the pixels on / one short of a rounding step first."""
    steps = N.gray_step_pixels()
    rng = np.random.default_rng(0)
    out = []
    for shape in ((1, 1), (1, 255), (1, 257), (64, 96)):
        n = shape[0] * shape[1]
        px = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        k = min(n, steps.shape[0])
        px[:k, :3] = steps[::-1][:k]                 # (255, 255, 255) is among the last of the list: it leads, so the 1-pixel image is white
        out.append((f"{shape[1]}x{shape[0]}", px.reshape(shape[0], shape[1], 4)))
    assert tuple(out[0][1][0, 0, :3]) in ((255, 255, 255), (0, 0, 0))
    return out


# =============================================================================================================================
# without a GPU: the NumPy restatements against the oracle, on the inputs of the GPU tests
# =============================================================================================================================
def test_numpy_k1_k2_equal_the_oracle(oracle):
    for bf, factor in SCALES:
        for n in (1, 255, 256, 257, 1242 * 375):
            d = N.raw_depth(n, n)
            assert N.bits_equal(N.depth_preprocess(d, bf, factor), oracle_depth(oracle, d, bf, factor)), (n, bf)
    # the special values do what the formula says: negative -> 0, +0 -> +inf, -0 -> -inf, inf -> 0, NaN -> NaN
    out = N.depth_preprocess(N.SPECIAL_DEPTH, BF, DEPTH_MAP_FACTOR)
    assert out[0] == 0 and out[1] == -np.inf and out[2] == np.inf and out[3] == 0 and np.isnan(out[4]) and out[7] == 0 and np.isfinite(out[5]) and out[5] > 0
    steps = N.gray_step_pixels()
    s = steps.astype(np.int64)
    res = (s[:, 0] * 4899 + s[:, 1] * 9617 + s[:, 2] * 1868 + 8192) & 16383
    assert (res == 0).sum() > 100 and (res == 16383).sum() > 100 and (steps == 255).all(axis=1).any()
    for name, img in _gray_images():
        for ch in (3, 4):
            for order in (True, False):
                assert np.array_equal(N.rgb2gray(img[..., :ch], order), oracle_gray(oracle, img[..., :ch], order)), (name, ch, order)
    # a pixel one short of a step and its neighbour on the step differ by one grey level
    assert N.rgb2gray(np.array([[[255, 255, 255]]], np.uint8))[0, 0] == 255


def test_numpy_k10_equals_the_oracle(oracle):
    for w, h, step in N.K10_SHAPES:
        mask, depth, flow, kept = N.k10_image(w, h, step)
        a = N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, step)
        b = R.object_sample(oracle, mask, depth, flow, TH_DEPTH_OBJ, step)
        assert a["label"].size == kept, (w, h, step)
        _same_bits(a, b, K10_KEYS, f"{w}x{h}/{step}")
    for kept in (0, 1, 8192, 8193, 10001):
        mask, depth, flow = N.k10_count_image(kept)
        a = N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, 4)
        assert a["label"].size == kept
        _same_bits(a, R.object_sample(oracle, mask, depth, flow, TH_DEPTH_OBJ, 4), K10_KEYS, f"kept {kept}")
    mask, depth, flow, probes = N.k10_big_image()
    a = N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, 4)
    assert np.array_equal(a["label"], 1 + np.arange(len(probes)))
    _same_bits(a, R.object_sample(oracle, mask, depth, flow, TH_DEPTH_OBJ, 4), K10_KEYS, "2048x2052")


def test_numpy_k9_equals_the_oracle(oracle):
    for w, h in ((320, 200), (64, 48)):
        for n in N.K9_N:
            for pat in N.K9_PATTERNS:
                kx, ky, mask, depth, flow, keep = N.k9_case(w, h, n, pat)
                for sampled in (False, True):
                    a = N.static_filter(kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled)
                    assert np.array_equal(a["keep_idx"], np.nonzero(keep)[0]), (w, n, pat, sampled)
                    _same_bits(a, oracle_static_filter(oracle, kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled), K9_KEYS, f"{w} {n} {pat} {sampled}")
    kx, ky, mask, depth, flow, names, k_orb, k_smp = N.k9_boundary_case()
    for sampled, exp in ((False, k_orb), (True, k_smp)):
        a = N.static_filter(kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled)
        b = oracle_static_filter(oracle, kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled)
        # both references agree with what the rows were built to do - in particular "px + fx < 0 is kept" in the ORB branch, which checks
        # the right and the bottom side only (src/Frame.cc:116-124)
        got = np.zeros(kx.size, bool); got[a["keep_idx"]] = True
        assert [n for n, g, e in zip(names, got, exp) if g != e] == [], sampled
        _same_bits(a, b, K9_KEYS, f"boundary rows, sampled={sampled}")


# =============================================================================================================================
# 1. vdo_frame_images_ingest_device
# =============================================================================================================================
INGEST_SIZES = [(1, 1), (3, 1), (2, 2), (5, 1), (7, 3), (257, 3), (1242, 375)]


def _ingest_inputs(w, h):
    n = w * h
    rng = np.random.default_rng(n)
    depth = N.raw_depth(n, n).reshape(h, w)
    flow = rng.normal(0, 3, (h, w, 2)).astype(np.float32)
    flow.ravel()[: min(4, 2 * n)] = np.array([-0.0, np.inf, 1e-42, -7.5], np.float32)[: min(4, 2 * n)]     # copied bit for bit, whatever they are
    mask = rng.integers(-3, 9, (h, w)).astype(np.int32)
    mask.ravel()[-1] = np.iinfo(np.int32).min
    return depth, flow, mask


@gpu
@pytest.mark.parametrize("w,h", INGEST_SIZES)
def test_ingest_device_sizes_tails_and_unaligned_sources(ctx, oracle, w, h):
    """The float4 body, the element-by-element tail (pixel count = 0, 1, 2, 3 mod 4), fewer than 4 pixels (the n4 == 0 launch), more than
    one workgroup, and the fallback for sources that are not 16-byte aligned (copies + K1): all the same bits."""
    import torch
    from vdo_slam_amd.frontend import FrameImages
    from vdo_slam_amd.tracking import download_mask
    n = w * h
    depth, flow, mask = _ingest_inputs(w, h)
    assert {(a * b) % 4 for a, b in INGEST_SIZES} == {0, 1, 2, 3} and min(a * b for a, b in INGEST_SIZES) < 4 and max(a * b for a, b in INGEST_SIZES) // 4 > 256
    dev = torch.device("cuda")
    # one element of slack in front: [1:] is the source moved by one element (4 bytes: off the 16-byte grid)
    td = torch.zeros(n + 8, dtype=torch.float32, device=dev); tf = torch.zeros(2 * n + 8, dtype=torch.float32, device=dev); tm = torch.zeros(n + 8, dtype=torch.int32, device=dev)
    im = FrameImages(ctx, w, h)
    junk = (np.full((h, w), 7.0, np.float32), np.full((h, w, 2), 7.0, np.float32), np.full((h, w), 7, np.int32))
    for bf, factor in SCALES:
        for convert in (0, 1):
            exp_d, exp_f, exp_m = N.ingest(depth, flow, mask, bf, factor, convert)
            if convert:
                assert N.bits_equal(exp_d, oracle_depth(oracle, depth, bf, factor))
            for shifted in (None, "depth", "flow", "mask"):
                offs = {k: (1 if shifted == k else 0) for k in ("depth", "flow", "mask")}
                for name, t, cnt, a in (("depth", td, n, depth), ("flow", tf, 2 * n, flow), ("mask", tm, n, mask)):
                    t.zero_()
                    t[offs[name]:offs[name] + cnt] = torch.from_numpy(a.ravel()).to(dev)
                ptr = [t[offs[k]:].data_ptr() for k, t in (("depth", td), ("flow", tf), ("mask", tm))]
                aligned = all(p % 16 == 0 for p in ptr)
                assert aligned == (shifted is None), "k_ingest takes 16-byte aligned sources, the fallback anything else"
                im.upload(*junk)
                torch.cuda.synchronize()                       # the library works on its own stream
                im.ingest_device(ptr[0], ptr[1], ptr[2], bf, factor, convert)
                got_d, got_f = im.download_depth(), im.download_flow()
                got_m = download_mask(im)
                what = (w, h, bf, convert, shifted)
                assert N.bits_equal(got_d, exp_d), what
                assert got_f.tobytes() == exp_f.tobytes() and got_m.tobytes() == exp_m.tobytes(), what
    im.close()


# =============================================================================================================================
# 2. K1 / K2 on their own
# =============================================================================================================================
@gpu
def test_depth_preprocess_and_rgb2gray_on_their_own(ctx, oracle):
    from vdo_slam_amd.frontend import depth_preprocess, rgb2gray
    for bf, factor in SCALES:
        for n in (1, 255, 256, 257):
            d = N.raw_depth(n, n)
            exp = N.depth_preprocess(d, bf, factor)
            assert N.bits_equal(exp, oracle_depth(oracle, d, bf, factor))
            assert N.bits_equal(depth_preprocess(ctx, d, bf, factor), exp), (n, bf)
    for name, img in _gray_images():
        for ch in (3, 4):
            for order in (True, False):
                src = np.ascontiguousarray(img[..., :ch])
                exp = N.rgb2gray(src, order)
                assert np.array_equal(exp, oracle_gray(oracle, src, order))
                assert np.array_equal(rgb2gray(ctx, src, order), exp), (name, ch, order)


# =============================================================================================================================
# 3. K10
# =============================================================================================================================
def _upload(ctx, mask, depth, flow):
    from vdo_slam_amd.frontend import FrameImages
    h, w = mask.shape
    im = FrameImages(ctx, w, h)
    im.upload(depth, flow, mask)
    return im


def _nblk(w, h, step):
    return (((w + step - 1) // step) * ((h + step - 1) // step) + 255) // 256


@gpu
@pytest.mark.parametrize("w,h,step", N.K10_SHAPES)
def test_object_sample_sizes_steps_and_bounds(ctx, oracle, w, h, step):
    """Probe p is of category p % 15 (tests/image_kernels_ref.K10_CATS): negative labels kept, depth exactly th_obj dropped and the float
    below it kept, landing exactly on 0 / w / h dropped and on the nearest float inside kept.  Shapes of 1 to 115 workgroups."""
    mask, depth, flow, kept = N.k10_image(w, h, step)
    exp = N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, step)
    _same_bits(exp, R.object_sample(oracle, mask, depth, flow, TH_DEPTH_OBJ, step), K10_KEYS, "oracle")
    assert exp["label"].size == kept and (kept >= 1)
    if w * h > 16:
        assert (exp["label"] < 0).sum() > 0 and kept < ((w + step - 1) // step) * ((h + step - 1) // step)
    im = _upload(ctx, mask, depth, flow)
    got = im.object_sample(TH_DEPTH_OBJ, step)
    _same_bits(got, exp, K10_KEYS, f"{w}x{h}/{step}")
    if (w, h, step) in ((1242, 375, 4), (61, 37, 3), (1, 1, 4)):          # K9 + K10 in one call = the two separate calls
        rng = np.random.default_rng(w)
        kx = rng.uniform(0, w, 300).astype(np.float32); ky = rng.uniform(0, h, 300).astype(np.float32)
        m0 = np.where(mask == 3, 0, mask)                                 # (background between the probes, so that K9 keeps some)
        im.upload(depth, flow, m0)
        sep_s = {k: v.copy() for k, v in im.static_filter(kx, ky, TH_DEPTH_BG).items()}
        sep_o = {k: v.copy() for k, v in im.object_sample(TH_DEPTH_OBJ, step).items()}
        st, ob = im.filters(kx, ky, TH_DEPTH_BG, TH_DEPTH_OBJ, step)
        _same_bits(st, sep_s, K9_KEYS, "filters: K9"); _same_bits(ob, sep_o, K10_KEYS, "filters: K10")
        _same_bits(st, N.static_filter(kx, ky, m0, depth, flow, TH_DEPTH_BG, False), K9_KEYS, "filters: K9 reference")
        _same_bits(ob, N.object_sample(m0, depth, flow, TH_DEPTH_OBJ, step), K10_KEYS, "filters: K10 reference")
        assert ob["label"].size >= 1 and (w * h < 16 or st["keep_idx"].size > 20)
    im.close()


@gpu
def test_object_sample_kept_counts_around_the_second_copy(ctx, oracle):
    """512 x 320, all object: 10 240 probes, exactly 0 / 1 / 8192 / 8193 / 10 001 kept.  Up to 8192 (kObjSpec) columns come back with the
    count; one more takes the second strided copy.  Then the refusals: an output capacity one below the kept count, and a step whose
    probes exceed the scratch capacity - VdoError, outputs untouched."""
    im = None
    for kept in (0, 1, 8192, 8193, 10001):
        mask, depth, flow = N.k10_count_image(kept)
        exp = N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, 4)
        _same_bits(exp, R.object_sample(oracle, mask, depth, flow, TH_DEPTH_OBJ, 4), K10_KEYS, "oracle")
        assert exp["label"].size == kept
        if im is None:
            im = _upload(ctx, mask, depth, flow)
        else:
            im.upload(depth, flow, mask)
        got = im.object_sample(TH_DEPTH_OBJ, 4)
        second_copy = got["label"].size > K_OBJ_SPEC
        assert second_copy == (kept in (8193, 10001)), kept
        _same_bits(got, exp, K10_KEYS, f"kept {kept}")
        st, ob = im.filters(np.array([5.5], np.float32), np.array([6.5], np.float32), TH_DEPTH_BG, TH_DEPTH_OBJ, 4)     # (the second scratch set)
        _same_bits(ob, exp, K10_KEYS, f"filters, kept {kept}")
        if kept in (1, 8193):            # a capacity one below the count
            with pytest.raises(K.VdoError, match="exceed the output capacity"):
                _sentinel_object_sample(im, TH_DEPTH_OBJ, 4, kept - 1)
    im.close()
    # probes over the scratch capacity: 128 x 128 at step 1 = 16 384 probes, capacity 32 * 32 + 4096 = 5120
    mask, depth, flow, _ = N.k10_image(128, 128, 1)
    im = _upload(ctx, mask, depth, flow)
    assert 128 * 128 > (128 // 4) * (128 // 4) + 4096
    with pytest.raises(K.VdoError, match="scratch capacity"):
        _sentinel_object_sample(im, TH_DEPTH_OBJ, 1, 128 * 128)
    got = im.object_sample(TH_DEPTH_OBJ, 4)                              # and the image set still works
    _same_bits(got, N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, 4), K10_KEYS, "after the refusal")
    im.close()


def _sentinel_object_sample(im, th, step, cap):
    """vdo_frame_object_sample into sentinel-filled buffers of ``cap`` entries (+ a guard entry); on an error the buffers must be
    untouched, which is asserted before the error is passed on."""
    from vdo_slam_amd import frontend as FE
    L = FE._lib()
    f = [np.full(cap + 1, -777.0, np.float32) for _ in range(7)]
    lab = np.full(cap + 1, -777, np.int32)
    m = C.c_int(-5)
    rc = L.vdo_frame_object_sample(im._h, th, step, cap, *[R._fp(a) for a in f], R._ip(lab), C.byref(m))
    if rc != 0:
        assert all((a == -777.0).all() for a in f) and (lab == -777).all(), "outputs written although the call was refused"
    K.check(rc)
    return f, lab, m.value


@gpu
def test_object_sample_second_scan_chunk(ctx, oracle):
    """2048 x 2052 at step 4: 262 656 probes = 1026 workgroups, so the scan of the workgroup counts (1024 per chunk) carries into a
    second chunk.  Kept probes lie in the first, the 1024th, the 1025th and the last workgroup; output order = raster order."""
    mask, depth, flow, probes = N.k10_big_image()
    assert _nblk(2048, 2052, 4) == 1026 and sorted({p // 256 for p in probes}) == [0, 1023, 1024, 1025]
    exp = N.object_sample(mask, depth, flow, TH_DEPTH_OBJ, 4)
    _same_bits(exp, R.object_sample(oracle, mask, depth, flow, TH_DEPTH_OBJ, 4), K10_KEYS, "oracle")
    assert np.array_equal(exp["label"], 1 + np.arange(len(probes)))       # the labels count the kept probes in raster order
    im = _upload(ctx, mask, depth, flow)
    got = im.object_sample(TH_DEPTH_OBJ, 4)
    _same_bits(got, exp, K10_KEYS, "2048x2052")
    im.close()


# =============================================================================================================================
# 4. K9, both branches
# =============================================================================================================================
@gpu
@pytest.mark.parametrize("w,h", [(320, 200), (64, 48)])
def test_static_filter_keep_patterns_across_waves_and_chunks(ctx, oracle, w, h):
    """n around the wave (64) and chunk (1024) sizes x six keep patterns made through the mask / depth / flow under the points x both
    branches: keep_idx ascending and every row equal to the references."""
    from vdo_slam_amd.frontend import FrameImages
    im = FrameImages(ctx, w, h)
    for n in N.K9_N:
        for pat in N.K9_PATTERNS:
            kx, ky, mask, depth, flow, keep = N.k9_case(w, h, n, pat)
            im.upload(depth, flow, mask)
            for sampled in (False, True):
                exp = N.static_filter(kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled)
                assert np.array_equal(exp["keep_idx"], np.nonzero(keep)[0])
                got = im.static_filter(kx, ky, TH_DEPTH_BG, sampled=sampled)
                assert (np.diff(got["keep_idx"]) > 0).all()
                _same_bits(got, exp, K9_KEYS, f"{w}x{h} n={n} {pat} sampled={sampled}")
        if n in (1, 1025, 3000):           # one of each against the oracle on the GPU machine too (all of them are, without a GPU, above)
            _same_bits(exp, oracle_static_filter(oracle, kx, ky, mask, depth, flow, TH_DEPTH_BG, True), K9_KEYS, "oracle")
    im.close()


@gpu
def test_static_filter_boundary_rows(ctx, oracle):
    kx, ky, mask, depth, flow, names, k_orb, k_smp = N.k9_boundary_case()
    im = _upload(ctx, mask, depth, flow)
    for sampled, flags in ((False, k_orb), (True, k_smp)):
        exp = N.static_filter(kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled)
        _same_bits(exp, oracle_static_filter(oracle, kx, ky, mask, depth, flow, TH_DEPTH_BG, sampled), K9_KEYS, "oracle")
        assert np.array_equal(exp["keep_idx"], np.nonzero(flags)[0])
        got = im.static_filter(kx, ky, TH_DEPTH_BG, sampled=sampled)
        kept = np.zeros(kx.size, bool); kept[got["keep_idx"]] = True
        assert [n for n, g, e in zip(names, kept, flags) if g != e] == [], f"sampled={sampled}"
        _same_bits(got, exp, K9_KEYS, f"sampled={sampled}")
    assert k_orb[names.index("px + fx < 0")] and not k_smp[names.index("px + fx < 0")]
    im.close()


@gpu
def test_static_filter_staging_limit(ctx, oracle):
    """64 x 48: capacity 16 * 12 + 4096 = 4288 columns, the staging block holds 8 of them per row and a call needs 10 n: 3430 keypoints
    run, 3431 are refused (both branches, and through filters())."""
    w, h = 64, 48
    cap = (w // 4) * (h // 4) + 4096
    assert cap == 4288 and 10 * 3430 <= 8 * cap < 10 * 3431
    _, _, mask, depth, flow, _ = N.k9_case(w, h, w * h, "alternating")
    im = _upload(ctx, mask, depth, flow)
    q = np.arange(3431) % (w * h)
    kx = (q % w + 0.25).astype(np.float32); ky = (q // w + 0.5).astype(np.float32)
    for sampled in (False, True):
        exp = N.static_filter(kx[:3430], ky[:3430], mask, depth, flow, TH_DEPTH_BG, sampled)
        _same_bits(exp, oracle_static_filter(oracle, kx[:3430], ky[:3430], mask, depth, flow, TH_DEPTH_BG, sampled), K9_KEYS, "oracle")
        assert exp["keep_idx"].size == 1715
        _same_bits(im.static_filter(kx[:3430], ky[:3430], TH_DEPTH_BG, sampled=sampled), exp, K9_KEYS, f"n=3430 sampled={sampled}")
        with pytest.raises(K.VdoError, match="staging"):
            im.static_filter(kx, ky, TH_DEPTH_BG, sampled=sampled)
        with pytest.raises(K.VdoError):
            im.filters(kx, ky, TH_DEPTH_BG, TH_DEPTH_OBJ, 4, sampled=sampled)
        st, _ = im.filters(kx[:3430], ky[:3430], TH_DEPTH_BG, TH_DEPTH_OBJ, 4, sampled=sampled)
        _same_bits(st, exp, K9_KEYS, f"filters n=3430 sampled={sampled}")
    im.close()
