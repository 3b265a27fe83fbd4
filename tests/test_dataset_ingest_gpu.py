"""Dataset ingest on the device (vdo_ingest_*, vdo_slam_amd/csrc/ingest.hip) against the host DatasetIO it replaces: the mask text parse
equals LoadMask on well-formed and odd byte strings, the .flo copy equals ReadOpticalFlow, the PNG un-filter + conversion equals ReadPNG
(+ vdo_rgb2gray for colour); refused inputs write nothing.  End to end, System.track_files on a sequence on disk equals System.track_rgbd
on the same files decoded by DatasetIO."""
import ctypes as C

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd import dataset_files as DF
from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
from vdo_slam_amd.ba import Context
from vdo_slam_amd.ingest import Ingest, inflate_png

pytestmark = pytest.mark.gpu
SENTINEL = -777


@pytest.fixture(scope="module")
def host():
    L = K.load_host_lib()
    L.host_io_read_flo.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_void_p]
    L.host_io_load_mask.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    L.host_io_read_png.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_mask(host, path, rows, cols):
    out = np.full((rows, cols), SENTINEL, np.int32)
    return host.host_io_load_mask(str(path).encode(), rows, cols, _p(out)), out


def _device_mask(ing, text):
    import torch
    out = torch.full((ing.height, ing.width), SENTINEL, dtype=torch.int32, device="cuda")
    try:
        ing.frame(mask_text=text, mask_out=out.data_ptr())
        rc = 0
    except K.VdoError as e:
        assert "mask" in str(e)
        rc = -1
    return rc, out.cpu().numpy()


def _check_mask(host, ing, tmp_path, text, name="m.txt"):
    path = tmp_path / name
    path.write_bytes(text)
    rc_h, ref = _host_mask(host, path, ing.height, ing.width)
    rc_d, got = _device_mask(ing, text)
    assert (rc_h == 0) == (rc_d == 0), (text[:200], rc_h, rc_d)
    if rc_h == 0:
        assert np.array_equal(got, ref), text[:200]
    else:
        assert (got == SENTINEL).all(), "a refused mask wrote into the output"
    return rc_h


def test_mask_kitti_sized_label_image_with_odd_layout(host, ctx, tmp_path):
    W, H = synth.KITTI_W, synth.KITTI_H
    rng = np.random.default_rng(1)
    lab = rng.integers(-1, 12, (H, W)).astype(np.int32)
    lines = []
    for y in range(H):
        seps = rng.choice([" ", "  ", "\t", " \t "], size=W)
        line = "".join(f"{v}{s}" for v, s in zip(lab[y].tolist(), seps))         # trailing blanks
        lines.append(line + ("\r" if y % 3 == 0 else ""))                      # CRLF lines
        if y % 50 == 7:
            lines.append(" \t\r")                                              # blank lines do not count as rows
    text = ("\n".join(lines) + "\n").encode()
    ing = Ingest(ctx, W, H)
    assert _check_mask(host, ing, tmp_path, text) == 0
    rc, got = _device_mask(ing, text)
    assert np.array_equal(got, lab)
    ing.close()


@pytest.mark.parametrize("cols_in,rows_in", [(3, 4), (9, 4), (6, 2), (6, 8), (9, 8), (3, 2)])
def test_mask_more_and_fewer_integers_and_lines(host, ctx, tmp_path, cols_in, rows_in):
    ing = Ingest(ctx, 6, 4)
    rng = np.random.default_rng(cols_in * 10 + rows_in)
    text = ("\n".join(" ".join(str(v) for v in rng.integers(0, 300, cols_in)) for _ in range(rows_in)) + "\n").encode()
    assert _check_mask(host, ing, tmp_path, text) == 0
    ing.close()


@pytest.mark.parametrize("text", [b"--5 ---5 -x7 12ab34\n", b"-5-3 x-7 7-- -\n--\n-", b"1" * 40 + b" -" + b"9" * 40 + b"\n0000000000000123456789012\n",
                                  b"12ab34 --5\n---5 -x7\n", b"", b"abc - -- x\n\n", b"-", b"7", b"\n\n\n1"])
def test_mask_traps(host, ctx, tmp_path, text):
    ing = Ingest(ctx, 5, 3)
    _check_mask(host, ing, tmp_path, text)
    ing.close()


def test_mask_random_strings(host, ctx, tmp_path):
    ing = Ingest(ctx, 5, 7)
    rng = np.random.default_rng(2024)
    alphabet = np.frombuffer(b"0123456789 -\t\r\nx", np.uint8)
    weights = np.array([3] * 10 + [4, 3, 1, 1, 2, 1], np.float64)
    refused = 0
    for k in range(600):
        n = int(rng.integers(0, 160 if k % 10 else 9000))                     # a few strings longer than one 4 KiB block of the scan
        text = alphabet[rng.choice(alphabet.size, n, p=weights / weights.sum())].tobytes()
        refused += _check_mask(host, ing, tmp_path, text) != 0
    assert 0 < refused < 600
    ing.close()


def test_flo(host, ctx, tmp_path):
    import torch
    W, H = synth.KITTI_W, synth.KITTI_H
    flow = np.random.default_rng(3).normal(0, 20, (H, W, 2)).astype(np.float32)
    blob = DF.flo_bytes(flow)
    (tmp_path / "f.flo").write_bytes(blob)
    dims = (C.c_int * 3)()
    ref = np.zeros((H, W, 2), np.float32)
    assert host.host_io_read_flo(str(tmp_path / "f.flo").encode(), dims, _p(ref)) == 0
    ing = Ingest(ctx, W, H)
    out = torch.full((H, W, 2), float(SENTINEL), device="cuda")
    ing.frame(flo=blob, flow_out=out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ref, flow)
    bad = {"magic": b"\0\0\0\0" + blob[4:], "truncated": blob[:-8], "size": DF.flo_bytes(flow[:, :-1])}
    for what, b in bad.items():
        out.fill_(float(SENTINEL))
        with pytest.raises(K.VdoError, match=r"\.flo"):
            ing.frame(flo=b, flow_out=out.data_ptr())
        assert (out == SENTINEL).all(), what
    ing.close()


FILTER_SETS = [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4), (4, 3, 1, 2, 0, 4, 4, 1)]
FORMATS = [("grey8", 1, 8), ("grey16", 1, 16), ("rgb", 3, 8), ("rgba", 4, 8)]


def _check_png(host, ctx, tmp_path, fmt, w, h, filters, seed):
    import torch
    name, ch, bd = fmt
    rng = np.random.default_rng(seed)
    hi = 65536 if bd == 16 else 256
    arr = rng.integers(0, hi, (h, w) if ch == 1 else (h, w, ch))
    arr[: h // 2] = (arr[: h // 2] // 37) * 37 if h > 1 else arr[: h // 2]         # (smooth-ish rows as well as noise)
    path = tmp_path / f"{name}_{w}x{h}.png"
    path.write_bytes(DF.png_bytes(arr, bd, filters))
    scan = inflate_png(path)
    assert scan is not None and scan[1:] == (w, h, bd, ch)
    ing = Ingest(ctx, w, h)
    dims = (C.c_int * 3)()
    if ch == 1:                                                                  # disparity path: ReadPNG(.., as_float)
        ref = np.zeros((h, w), np.float32)
        assert host.host_io_read_png(str(path).encode(), 1, dims, _p(ref)) == 0
        out = torch.full((h, w), -1.0, device="cuda")
        ing.frame(depth=scan, depth_out=out.data_ptr())
        assert np.array_equal(out.cpu().numpy(), ref), (name, w, h, filters)
    if bd == 8:                                                                  # grey path: ReadPNG (+ K2 for colour)
        img = np.zeros((h, w, ch), np.uint8)
        assert host.host_io_read_png(str(path).encode(), 0, dims, _p(img)) == 0
        for order in ((0, 1) if ch > 1 else (1,)):
            if ch == 1:
                ref = img[:, :, 0]
            else:
                ref = np.zeros((h, w), np.uint8)
                K.check(K.lib().vdo_rgb2gray(ctx._h, _p(img), C.c_int64(w * h), ch, order, _p(ref)))
            out = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
            ing.frame(color=scan, rgb_order=order, gray_out=out.data_ptr())
            assert np.array_equal(out.cpu().numpy(), ref), (name, w, h, filters, order)
    ing.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=[f[0] for f in FORMATS])
@pytest.mark.parametrize("w,h", [(1, 1), (37, 1), (1242, 1), (1, 375), (37, 375), (1242, 375)])
def test_png_against_readpng(host, ctx, tmp_path, fmt, w, h):
    sets = FILTER_SETS if w * h < 100000 else [FILTER_SETS[4], FILTER_SETS[5], FILTER_SETS[6]]
    for k, filters in enumerate(sets):
        _check_png(host, ctx, tmp_path, fmt, w, h, filters, seed=k + 17 * w + h)


def test_png_every_filter_alone_kitti_sized(host, ctx, tmp_path):
    for k, filters in enumerate(FILTER_SETS[:4]):
        _check_png(host, ctx, tmp_path, FORMATS[2], 1242, 375, filters, seed=100 + k)


def test_png_taller_than_one_band(host, ctx, tmp_path):
    _check_png(host, ctx, tmp_path, FORMATS[2], 5, 1100, FILTER_SETS[6], seed=5)
    _check_png(host, ctx, tmp_path, FORMATS[1], 3, 2100, FILTER_SETS[5], seed=6)


def test_png_refusals_write_nothing(ctx, tmp_path):
    import torch
    w, h = 37, 9
    path = tmp_path / "c.png"
    path.write_bytes(DF.png_bytes(np.random.default_rng(0).integers(0, 256, (h, w, 3)), 8, (0, 1, 2)))
    buf, *meta = inflate_png(path)
    ing = Ingest(ctx, w, h)
    out = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
    bad = buf.copy(); bad[2 * (1 + 3 * w)] = 5                                    # filter byte of row 2
    with pytest.raises(K.VdoError, match="filter type 5"):
        ing.frame(color=(bad, *meta), gray_out=out.data_ptr())
    with pytest.raises(K.VdoError, match="colour PNG"):
        ing.frame(color=(buf[:-1], *meta), gray_out=out.data_ptr())
    with pytest.raises(K.VdoError, match="colour PNG is"):
        ing.frame(color=(buf, w, h + 1, 8, 3), gray_out=out.data_ptr())
    with pytest.raises(K.VdoError, match="depth PNG"):                           # colour is not a disparity map
        dep = torch.zeros((h, w), device="cuda")
        ing.frame(depth=(buf, *meta), depth_out=dep.data_ptr())
    with pytest.raises(K.VdoError, match="mask"):                                # a mask without a row: nothing else is written either
        ing.frame(mask_text=b"x - \n\n", color=(buf, *meta), gray_out=out.data_ptr(), mask_out=torch.zeros((h, w), dtype=torch.int32, device="cuda").data_ptr())
    assert (out == 7).all()
    ing.close()


def _settings(tmp_path):
    from vdo_slam_amd.system import write_settings
    return write_settings(tmp_path / "kitti.yaml", synth.KITTI_W, synth.KITTI_H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)


def test_track_files_equals_track_rgbd_on_datasetio_images(host, tmp_path):
    from vdo_slam_amd.system import System
    W, H = synth.KITTI_W, synth.KITTI_H
    n_frames = 10
    Ts = SQ.camera_poses(n_frames)
    objs = SQ.default_objects()
    files = []
    for k in range(n_frames):
        fr = SQ.render_frame(k, Ts, objs, flow_sigma=0.1)
        g = fr["gray"].astype(np.int32)
        rgb = np.stack([g, 255 - g // 2, (g * 7) % 256], -1).astype(np.uint8)       # three different channels: the BGR swap matters
        disp = np.clip(fr["depth_raw"], 0, 65535).astype(np.uint16)                 # what a 16-bit PNG can hold: both sides read the same values
        files.append(DF.write_frame(str(tmp_path / f"{k:06d}"), rgb, disp, fr["flow"], fr["mask"]))
    rows = lambda k: np.array([[k, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in (1, 2, 3)], np.float32)
    cfg = _settings(tmp_path)

    def run(from_files):
        s = System(cfg)
        out = []
        for k, (prgb, pdep, pflo, pmask) in enumerate(files):
            if from_files:
                T = s.track_files(prgb, pdep, pflo, pmask, rows(k), n_images=n_frames)
            else:                                                                     # the driver's loop on DatasetIO's host decode
                dims = (C.c_int * 3)()
                im = np.zeros((H, W, 3), np.uint8); dep = np.zeros((H, W), np.float32)
                flo = np.zeros((H, W, 2), np.float32); msk = np.zeros((H, W), np.int32)
                assert host.host_io_read_png(prgb.encode(), 0, dims, _p(im)) == 0 and tuple(dims) == (H, W, 3)
                assert host.host_io_read_png(pdep.encode(), 1, dims, _p(dep)) == 0
                assert host.host_io_read_flo(pflo.encode(), dims, _p(flo)) == 0
                assert host.host_io_load_mask(pmask.encode(), H, W, _p(msk)) == 0
                T = s.track_rgbd(im, dep, flo, msk, rows(k), n_images=n_frames)
            assert T is not None, (from_files, k)
            d, m = s.frame_images(W, H)
            out.append(dict(T=T, motions=s.motions(), depth=d, mask=m))
        out.append(dict(refined=s.refined_poses(n_frames)))
        s.close()
        return out

    a, b = run(False), run(True)
    for k in range(n_frames):
        assert np.array_equal(a[k]["T"], b[k]["T"]), k
        assert [l for l, _ in a[k]["motions"]] == [l for l, _ in b[k]["motions"]], k
        assert all(np.array_equal(x, y) for (_, x), (_, y) in zip(a[k]["motions"], b[k]["motions"])), k
        assert np.array_equal(a[k]["depth"], b[k]["depth"]) and np.array_equal(a[k]["mask"], b[k]["mask"]), k
    assert any(a[k]["motions"] for k in range(1, n_frames))
    assert a[-1]["refined"].shape == (n_frames, 4, 4) and np.array_equal(a[-1]["refined"], b[-1]["refined"])


def test_track_files_refuses_a_missing_or_broken_file(tmp_path):
    from vdo_slam_amd.system import System
    W, H = synth.KITTI_W, synth.KITTI_H
    fr = SQ.render_frame(0, SQ.camera_poses(1), SQ.default_objects())
    p = DF.write_frame(str(tmp_path / "f"), fr["gray"], np.clip(fr["depth_raw"], 0, 65535).astype(np.uint16), fr["flow"], fr["mask"])
    s = System(_settings(tmp_path))
    assert s.track_files(p[0], p[1], p[2], str(tmp_path / "missing.txt")) is None
    (tmp_path / "short.flo").write_bytes(DF.flo_bytes(fr["flow"][:, :W // 2]))
    assert s.track_files(p[0], p[1], str(tmp_path / "short.flo"), p[3]) is None
    assert s.track_files(*p) is not None                                            # grey 8-bit colour input: ReadPNG's image is the grey image
    s.close()
