"""Stereo rectifier: lens undistortion and rectification of raw 8-bit images by a fixed-point map (``vdo_rectify_*`` of libvdo_hip.so; semantics
in include/vdo_slam_hip.h).  The map planner ``plan`` is host code and needs no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


class RectifyCameraC(C.Structure):
    _fields_ = [("K", C.c_double * 4), ("D", C.c_double * 5), ("R", C.c_double * 9), ("src_width", C.c_int32), ("src_height", C.c_int32)]


class RectifyParamsC(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("P", C.c_double * 4), ("cam", RectifyCameraC * 2)]


class RectifyJobC(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_int64), ("channels", C.c_int32), ("rgb_order", C.c_int32), ("cam", C.c_int32),
                ("nearest", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int64)]


def _lib():
    vp = C.c_void_p
    return K.declare(K.lib(), "vdo_rectify_", {
        "plan": [C.POINTER(RectifyParamsC), C.c_int, vp, vp, K.c_int32_p],
        "create": [vp, C.POINTER(RectifyParamsC), C.POINTER(vp)],
        "create_from_maps": [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), K.c_int32_p, K.c_int32_p, C.POINTER(vp)],
        "destroy": [vp],
        "compute": [vp, C.POINTER(RectifyJobC), C.c_int, C.c_int, C.c_int, C.c_int],
        "gate": [vp, C.c_int, vp, C.c_int64, C.c_int, K.c_int32_p],
        "get_map": [vp, C.c_int, vp],
        "get_valid": [vp, C.c_int, vp, K.c_int32_p],
        "last_timing": [vp, K.c_double_p],
        "device_images": [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)],
        "download_image": [vp, vp, C.c_int64, vp],
    })


def camera(K4, D=(0, 0, 0, 0, 0), R=(1, 0, 0, 0, 1, 0, 0, 0, 1), src_size=(0, 0)) -> dict:
    """One raw camera: K4 = (fx, fy, cx, cy), D = (k1, k2, p1, p2[, k3]), R row-major (9 values or 3 x 3), src_size = (Ws, Hs)."""
    D = [float(v) for v in D]
    if len(D) == 4:
        D.append(0.0)
    R = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
    if len(K4) != 4 or len(D) != 5 or len(R) != 9:
        raise ValueError("camera: K4 takes 4 values, D 4 or 5, R 9")
    return {"K": [float(v) for v in K4], "D": D, "R": R, "src_size": (int(src_size[0]), int(src_size[1]))}


def params(P4, size, cams) -> RectifyParamsC:
    """P4 = (fx', fy', cx', cy') of the rectified camera, size = (W, H) of the destination, cams = one or two ``camera`` dicts."""
    p = RectifyParamsC()
    p.n_cams = len(cams)
    p.width, p.height = int(size[0]), int(size[1])
    p.P = (C.c_double * 4)(*[float(v) for v in P4])
    for c, cam in enumerate(cams[:2]):
        p.cam[c].K = (C.c_double * 4)(*cam["K"])
        p.cam[c].D = (C.c_double * 5)(*cam["D"])
        p.cam[c].R = (C.c_double * 9)(*cam["R"])
        p.cam[c].src_width, p.cam[c].src_height = cam["src_size"]
    return p


def plan(prm: RectifyParamsC, cam=0):
    """The map of one camera, on the host: (map int32 [H, W, 2] = (qx, qy), valid uint8 [H, W], n_valid)."""
    L = _lib()
    W, H = max(int(prm.width), 0), max(int(prm.height), 0)
    m = np.zeros((H, W, 2), np.int32)
    v = np.zeros((H, W), np.uint8)
    n = C.c_int32()
    K.check(L.vdo_rectify_plan(C.byref(prm), int(cam), m.ctypes.data, v.ctypes.data, C.byref(n)))
    return m, v, n.value


def job(src, src_stride, channels, dst, dst_stride, cam=0, rgb_order=0, nearest=0) -> RectifyJobC:
    """A job on addresses."""
    return RectifyJobC(C.c_void_p(src or None), int(src_stride), int(channels), int(rgb_order), int(cam), int(nearest), C.c_void_p(dst or None), int(dst_stride))


class StereoRectifier(K.StageHandle):
    """``vdo_rectify`` handle; every device buffer is allocated here.  Built from ``params(...)`` or, with ``maps=``, from ready-made maps
    (a list of int32 [H, W, 2] arrays) and ``src_sizes`` (a list of (Ws, Hs))."""
    _prefix = "vdo_rectify_"

    def __init__(self, ctx, prm: RectifyParamsC = None, maps=None, src_sizes=None):
        super().__init__(_lib())
        self._ctx = ctx
        if maps is not None:
            maps = [np.ascontiguousarray(m, np.int32) for m in maps]
            H, W = maps[0].shape[:2]
            if any(m.shape != (H, W, 2) for m in maps) or len(src_sizes) != len(maps):
                raise ValueError("maps: one int32 [H, W, 2] array and one (Ws, Hs) per camera")
            ptrs = (C.c_void_p * len(maps))(*[m.ctypes.data for m in maps])
            ws = (C.c_int32 * len(maps))(*[int(s[0]) for s in src_sizes])
            hs = (C.c_int32 * len(maps))(*[int(s[1]) for s in src_sizes])
            K.check(self._L.vdo_rectify_create_from_maps(ctx._h, W, H, len(maps), ptrs, ws, hs, C.byref(self._h)))
            self.width, self.height, self.n_cams = W, H, len(maps)
            self.src_sizes = [(int(s[0]), int(s[1])) for s in src_sizes]
        else:
            K.check(self._L.vdo_rectify_create(ctx._h, C.byref(prm), C.byref(self._h)))
            self.width, self.height, self.n_cams = int(prm.width), int(prm.height), int(prm.n_cams)
            self.src_sizes = [(int(prm.cam[c].src_width), int(prm.cam[c].src_height)) for c in range(self.n_cams)]

    def compute_raw(self, jobs, src_is_device, dst_is_device, border=0):
        """The C entry as it is, on a list of ``job(...)``."""
        arr = (RectifyJobC * max(len(jobs), 1))(*jobs)
        K.check(self._L.vdo_rectify_compute(self._h, arr, len(jobs), int(bool(src_is_device)), int(bool(dst_is_device)), int(border)))

    def compute(self, images, cams=None, rgb_order=0, nearest=None, border=0):
        """Host images (uint8 [Hs, Ws] or [Hs, Ws, 3 | 4]; row strides are honoured), one job each in one call -> a list of uint8 [H, W]."""
        cams = list(cams) if cams is not None else [0] * len(images)
        nearest = list(nearest) if nearest is not None else [0] * len(images)
        keep, jobs, outs = [], [], []
        for im, cam, nn in zip(images, cams, nearest):
            im = np.asarray(im)
            ch = 1 if im.ndim == 2 else im.shape[2]
            ws, hs = self.src_sizes[cam]
            if im.dtype != np.uint8 or im.shape[:2] != (hs, ws):
                raise ValueError(f"image: {im.dtype} {im.shape}, expected uint8 {(hs, ws)} of camera {cam}")
            if im.strides[-1] != 1 or (im.ndim == 3 and im.strides[1] != ch) or im.strides[0] < ws * ch:
                im = np.ascontiguousarray(im)
            out = np.zeros((self.height, self.width), np.uint8)
            keep.append(im); outs.append(out)
            jobs.append(job(im.ctypes.data, im.strides[0], ch, out.ctypes.data, self.width, cam, rgb_order, nn))
        self.compute_raw(jobs, False, False, border)
        return outs

    def gate_raw(self, cam, image_ptr, stride_floats, is_device):
        """The C entry as it is, on an address; returns n_cleared."""
        n = C.c_int32()
        K.check(self._L.vdo_rectify_gate(self._h, int(cam), C.c_void_p(image_ptr or None), int(stride_floats), int(bool(is_device)), C.byref(n)))
        return n.value

    def gate(self, image, cam=0):
        """A host float32 [H, W] image -> (the gated copy, n_cleared)."""
        out = np.array(image, dtype=np.float32, order="C", copy=True)
        if out.shape != (self.height, self.width):
            raise ValueError(f"image: {out.shape}, expected {(self.height, self.width)}")
        return out, self.gate_raw(cam, out.ctypes.data, self.width, False)

    def map(self, cam=0):
        """int32 [H, W, 2] = (qx, qy) of one camera"""
        m = np.zeros((self.height, self.width, 2), np.int32)
        K.check(self._L.vdo_rectify_get_map(self._h, int(cam), m.ctypes.data))
        return m

    def valid(self, cam=0):
        """(uint8 [H, W] bilinear validity of one camera, its count)"""
        v = np.zeros((self.height, self.width), np.uint8)
        n = C.c_int32()
        K.check(self._L.vdo_rectify_get_valid(self._h, int(cam), v.ctypes.data, C.byref(n)))
        return v, n.value

    def device_images(self, k=0):
        """Addresses of the handle's own device images of slot k = 0..3: (source staging, destination)"""
        p = [C.c_void_p() for _ in range(2)]
        K.check(self._L.vdo_rectify_device_images(self._h, int(k), *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def download_image(self, image_ptr, stride=None):
        """A width x height uint8 image on the device -> uint8 [H, W]"""
        out = np.zeros((self.height, self.width), np.uint8)
        K.check(self._L.vdo_rectify_download_image(self._h, C.c_void_p(image_ptr or None), int(stride or self.width), out.ctypes.data))
        return out
