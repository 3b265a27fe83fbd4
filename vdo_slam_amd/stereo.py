"""Stereo matcher: census + semi-global matching on the device (``vdo_stereo_*`` of libvdo_hip.so; semantics in
include/vdo_slam_hip.h).  From a rectified 8-bit pair to disparity x 256 - the ``depth_raw`` image the frame pipeline takes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


class StereoParamsC(C.Structure):
    _fields_ = [("max_disparity", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("paths", C.c_int32),
                ("uniqueness", C.c_int32), ("lr_max_diff", C.c_int32), ("subpixel", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(K.lib(), "vdo_stereo_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(StereoParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "compute": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, C.c_int, K.c_int32_p],
        "set_output_scale": [vp, C.c_float],
        "get_census": [vp, C.c_int, vp],
        "get_cost": [vp, vp],
        "get_aggregated": [vp, vp],
        "last_timing": [vp, K.c_double_p],
    })


def params(max_disparity=128, p1=10, p2=120, paths=8, uniqueness=5, lr_max_diff=1, subpixel=True) -> StereoParamsC:
    """The defaults of the settings file's ``Stereo.*`` keys."""
    return StereoParamsC(int(max_disparity), int(p1), int(p2), int(paths), int(uniqueness), int(lr_max_diff), int(bool(subpixel)))


class StereoMatcher(K.StageHandle):
    """``vdo_stereo`` handle for width x height images; every device buffer is allocated here."""
    _prefix = "vdo_stereo_"

    def __init__(self, ctx, width, height, **prm):
        super().__init__(_lib())
        self.width, self.height = int(width), int(height)
        self.params = params(**prm)
        self._ctx = ctx
        K.check(self._L.vdo_stereo_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def compute_raw(self, left_ptr, left_stride, right_ptr, right_stride, src_is_device, out_ptr, out_is_device):
        """The C entry as it is, on addresses; returns n_valid."""
        n = C.c_int32()
        K.check(self._L.vdo_stereo_compute(self._h, C.c_void_p(left_ptr), int(left_stride), C.c_void_p(right_ptr), int(right_stride), int(bool(src_is_device)),
                                           C.c_void_p(out_ptr), int(bool(out_is_device)), C.byref(n)))
        return n.value

    def compute(self, left, right):
        """Host images (uint8 [height, width]; a row stride is honoured) -> (disparity256 float32 [height, width], n_valid)."""
        imgs = []
        for name, a in (("left", left), ("right", right)):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.shape != (self.height, self.width):
                raise ValueError(f"{name}: {a.dtype} {a.shape}, expected uint8 {(self.height, self.width)}")
            if a.strides[1] != 1 or a.strides[0] < self.width:
                a = np.ascontiguousarray(a)
            imgs.append(a)
        out = np.zeros((self.height, self.width), np.float32)
        n = self.compute_raw(imgs[0].ctypes.data, imgs[0].strides[0], imgs[1].ctypes.data, imgs[1].strides[0], False, out.ctypes.data, False)
        return out, n

    def set_output_scale(self, scale):
        K.check(self._L.vdo_stereo_set_output_scale(self._h, float(scale)))

    def census(self, which):
        out = np.zeros((self.height, self.width), np.uint64)
        K.check(self._L.vdo_stereo_get_census(self._h, int(which), out.ctypes.data))
        return out

    def cost(self):
        out = np.zeros((self.height, self.width, self.params.max_disparity), np.uint8)
        K.check(self._L.vdo_stereo_get_cost(self._h, out.ctypes.data))
        return out

    def aggregated(self):
        out = np.zeros((self.height, self.width, self.params.max_disparity), np.uint16)
        K.check(self._L.vdo_stereo_get_aggregated(self._h, out.ctypes.data))
        return out

    last_timing = K.StageHandle.timing      # (wall ms of the call, device ms by events) of the last compute


def compute(ctx, left, right, **prm):
    """One pair through a matcher made for it: (disparity256, n_valid)."""
    left = np.asarray(left)
    m = StereoMatcher(ctx, left.shape[1], left.shape[0], **prm)
    try:
        return m.compute(left, right)
    finally:
        m.close()
