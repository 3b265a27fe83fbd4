"""Dense optical-flow matcher: coarse-to-fine census search on the device (``vdo_optflow_*`` of libvdo_hip.so; semantics in
include/vdo_slam_hip.h).  From two 8-bit grey images to the flow image [height, width, 2] the frame pipeline takes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


class FlowParamsC(C.Structure):
    _fields_ = [("levels", C.c_int32), ("radius", C.c_int32), ("window", C.c_int32), ("median", C.c_int32),
                ("fb_max_diff", C.c_int32), ("subpixel", C.c_int32)]


def _lib():
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    return K.declare(K.lib(), "vdo_optflow_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(FlowParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "compute": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, vp, C.c_int, K.c_int32_p],
        "level_size": [vp, C.c_int, ip, ip],
        "get_pyramid": [vp, C.c_int, C.c_int, vp],
        "get_census": [vp, C.c_int, C.c_int, vp],
        "get_level_flow": [vp, C.c_int, C.c_int, vp],
        "last_timing": [vp, K.c_double_p],
        "device_images": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
    })


def params(levels=6, radius=2, window=2, median=True, fb_max_diff=1, subpixel=True) -> FlowParamsC:
    """The defaults of the settings file's ``Flow.*`` keys."""
    return FlowParamsC(int(levels), int(radius), int(window), int(median), int(fb_max_diff), int(subpixel))


class FlowMatcher(K.StageHandle):
    """``vdo_optflow`` handle for width x height images; every device buffer is allocated here."""
    _prefix = "vdo_optflow_"

    def __init__(self, ctx, width, height, **prm):
        super().__init__(_lib())
        self.width, self.height = int(width), int(height)
        self.params = params(**prm)
        self._ctx = ctx
        K.check(self._L.vdo_optflow_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def compute_raw(self, im0_ptr, stride0, im1_ptr, stride1, src_is_device, flow_ptr, valid_ptr, out_is_device):
        """The C entry as it is, on addresses (valid_ptr may be 0 / None); returns n_valid."""
        n = C.c_int32()
        K.check(self._L.vdo_optflow_compute(self._h, C.c_void_p(im0_ptr), int(stride0), C.c_void_p(im1_ptr), int(stride1), int(bool(src_is_device)),
                                            C.c_void_p(flow_ptr), C.c_void_p(valid_ptr or None), int(bool(out_is_device)), C.byref(n)))
        return n.value

    def compute(self, im0, im1):
        """Host images (uint8 [height, width]; a row stride is honoured) -> (flow float32 [height, width, 2], valid uint8 [height, width], n_valid)."""
        imgs = []
        for name, a in (("im0", im0), ("im1", im1)):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.shape != (self.height, self.width):
                raise ValueError(f"{name}: {a.dtype} {a.shape}, expected uint8 {(self.height, self.width)}")
            if a.strides[1] != 1 or a.strides[0] < self.width:
                a = np.ascontiguousarray(a)
            imgs.append(a)
        flow = np.zeros((self.height, self.width, 2), np.float32)
        valid = np.zeros((self.height, self.width), np.uint8)
        n = self.compute_raw(imgs[0].ctypes.data, imgs[0].strides[0], imgs[1].ctypes.data, imgs[1].strides[0], False, flow.ctypes.data, valid.ctypes.data, False)
        return flow, valid, n

    def level_size(self, level):
        """(width, height) of a pyramid level"""
        w, h = C.c_int(), C.c_int()
        K.check(self._L.vdo_optflow_level_size(self._h, int(level), C.byref(w), C.byref(h)))
        return w.value, h.value

    def _level(self, fn, sel, level, dtype, tail=()):
        w, h = self.level_size(level)
        out = np.zeros((h, w) + tail, dtype)
        K.check(fn(self._h, int(sel), int(level), out.ctypes.data))
        return out

    def pyramid(self, which, level):
        return self._level(self._L.vdo_optflow_get_pyramid, which, level, np.uint8)

    def census(self, which, level):
        return self._level(self._L.vdo_optflow_get_census, which, level, np.uint64)

    def level_flow(self, direction, level):
        """int32 [H_l, W_l, 2] of the forward (0) or backward (1) run, as the level below reads it"""
        return self._level(self._L.vdo_optflow_get_level_flow, direction, level, np.int32, (2,))

    def device_images(self):
        """Addresses of the handle's own device images: (im0, im1, flow, valid)"""
        p = [C.c_void_p() for _ in range(4)]
        K.check(self._L.vdo_optflow_device_images(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)


def compute(ctx, im0, im1, **prm):
    """One pair through a matcher made for it: (flow, valid, n_valid)."""
    im0 = np.asarray(im0)
    m = FlowMatcher(ctx, im0.shape[1], im0.shape[0], **prm)
    try:
        return m.compute(im0, im1)
    finally:
        m.close()
