"""Instance labeller: connected components of a class image to the int32 mask image the frame pipeline takes, and the same engine as a
disparity speckle filter (``vdo_labels_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


class LabelParamsC(C.Structure):
    _fields_ = [("connectivity", C.c_int32), ("max_disp_diff", C.c_int32), ("min_area", C.c_int32), ("max_labels", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(K.lib(), "vdo_labels_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(LabelParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "compute": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, C.c_int, K.c_int32_p],
        "filter_speckles": [vp, vp, C.c_int, C.c_int, C.c_int, K.c_int32_p],
        "get_roots": [vp, vp],
        "get_areas": [vp, vp],
        "last_timing": [vp, K.c_double_p],
        "device_images": [vp, C.POINTER(vp), C.POINTER(vp)],
        "stage_classes": [vp, vp, C.c_int64, C.POINTER(vp)],
    })


def params(connectivity=8, max_disp_diff=512, min_area=200, max_labels=1023) -> LabelParamsC:
    """The defaults of the settings file's ``Labels.*`` keys."""
    return LabelParamsC(int(connectivity), int(max_disp_diff), int(min_area), int(max_labels))


class InstanceLabeler(K.StageHandle):
    """``vdo_labels`` handle for width x height images; every device buffer is allocated here."""
    _prefix = "vdo_labels_"

    def __init__(self, ctx, width, height, **prm):
        super().__init__(_lib())
        self.width, self.height = int(width), int(height)
        self.params = params(**prm)
        self._ctx = ctx
        K.check(self._L.vdo_labels_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def compute_raw(self, cls_ptr, cls_stride, disp_ptr, disp_stride_floats, src_is_device, mask_ptr, out_is_device):
        """The C entry as it is, on addresses (disp_ptr may be 0 / None); returns (n_labels, n_components, area_threshold)."""
        out = (C.c_int32 * 3)()
        K.check(self._L.vdo_labels_compute(self._h, C.c_void_p(cls_ptr or None), int(cls_stride), C.c_void_p(disp_ptr or None), int(disp_stride_floats),
                                           int(bool(src_is_device)), C.c_void_p(mask_ptr or None), int(bool(out_is_device)), out))
        return out[0], out[1], out[2]

    def compute(self, cls, disp=None):
        """Host images (cls uint8 [height, width], disp float32 [height, width] or None; row strides are honoured) ->
        (mask int32 [height, width], n_labels, n_components, area_threshold)."""
        cls = np.asarray(cls)
        if cls.dtype != np.uint8 or cls.shape != (self.height, self.width):
            raise ValueError(f"cls: {cls.dtype} {cls.shape}, expected uint8 {(self.height, self.width)}")
        if cls.strides[1] != 1 or cls.strides[0] < self.width:
            cls = np.ascontiguousarray(cls)
        dp, ds = None, 0
        if disp is not None:
            disp = np.asarray(disp)
            if disp.dtype != np.float32 or disp.shape != (self.height, self.width):
                raise ValueError(f"disp: {disp.dtype} {disp.shape}, expected float32 {(self.height, self.width)}")
            if disp.strides[1] != 4 or disp.strides[0] < 4 * self.width or disp.strides[0] % 4:
                disp = np.ascontiguousarray(disp)
            dp, ds = disp.ctypes.data, disp.strides[0] // 4
        mask = np.zeros((self.height, self.width), np.int32)
        n, nc, a = self.compute_raw(cls.ctypes.data, cls.strides[0], dp, ds, False, mask.ctypes.data, False)
        return mask, n, nc, a

    def filter_speckles_raw(self, disp_ptr, is_device, max_diff, max_size):
        """The C entry as it is, on an address; returns n_removed."""
        n = C.c_int32()
        K.check(self._L.vdo_labels_filter_speckles(self._h, C.c_void_p(disp_ptr or None), int(bool(is_device)), int(max_diff), int(max_size), C.byref(n)))
        return n.value

    def filter_speckles(self, disp, max_diff, max_size):
        """A host disparity image (float32 [height, width]) -> (the filtered copy, n_removed)."""
        out = np.array(disp, dtype=np.float32, order="C", copy=True)
        if out.shape != (self.height, self.width):
            raise ValueError(f"disp: {out.shape}, expected {(self.height, self.width)}")
        return out, self.filter_speckles_raw(out.ctypes.data, False, max_diff, max_size)

    def _image(self, fn):
        out = np.zeros((self.height, self.width), np.int32)
        K.check(fn(self._h, out.ctypes.data))
        return out

    def roots(self):
        """int32 [height, width] of the last compute or filter: the root (smallest raster index) of every pixel's component, or -1"""
        return self._image(self._L.vdo_labels_get_roots)

    def areas(self):
        """int32 [height, width] of the last compute or filter: the area at each root, 0 elsewhere"""
        return self._image(self._L.vdo_labels_get_areas)

    def device_images(self):
        """Addresses of the handle's own device images: (cls, mask)"""
        p = [C.c_void_p() for _ in range(2)]
        K.check(self._L.vdo_labels_device_images(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def stage_classes(self, cls):
        """Uploads a host class image (uint8 [height, width]) into the handle's device class image; returns its address"""
        cls = np.ascontiguousarray(cls, np.uint8)
        if cls.shape != (self.height, self.width):
            raise ValueError(f"cls: {cls.shape}, expected {(self.height, self.width)}")
        p = C.c_void_p()
        K.check(self._L.vdo_labels_stage_classes(self._h, cls.ctypes.data, self.width, C.byref(p)))
        return p.value


def compute(ctx, cls, disp=None, **prm):
    """One class image through a labeller made for it: (mask, n_labels, n_components, area_threshold)."""
    cls = np.asarray(cls)
    if disp is None:
        prm.setdefault("max_disp_diff", -1)
    m = InstanceLabeler(ctx, cls.shape[1], cls.shape[0], **prm)
    try:
        return m.compute(cls, disp)
    finally:
        m.close()


def filter_speckles(ctx, disp, max_diff, max_size):
    """One disparity image through a labeller made for it: (the filtered copy, n_removed)."""
    disp = np.asarray(disp)
    m = InstanceLabeler(ctx, disp.shape[1], disp.shape[0], max_disp_diff=-1)
    try:
        return m.filter_speckles(disp, max_diff, max_size)
    finally:
        m.close()
