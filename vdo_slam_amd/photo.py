"""Photometric aligner: the intensity term beside the aligner's ICP and their joint solve (``vdo_photo_*`` of libvdo_hip.so; semantics in
include/vdo_slam_hip.h, "Photometric aligner").  ``combine`` is host code and needs no device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import align as _align


class PhotoParamsC(C.Structure):
    _fields_ = [("K", C.c_float * 4), ("min_depth", C.c_float), ("max_depth", C.c_float), ("max_dist", C.c_float), ("max_diff", C.c_float), ("subsample", C.c_int32),
                ("min_pixels", C.c_int32), ("max_iterations", C.c_int32), ("eps", C.c_float), ("keep_rows", C.c_int32)]


class PhotoReportC(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("used_geo", C.c_int64), ("used_photo", C.c_int64), ("rms_geo_first", C.c_double), ("rms_geo_last", C.c_double),
                ("rms_photo_first", C.c_double), ("rms_photo_last", C.c_double), ("xi", C.c_double * 6)]


TRACE_ROW = 16 + 28 + 5 + 28 + 5


def _lib():
    vp, i64, ci, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    return K.declare(_align._lib(), "vdo_photo_", {
        "create": [vp, ci, ci, C.POINTER(PhotoParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "set_image": [vp, vp, i64, ci, ci, ci],
        "set_model": [vp, vp, vp, ci, ci, vp, vp, ci],
        "keep_as_model": [vp, vp, i64, vp, i64, ci, vp],
        "keep_as_model_frame": [vp, vp, vp],
        "get_image": [vp, vp],
        "get_model": [vp, vp, vp, vp],
        "combine": [vp, vp, dbl, vp],
        "linearise": [vp, vp, i64, vp, i64, ci, vp, vp, vp],
        "linearise_frame": [vp, vp, vp, vp, vp],
        "solve": [vp, vp, vp, i64, vp, i64, ci, dbl, vp, vp, vp, vp],
        "solve_frame": [vp, vp, vp, dbl, vp, vp, vp, vp],
        "get_rows": [vp, vp],
        "last_timing": [vp, K.c_double_p],
    })


def params(K4, min_depth=0.0, max_depth=40.0, max_dist=0.4, max_diff=255.0, subsample=1, min_pixels=6, max_iterations=10, eps=1e-5, keep_rows=False) -> PhotoParamsC:
    return PhotoParamsC((C.c_float * 4)(*[float(v) for v in K4]), float(min_depth), float(max_depth), float(max_dist), float(max_diff), int(subsample), int(min_pixels),
                        int(max_iterations), float(eps), int(keep_rows))


_T16 = _align._T16


def combine(geo, photo, weight):
    """``vdo_photo_combine``: geo (28 or None) + weight^2 * photo -> float64 [28]"""
    L = _lib()
    g = np.ascontiguousarray(np.asarray(geo, np.float64).reshape(28)) if geo is not None else None
    p = np.ascontiguousarray(np.asarray(photo, np.float64).reshape(28))
    out = np.zeros(28, np.float64)
    K.check(L.vdo_photo_combine(g.ctypes.data if g is not None else None, p.ctypes.data, float(weight), out.ctypes.data))
    return out


def _report(r):
    return dict(iterations=r.iterations, status=r.status, used_geo=r.used_geo, used_photo=r.used_photo, rms_geo_first=r.rms_geo_first, rms_geo_last=r.rms_geo_last,
                rms_photo_first=r.rms_photo_first, rms_photo_last=r.rms_photo_last, xi=np.array(list(r.xi), np.float64))


def _vp(h):
    return h if isinstance(h, C.c_void_p) else C.c_void_p(h or None)


class PhotoAligner(K.StageHandle):
    """``vdo_photo`` handle for width x height frames with intrinsics K4 = (fx, fy, cx, cy).  Every device buffer is allocated here."""
    _prefix = "vdo_photo_"

    def __init__(self, ctx, width, height, K4, **prm):
        super().__init__(_lib())
        self._ctx = ctx
        self.width, self.height = int(width), int(height)
        self.params = params(K4, **prm)
        s = self.params.subsample
        self.grid = (-(-self.height // s), -(-self.width // s)) if 1 <= s <= 8 else (0, 0)      # (Hs, Ws)
        K.check(self._L.vdo_photo_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def set_image_raw(self, image_ptr, stride_bytes, channels, rgb_order, is_device):
        K.check(self._L.vdo_photo_set_image(self._h, C.c_void_p(image_ptr or None), int(stride_bytes), int(channels), int(rgb_order), int(bool(is_device))))

    def set_image(self, image, rgb_order=0):
        """Host image uint8 [H, W] or [H, W, 1 | 3 | 4] (row strides are honoured)"""
        a = np.asarray(image)
        channels = 1 if a.ndim == 2 else a.shape[2]
        shape = (self.height, self.width) if a.ndim == 2 else (self.height, self.width, channels)
        a, p, stride = K.rows(a, "image", np.uint8, shape, unit=1)
        self.set_image_raw(p, stride, channels, rgb_order, False)

    def image(self):
        """The grey image I, float32 [H, W]"""
        g = np.zeros((self.height, self.width), np.float32)
        K.check(self._L.vdo_photo_get_image(self._h, g.ctypes.data))
        return g

    def set_model(self, depth, intensity, Km, Tm):
        """Host images float32 [Hm, Wm], copied"""
        d = np.ascontiguousarray(depth, np.float32); i = np.ascontiguousarray(intensity, np.float32)
        if d.ndim != 2 or i.shape != d.shape:
            raise ValueError(f"model: depth {d.shape}, intensity {i.shape}")
        Km = np.ascontiguousarray(Km, np.float32); Tm = _T16(Tm)
        K.check(self._L.vdo_photo_set_model(self._h, d.ctypes.data, i.ctypes.data, d.shape[1], d.shape[0], Km.ctypes.data, Tm.ctypes.data, 0))

    def set_model_device(self, depth_ptr, intensity_ptr, Wm, Hm, Km, Tm):
        """Packed device images (addresses), copied"""
        Km = np.ascontiguousarray(Km, np.float32); Tm = _T16(Tm)
        K.check(self._L.vdo_photo_set_model(self._h, C.c_void_p(depth_ptr or None), C.c_void_p(intensity_ptr or None), int(Wm), int(Hm), Km.ctypes.data, Tm.ctypes.data, 1))

    def keep_as_model_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, T):
        K.check(self._L.vdo_photo_keep_as_model(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)),
                                                _T16(T).ctypes.data))

    def keep_as_model(self, depth, mask, T):
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width)) if mask is not None else (None, None, 0)
        self.keep_as_model_raw(pd, sd, pm, sm, False, T)

    def keep_as_model_frame(self, frame_handle, T):
        K.check(self._L.vdo_photo_keep_as_model_frame(self._h, _vp(frame_handle), _T16(T).ctypes.data))

    def model(self):
        """The packed model, float32 [Hm, Wm, 2]: depth, intensity"""
        wm, hm = C.c_int(), C.c_int()
        K.check(self._L.vdo_photo_get_model(self._h, None, C.addressof(wm), C.addressof(hm)))
        pairs = np.zeros((hm.value, wm.value, 2), np.float32)
        K.check(self._L.vdo_photo_get_model(self._h, pairs.ctypes.data, None, None))
        return pairs

    def linearise_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, T):
        """The C entry as it is, on addresses; -> (sums float64 [28], counts int64 [5])"""
        sums = np.zeros(28, np.float64); counts = np.zeros(5, np.int64)
        K.check(self._L.vdo_photo_linearise(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)),
                                            _T16(T).ctypes.data, sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def linearise(self, depth, mask, T):
        """Host images (row strides are honoured); -> (sums, counts: used, no depth, masked, no model, far)"""
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width)) if mask is not None else (None, None, 0)
        return self.linearise_raw(pd, sd, pm, sm, False, T)

    def linearise_frame(self, frame_handle, T):
        sums = np.zeros(28, np.float64); counts = np.zeros(5, np.int64)
        K.check(self._L.vdo_photo_linearise_frame(self._h, _vp(frame_handle), _T16(T).ctypes.data, sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def _trace(self):
        return np.zeros((self.params.max_iterations, TRACE_ROW), np.float64)

    def solve_raw(self, geo, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, weight, T_init):
        """geo: an ``align.Aligner`` or None; -> (T float32 [4, 4], report dict, trace float64 [iterations, 82])"""
        out = np.zeros(16, np.float32); rep = PhotoReportC(); trace = self._trace()
        K.check(self._L.vdo_photo_solve(self._h, geo._h if geo is not None else None, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride),
                                        int(bool(src_is_device)), float(weight), _T16(T_init).ctypes.data, out.ctypes.data, C.addressof(rep), trace.ctypes.data))
        return out.reshape(4, 4), _report(rep), trace[:rep.iterations]

    def solve(self, geo, depth, mask, weight, T_init):
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width)) if mask is not None else (None, None, 0)
        return self.solve_raw(geo, pd, sd, pm, sm, False, weight, T_init)

    def solve_frame(self, geo, frame_handle, weight, T_init):
        out = np.zeros(16, np.float32); rep = PhotoReportC(); trace = self._trace()
        K.check(self._L.vdo_photo_solve_frame(self._h, geo._h if geo is not None else None, _vp(frame_handle), float(weight), _T16(T_init).ctypes.data, out.ctypes.data,
                                              C.addressof(rep), trace.ctypes.data))
        return out.reshape(4, 4), _report(rep), trace[:rep.iterations]

    def rows(self):
        """With keep_rows: float32 [Hs, Ws, 8] of the last linearisation - J (6), e, w"""
        r = np.zeros(self.grid + (8,), np.float32)
        K.check(self._L.vdo_photo_get_rows(self._h, r.ctypes.data))
        return r
