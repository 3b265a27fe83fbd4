"""Motion segmenter: the class image of the pixels that move against the scene, from two disparity images, the flow between them and the
camera motion, and the ego-motion from the same images (``vdo_motionseg_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K


class MotionSegParamsC(C.Structure):
    _fields_ = [("K", C.c_float * 4), ("bf", C.c_float), ("disp_unit", C.c_float), ("sigma_flow", C.c_float), ("sigma_disp", C.c_float), ("chi2", C.c_float),
                ("min_disparity", C.c_float), ("vote_radius", C.c_int32), ("vote_num", C.c_int32), ("vote_den", C.c_int32), ("min_known", C.c_int32),
                ("class_value", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(K.lib(), "vdo_motionseg_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(MotionSegParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "egomotion": [vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp],
        "compute": [vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, vp, C.c_int, vp],
        "get_state": [vp, vp],
        "get_residual": [vp, vp],
        "get_samples": [vp, vp, vp, K.c_int32_p],
        "last_timing": [vp, K.c_double_p],
        "device_images": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
    })


def params(K4, bf, disp_unit, sigma_flow=0.5, sigma_disp=0.5, chi2=9.0, min_disparity=0.0, vote_radius=2, vote_num=1, vote_den=2, min_known=6,
           class_value=1) -> MotionSegParamsC:
    """The defaults of the settings file's ``Motion.*`` keys (there ``min_disparity`` defaults to Camera.bf / ThDepthBG)."""
    return MotionSegParamsC((C.c_float * 4)(*[float(v) for v in K4]), float(bf), float(disp_unit), float(sigma_flow), float(sigma_disp), float(chi2), float(min_disparity),
                            int(vote_radius), int(vote_num), int(vote_den), int(min_known), int(class_value))


class MotionSegmenter(K.StageHandle):
    """``vdo_motionseg`` handle for width x height images; every device buffer is allocated here."""
    _prefix = "vdo_motionseg_"

    def __init__(self, ctx, width, height, K4, bf, disp_unit, **prm):
        super().__init__(_lib())
        self.width, self.height = int(width), int(height)
        self.params = params(K4, bf, disp_unit, **prm)
        self._ctx = ctx
        K.check(self._L.vdo_motionseg_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def egomotion_raw(self, disp0_ptr, disp0_stride, flow_ptr, flow_stride, valid_ptr, valid_stride, src_is_device, step=16, max_iterations=500, threshold=1.0,
                      confidence=0.98, min_inliers=50):
        """The C entry as it is, on addresses (valid_ptr may be 0 / None); returns (T float32 [4, 4], (n_samples, n_inliers, iterations_run))."""
        T = np.zeros(16, np.float32)
        out = (C.c_int32 * 3)()
        K.check(self._L.vdo_motionseg_egomotion(self._h, C.c_void_p(disp0_ptr or None), int(disp0_stride), C.c_void_p(flow_ptr or None), int(flow_stride),
                                                C.c_void_p(valid_ptr or None), int(valid_stride), int(bool(src_is_device)), int(step), int(max_iterations), float(threshold),
                                                float(confidence), int(min_inliers), T.ctypes.data, out))
        return T.reshape(4, 4), (out[0], out[1], out[2])

    def _sources(self, disp0, flow, flow_valid):
        H, W = self.height, self.width
        keep = [K.rows(disp0, "disp0", np.float32, (H, W), 4), K.rows(flow, "flow", np.float32, (H, W, 2), 4)]
        keep.append(K.rows(flow_valid, "flow_valid", np.uint8, (H, W), 1) if flow_valid is not None else (None, None, 0))
        return keep

    def egomotion(self, disp0, flow, flow_valid=None, **kw):
        """Host images (disp0 float32 [height, width], flow float32 [height, width, 2], flow_valid uint8 [height, width] or None; row strides are
        honoured) -> (T, (n_samples, n_inliers, iterations_run))."""
        (d0, p0, s0), (fl, pf, sf), (fv, pv, sv) = self._sources(disp0, flow, flow_valid)
        return self.egomotion_raw(p0, s0, pf, sf, pv, sv, False, **kw)

    def compute_raw(self, disp0_ptr, disp0_stride, disp1_ptr, disp1_stride, flow_ptr, flow_stride, valid_ptr, valid_stride, src_is_device, T, cls_ptr, out_is_device):
        """The C entry as it is, on addresses; returns (n_moving, n_static, n_unknown)."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = (C.c_int32 * 3)()
        K.check(self._L.vdo_motionseg_compute(self._h, C.c_void_p(disp0_ptr or None), int(disp0_stride), C.c_void_p(disp1_ptr or None), int(disp1_stride),
                                              C.c_void_p(flow_ptr or None), int(flow_stride), C.c_void_p(valid_ptr or None), int(valid_stride), int(bool(src_is_device)),
                                              T.ctypes.data, C.c_void_p(cls_ptr or None), int(bool(out_is_device)), out))
        return out[0], out[1], out[2]

    def compute(self, disp0, disp1, flow, flow_valid, T):
        """Host images -> (cls uint8 [height, width], (n_moving, n_static, n_unknown))."""
        (d0, p0, s0), (fl, pf, sf), (fv, pv, sv) = self._sources(disp0, flow, flow_valid)
        d1, p1, s1 = K.rows(disp1, "disp1", np.float32, (self.height, self.width), 4)
        cls = np.zeros((self.height, self.width), np.uint8)
        return cls, self.compute_raw(p0, s0, p1, s1, pf, sf, pv, sv, False, T, cls.ctypes.data, False)

    def state(self):
        """uint8 [height, width] of the last compute: 0 static, 1 moving, 2 unknown"""
        out = np.zeros((self.height, self.width), np.uint8)
        K.check(self._L.vdo_motionseg_get_state(self._h, out.ctypes.data))
        return out

    def residual(self):
        """float32 [height, width] of the last compute: e, or -1 where the pixel is unknown"""
        out = np.zeros((self.height, self.width), np.float32)
        K.check(self._L.vdo_motionseg_get_residual(self._h, out.ctypes.data))
        return out

    def samples(self):
        """(X float64 [n, 3], uv float64 [n, 2]) of the last ego-motion"""
        n = C.c_int32()
        K.check(self._L.vdo_motionseg_get_samples(self._h, None, None, C.byref(n)))
        X = np.zeros((n.value, 3)); uv = np.zeros((n.value, 2))
        K.check(self._L.vdo_motionseg_get_samples(self._h, X.ctypes.data, uv.ctypes.data, C.byref(n)))
        return X, uv

    def device_images(self):
        """Addresses of the handle's own device images: (disp1, next_right, cls)"""
        p = [C.c_void_p() for _ in range(3)]
        K.check(self._L.vdo_motionseg_device_images(self._h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)


def compute(ctx, disp0, disp1, flow, flow_valid, T, K4, bf, disp_unit, **prm):
    """One frame through a segmenter made for it: (cls, (n_moving, n_static, n_unknown))."""
    disp0 = np.asarray(disp0)
    m = MotionSegmenter(ctx, disp0.shape[1], disp0.shape[0], K4, bf, disp_unit, **prm)
    try:
        return m.compute(disp0, disp1, flow, flow_valid, T)
    finally:
        m.close()
