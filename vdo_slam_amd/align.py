"""Aligner: point-to-plane ICP of a depth frame against a view of the dense map (``vdo_align_*`` of libvdo_hip.so; semantics in
include/vdo_slam_hip.h, "Aligner").  ``step`` is host code and needs no device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import raycast as _raycast


class AlignParamsC(C.Structure):
    _fields_ = [("K", C.c_float * 4), ("min_depth", C.c_float), ("max_depth", C.c_float), ("max_dist", C.c_float), ("subsample", C.c_int32), ("min_pixels", C.c_int32),
                ("max_iterations", C.c_int32), ("eps", C.c_float), ("keep_rows", C.c_int32)]


class AlignReportC(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("used", C.c_int64), ("rms_first", C.c_double), ("rms_last", C.c_double), ("xi", C.c_double * 6)]


TRACE_ROW = 16 + 28 + 5
def _lib():
    vp, i64 = C.c_void_p, C.c_int64
    return K.declare(_raycast._lib(), "vdo_align_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(AlignParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "set_model": [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int],
        "set_model_from_view": [vp, vp, vp, vp],
        "linearise": [vp, vp, i64, vp, i64, C.c_int, vp, vp, vp],
        "linearise_frame": [vp, vp, vp, vp, vp],
        "step": [vp, i64, i64, vp, vp, vp, vp],
        "solve": [vp, vp, i64, vp, i64, C.c_int, vp, vp, vp, vp],
        "solve_frame": [vp, vp, vp, vp, vp, vp],
        "get_rows": [vp, vp],
        "last_timing": [vp, K.c_double_p],
    })


def params(K4, min_depth=0.0, max_depth=40.0, max_dist=0.4, subsample=1, min_pixels=6, max_iterations=10, eps=1e-5, keep_rows=False) -> AlignParamsC:
    return AlignParamsC((C.c_float * 4)(*[float(v) for v in K4]), float(min_depth), float(max_depth), float(max_dist), int(subsample), int(min_pixels), int(max_iterations), float(eps),
                        int(keep_rows))


def _T16(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))


def step(sums, used, min_pixels, T):
    """``vdo_align_step``: -> (status, T' float32 [4, 4], xi float64 [6], rms)"""
    L = _lib()
    s = np.ascontiguousarray(np.asarray(sums, np.float64).reshape(28)); T = _T16(T)
    out = np.zeros(16, np.float32); xi = np.zeros(6, np.float64); rms = C.c_double()
    status = L.vdo_align_step(s.ctypes.data, int(used), int(min_pixels), T.ctypes.data, out.ctypes.data, xi.ctypes.data, C.addressof(rms))
    if status < 0:
        K.check(status)
    return status, out.reshape(4, 4), xi, rms.value


def _report(r):
    return dict(iterations=r.iterations, status=r.status, used=r.used, rms_first=r.rms_first, rms_last=r.rms_last, xi=np.array(list(r.xi), np.float64))


class Aligner(K.StageHandle):
    """``vdo_align`` handle for width x height frames with intrinsics K4 = (fx, fy, cx, cy).  Every device buffer is allocated here."""
    _prefix = "vdo_align_"

    def __init__(self, ctx, width, height, K4, **prm):
        super().__init__(_lib())
        self._ctx = ctx
        self._model = None                                      # what a borrowed or rendered model needs kept alive
        self.width, self.height = int(width), int(height)
        self.params = params(K4, **prm)
        s = self.params.subsample
        self.grid = (-(-self.height // s), -(-self.width // s)) if 1 <= s <= 8 else (0, 0)      # (Hs, Ws)
        K.check(self._L.vdo_align_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def set_model(self, depth, grad, Km, Tm):
        """Host images (depth float32 [Hm, Wm], grad float32 [Hm, Wm, 3]), copied"""
        d = np.ascontiguousarray(depth, np.float32); g = np.ascontiguousarray(grad, np.float32)
        if d.ndim != 2 or g.shape != d.shape + (3,):
            raise ValueError(f"model: depth {d.shape}, grad {g.shape}")
        Km = np.ascontiguousarray(Km, np.float32); Tm = _T16(Tm)
        K.check(self._L.vdo_align_set_model(self._h, d.ctypes.data, g.ctypes.data, d.shape[1], d.shape[0], Km.ctypes.data, Tm.ctypes.data, 0))
        self._model = None

    def set_model_device(self, depth_ptr, grad_ptr, Wm, Hm, Km, Tm, keep=None):
        """Packed device images (addresses), BORROWED until the next set_model; ``keep``: whatever owns them"""
        Km = np.ascontiguousarray(Km, np.float32); Tm = _T16(Tm)
        K.check(self._L.vdo_align_set_model(self._h, C.c_void_p(depth_ptr or None), C.c_void_p(grad_ptr or None), int(Wm), int(Hm), Km.ctypes.data, Tm.ctypes.data, 1))
        self._model = keep

    def set_model_from_view(self, view, Tm):
        """Renders ``view`` (a ``raycast.Raycaster``) at Tm into the handle's model images; returns the render's counts"""
        out = (C.c_int64 * 3)()
        K.check(self._L.vdo_align_set_model_from_view(self._h, view._h, _T16(Tm).ctypes.data, out))
        self._model = view
        return out[0], out[1], out[2]

    def linearise_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, T):
        """The C entry as it is, on addresses; -> (sums float64 [28], counts int64 [5])"""
        sums = np.zeros(28, np.float64); counts = np.zeros(5, np.int64)
        K.check(self._L.vdo_align_linearise(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)),
                                            _T16(T).ctypes.data, sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def linearise(self, depth, mask, T):
        """Host images (row strides are honoured); -> (sums, counts: used, no depth, masked, no model, far)"""
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width)) if mask is not None else (None, None, 0)
        return self.linearise_raw(pd, sd, pm, sm, False, T)

    def linearise_frame(self, frame_handle, T):
        sums = np.zeros(28, np.float64); counts = np.zeros(5, np.int64)
        fh = frame_handle if isinstance(frame_handle, C.c_void_p) else C.c_void_p(frame_handle or None)
        K.check(self._L.vdo_align_linearise_frame(self._h, fh, _T16(T).ctypes.data, sums.ctypes.data, counts.ctypes.data))
        return sums, counts

    def _trace(self):
        return np.zeros((self.params.max_iterations, TRACE_ROW), np.float64)

    def solve_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, T_init):
        """-> (T float32 [4, 4], report dict, trace float64 [iterations, 49])"""
        out = np.zeros(16, np.float32); rep = AlignReportC(); trace = self._trace()
        K.check(self._L.vdo_align_solve(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)),
                                        _T16(T_init).ctypes.data, out.ctypes.data, C.addressof(rep), trace.ctypes.data))
        return out.reshape(4, 4), _report(rep), trace[:rep.iterations]

    def solve(self, depth, mask, T_init):
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width)) if mask is not None else (None, None, 0)
        return self.solve_raw(pd, sd, pm, sm, False, T_init)

    def solve_frame(self, frame_handle, T_init):
        out = np.zeros(16, np.float32); rep = AlignReportC(); trace = self._trace()
        fh = frame_handle if isinstance(frame_handle, C.c_void_p) else C.c_void_p(frame_handle or None)
        K.check(self._L.vdo_align_solve_frame(self._h, fh, _T16(T_init).ctypes.data, out.ctypes.data, C.addressof(rep), trace.ctypes.data))
        return out.reshape(4, 4), _report(rep), trace[:rep.iterations]

    def rows(self):
        """With keep_rows: float32 [Hs, Ws, 8] of the last linearisation - J (6), e, w"""
        r = np.zeros(self.grid + (8,), np.float32)
        K.check(self._L.vdo_align_get_rows(self._h, r.ctypes.data))
        return r

    def close(self):
        super().close()
        self._model = None
