"""Raycaster: depth, gradient and weight views of a dense mapper's TSDF volume (``vdo_raycast_*`` of libvdo_hip.so; semantics in
include/vdo_slam_hip.h, "Raycaster").  A ``Raycaster`` borrows its ``DenseMapper``: close the views before the mapper."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import dense as _dense


class RaycastParamsC(C.Structure):
    _fields_ = [("K", C.c_float * 4), ("near", C.c_float), ("step", C.c_float), ("n_steps", C.c_int32), ("min_weight", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(_dense._lib(), "vdo_raycast_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(RaycastParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "render": [vp, vp, vp, vp, vp, C.c_int, vp],
        "set_skip": [vp, C.c_int],
        "last_timing": [vp, K.c_double_p],
        "grid_timing": [vp, K.c_double_p],
    })


def params(K4, near, step, n_steps, min_weight=2) -> RaycastParamsC:
    return RaycastParamsC((C.c_float * 4)(*[float(v) for v in K4]), float(near), float(step), int(n_steps), int(min_weight))


class Raycaster(K.StageHandle):
    """``vdo_raycast`` handle: a width x height view of ``mapper`` (a ``dense.DenseMapper``) with intrinsics K4 = (fx, fy, cx, cy); sample k of a ray
    lies at z-depth ``near + k * step``, k < n_steps.  Every device buffer of the view is allocated here."""
    _prefix = "vdo_raycast_"

    def __init__(self, mapper, width, height, K4, near, step, n_steps, min_weight=2):
        super().__init__(_lib())
        self._mapper = mapper                                   # the view borrows the map: keep it alive
        self.width, self.height = int(width), int(height)
        self.params = params(K4, near, step, n_steps, min_weight)
        K.check(self._L.vdo_raycast_create(mapper._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def render_raw(self, T, depth_ptr, grad_ptr, weight_ptr, out_is_device):
        """The C entry as it is, on addresses (each may be 0 / None); returns (hit, missed, no valid sample)."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = (C.c_int64 * 3)()
        K.check(self._L.vdo_raycast_render(self._h, T.ctypes.data, C.c_void_p(depth_ptr or None), C.c_void_p(grad_ptr or None), C.c_void_p(weight_ptr or None),
                                           int(bool(out_is_device)), out))
        return out[0], out[1], out[2]

    def render(self, T):
        """-> (depth float32 [H, W], grad float32 [H, W, 3], weight int32 [H, W], counts)"""
        H, W = self.height, self.width
        depth = np.zeros((H, W), np.float32); grad = np.zeros((H, W, 3), np.float32); weight = np.zeros((H, W), np.int32)
        counts = self.render_raw(T, depth.ctypes.data, grad.ctypes.data, weight.ctypes.data, False)
        return depth, grad, weight, counts

    def render_device(self, T, depth_ptr=None, grad_ptr=None, weight_ptr=None):
        """Into packed device images the caller owns (addresses; each may be None); returns the counts."""
        return self.render_raw(T, depth_ptr, grad_ptr, weight_ptr, True)

    def set_skip(self, on):
        K.check(self._L.vdo_raycast_set_skip(self._h, int(bool(on))))

    def timing(self):
        """(wall ms of the call, device ms by events, device ms of the occupancy-grid build) of the last render"""
        ms = super().timing()
        g = C.c_double()
        K.check(self._L.vdo_raycast_grid_timing(self._h, C.byref(g)))
        return ms[0], ms[1], g.value

    def close(self):
        super().close()
        self._mapper = None


def normals(grad):
    """The gradient image normalised in float64 and narrowed, or 0 (as DenseMapper::Render and a saved map's normals)"""
    g = np.asarray(grad, np.float64)
    n = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2])
    with np.errstate(all="ignore"):
        out = np.where(n[..., None] > 0, g / n[..., None], 0.0)
    return out.astype(np.float32)
