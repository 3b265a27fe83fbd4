"""Dense mapper: a TSDF voxel volume of the static scene on the device, fused from a frame's metric depth, instance mask and pose, and the surface
points extracted from it (``vdo_dense_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h).  ``FollowingMap`` is the per-frame flow of
``System`` (host/DenseMapper.cc) on top of it: the volume follows the camera, what leaves it is kept as points."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi as K


class DenseParamsC(C.Structure):
    _fields_ = [("n", C.c_int32 * 3), ("voxel", C.c_float), ("origin", C.c_int32 * 3), ("K", C.c_float * 4), ("trunc", C.c_float), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("max_weight", C.c_int32), ("stage_points", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(K.lib(), "vdo_dense_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(DenseParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "integrate": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, vp],
        "integrate_frame": [vp, vp, vp, vp],
        "recenter": [vp, vp],
        "extract": [vp, vp, vp, C.c_int, C.c_int64, vp, vp, vp, C.c_int, vp],
        "get_volume": [vp, vp, vp],
        "set_volume": [vp, vp],
        "last_timing": [vp, K.c_double_p],
        "device_volume": [vp, C.POINTER(vp)],
        "set_voxels_per_thread": [vp, C.c_int],
        "clear": [vp],
    })


def params(n, voxel, K4, origin=(0, 0, 0), trunc=None, min_depth=0.0, max_depth=40.0, max_weight=64, stage_points=1 << 20) -> DenseParamsC:
    """The defaults of the settings file's ``Dense.*`` keys (there ``max_depth`` defaults to ThDepthBG)."""
    trunc = 4.0 * float(np.float32(voxel)) if trunc is None else trunc
    return DenseParamsC((C.c_int32 * 3)(*[int(v) for v in n]), float(voxel), (C.c_int32 * 3)(*[int(v) for v in origin]), (C.c_float * 4)(*[float(v) for v in K4]), float(trunc),
                        float(min_depth), float(max_depth), int(max_weight), int(stage_points))


class DenseMapper(K.StageHandle):
    """``vdo_dense`` handle for an nx x ny x nz volume and width x height images; every device buffer is allocated here."""
    _prefix = "vdo_dense_"

    def __init__(self, ctx, width, height, n, voxel, K4, **prm):
        super().__init__(_lib())
        self.width, self.height = int(width), int(height)
        self.params = params(n, voxel, K4, **prm)
        self.n = tuple(self.params.n)
        self._ctx = ctx
        K.check(self._L.vdo_dense_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def integrate_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, T):
        """The C entry as it is, on addresses (mask_ptr may be 0 / None); returns (updated, masked, occluded)."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = (C.c_int64 * 3)()
        K.check(self._L.vdo_dense_integrate(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)),
                                            T.ctypes.data, out))
        return out[0], out[1], out[2]

    def integrate(self, depth, mask, T):
        """Host images (depth float32 [height, width] in metres, mask int32 [height, width] or None; row strides are honoured), T world -> camera."""
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width)) if mask is not None else (None, None, 0)
        return self.integrate_raw(pd, sd, pm, sm, False, T)

    def integrate_frame(self, frame_handle, T):
        """From the resident depth and mask of a ``vdo_frame_images`` (its address)."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = (C.c_int64 * 3)()
        fh = frame_handle if isinstance(frame_handle, C.c_void_p) else C.c_void_p(frame_handle or None)
        K.check(self._L.vdo_dense_integrate_frame(self._h, fh, T.ctypes.data, out))
        return out[0], out[1], out[2]

    def recenter(self, new_origin):
        o = (C.c_int32 * 3)(*[int(v) for v in new_origin])
        K.check(self._L.vdo_dense_recenter(self._h, o))

    def count(self, lo, hi, min_weight=2):
        return self.extract(lo, hi, min_weight, capacity=0)[3]

    def extract(self, lo, hi, min_weight=2, capacity=None):
        """-> (xyz float32 [m, 3], grad int32 [m, 3], weight int32 [m], count); capacity None: all of them."""
        clo = (C.c_int32 * 3)(*[int(v) for v in lo]); chi = (C.c_int32 * 3)(*[int(v) for v in hi])
        n = C.c_int64()
        if capacity is None:
            K.check(self._L.vdo_dense_extract(self._h, clo, chi, int(min_weight), 0, None, None, None, 0, C.byref(n)))
            capacity = n.value
        xyz = np.zeros((capacity, 3), np.float32); grad = np.zeros((capacity, 3), np.int32); wgt = np.zeros(capacity, np.int32)
        K.check(self._L.vdo_dense_extract(self._h, clo, chi, int(min_weight), int(capacity), xyz.ctypes.data if capacity else None, grad.ctypes.data if capacity else None,
                                          wgt.ctypes.data if capacity else None, 0, C.byref(n)))
        m = min(capacity, n.value)
        return xyz[:m], grad[:m], wgt[:m], n.value

    def extract_all(self, min_weight=2):
        o = self.origin()
        return self.extract(o, [o[a] + self.n[a] for a in range(3)], min_weight)

    def volume(self):
        """(words uint32 [nz, ny, nx] in slot order, origin (x, y, z))"""
        w = np.zeros(self.n[::-1], np.uint32)
        o = (C.c_int32 * 3)()
        K.check(self._L.vdo_dense_get_volume(self._h, w.ctypes.data, o))
        return w, (o[0], o[1], o[2])

    def set_volume(self, words):
        """Replace the words (uint32 [nz, ny, nx] in slot order): a saved volume, or one made by hand"""
        w = np.ascontiguousarray(words, np.uint32)
        if w.shape != self.n[::-1]:
            raise ValueError(f"words: {w.shape}, expected {self.n[::-1]}")
        K.check(self._L.vdo_dense_set_volume(self._h, w.ctypes.data))

    def clear(self):
        """Every word 0, the origin kept: a retired volume is reused"""
        K.check(self._L.vdo_dense_clear(self._h))

    def origin(self):
        o = (C.c_int32 * 3)()
        K.check(self._L.vdo_dense_get_volume(self._h, None, o))
        return (o[0], o[1], o[2])

    def device_volume(self):
        p = C.c_void_p()
        K.check(self._L.vdo_dense_device_volume(self._h, C.byref(p)))
        return p.value

    def set_voxels_per_thread(self, v):
        K.check(self._L.vdo_dense_set_voxels_per_thread(self._h, int(v)))


def camera_voxel(Tcw, voxel):
    """The global voxel of the camera centre -R^T t of a world -> camera pose, in float64 (as host/DenseMapper.cc)"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    v = float(np.float32(voxel))
    return [int(math.floor(-(T[0, a] * T[0, 3] + T[1, a] * T[1, 3] + T[2, a] * T[2, 3]) / v)) for a in range(3)]


def leaving_boxes(origin, new_origin, n):
    """The disjoint boxes [lo, hi) of global voxels that leave a volume moved from origin to new_origin, x slab first, then y, then z (the slab of an
    axis is cut to what stays on the axes before it).  A move of n or more on an axis: the whole volume, one box."""
    o, q = list(origin), list(new_origin)
    if any(abs(q[a] - o[a]) >= n[a] for a in range(3)):
        return [(o, [o[a] + n[a] for a in range(3)])]
    boxes = []
    lo, hi = list(o), [o[a] + n[a] for a in range(3)]
    for a in range(3):
        d = q[a] - o[a]
        if d == 0:
            continue
        blo, bhi = list(lo), list(hi)
        if d > 0:
            bhi[a] = o[a] + d; lo[a] = o[a] + d
        else:
            blo[a] = o[a] + n[a] + d; hi[a] = o[a] + n[a] + d
        boxes.append((blo, bhi))
    return boxes


class FollowingMap:
    """The per-frame flow of ``System`` with ``Dense.*`` keys: before a frame is fused, the volume is moved when the camera centre's voxel is further
    than ``margin`` voxels from its target place ``floor(anchor * n)``; what leaves is extracted first and kept as points."""

    def __init__(self, ctx, width, height, n, voxel, K4, anchor=(0.5, 0.5, 0.25), margin=None, min_weight=2, **prm):
        self.n = tuple(int(v) for v in n)
        self.voxel = float(np.float32(voxel))
        self.target = [int(math.floor(float(anchor[a]) * self.n[a])) for a in range(3)]
        self.margin = min(self.n) // 8 if margin is None else int(margin)
        self.min_weight = int(min_weight)
        self.mapper = DenseMapper(ctx, width, height, n, voxel, K4, **prm)
        self.started = False
        self.recenters = 0
        self.xyz, self.grad, self.wgt = [], [], []

    def _before_move(self, origin, new_origin):
        """Called once before every move of a started volume, the volume still at ``origin`` (mesh.FollowingMesh keeps its seam quads here)"""

    def _keep(self, lo, hi):
        xyz, grad, wgt, _ = self.mapper.extract(lo, hi, self.min_weight)
        self.xyz.append(xyz); self.grad.append(grad); self.wgt.append(wgt)

    def fuse(self, depth, mask, Tcw):
        c = camera_voxel(Tcw, self.voxel)
        o = self.mapper.origin()
        want = [c[a] - self.target[a] for a in range(3)]
        if not self.started or any(abs(c[a] - (o[a] + self.target[a])) > self.margin for a in range(3)):
            if self.started:
                self._before_move(o, want)
                for lo, hi in leaving_boxes(o, want, self.n):
                    self._keep(lo, hi)
                self.recenters += 1
            self.mapper.recenter(want)
            self.started = True
        return self.mapper.integrate(depth, mask, Tcw)

    def points(self):
        """Everything kept so far and what is in the volume now: (xyz, normals float32 [m, 3], weight int32 [m]) - what System.save_dense_map writes"""
        xyz, grad, wgt, _ = self.mapper.extract_all(self.min_weight)
        X = np.concatenate(self.xyz + [xyz]); G = np.concatenate(self.grad + [grad]).astype(np.float64); Wt = np.concatenate(self.wgt + [wgt])
        nrm = np.sqrt(G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1] + G[:, 2] * G[:, 2])
        with np.errstate(all="ignore"):
            N = np.where(nrm[:, None] > 0, G / nrm[:, None], 0.0).astype(np.float32)
        return X, N, Wt

    def close(self):
        self.mapper.close()


PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("weight", "<i4")])


def read_ply(path):
    """The binary little-endian PLY System.save_dense_map writes -> (xyz float32 [m, 3], normals float32 [m, 3], weight int32 [m])"""
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            if line.startswith(b"element vertex"):
                n = int(line.split()[2])
            if line.strip() == b"end_header":
                break
        a = np.frombuffer(f.read(), PLY_DTYPE, n)
    return (np.stack([a["x"], a["y"], a["z"]], -1), np.stack([a["nx"], a["ny"], a["nz"]], -1), a["weight"].copy())
