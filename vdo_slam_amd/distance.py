"""Distance field: the exact squared Euclidean distance, in voxels, from the voxels of a box of a dense mapper's TSDF volume to the nearest voxel at
a zero crossing, with the voxel's state (``vdo_distance_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h, "Distance field").  One
``DistanceField`` serves every ``DenseMapper`` of its context - the static map and the object volumes - for boxes of no more voxels than it was made
for, and keeps the last field as a snapshot that world points are looked up in."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import dense as _dense

FAR = 0x0FFFFFFF            # d2 of a voxel with no site of the box within the radius
OUTSIDE = 0xFFFFFFFF        # the word of a sampled point outside the snapshot's box
WINDOW = 262144             # VDO_DISTANCE_WINDOW: host points per window of a sample
UNKNOWN, FREE, INSIDE = 0, 1, 2


class DistanceParamsC(C.Structure):
    _fields_ = [("n", C.c_int32 * 3)]


def _lib():
    vp = C.c_void_p
    return K.declare(_dense._lib(), "vdo_distance_", {
        "create": [vp, C.POINTER(DistanceParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "compute": [vp, vp, vp, vp, C.c_int, C.c_int, vp],
        "get": [vp, vp, C.c_int, vp, vp],
        "sample": [vp, C.c_int64, vp, vp, C.c_int, vp],
        "device_field": [vp, C.POINTER(vp)],
        "set_method": [vp, C.c_int],
        "last_timing": [vp, K.c_double_p],
    })


class DistanceField(K.StageHandle):
    """``vdo_distance`` handle for boxes of up to nx * ny * nz voxels; every device buffer is allocated here."""
    _prefix = "vdo_distance_"

    def __init__(self, ctx, n):
        super().__init__(_lib())
        self._ctx = ctx
        self.params = DistanceParamsC((C.c_int32 * 3)(*[int(v) for v in n]))
        K.check(self._L.vdo_distance_create(ctx._h, C.byref(self.params), C.byref(self._h)))

    def compute(self, mapper, lo, hi, min_weight=2, radius=40):
        """The field of the box [lo, hi) (global voxels, clipped to the volume) becomes the snapshot -> (sites, voxels within the radius, voxels)"""
        clo = (C.c_int32 * 3)(*[int(v) for v in lo]); chi = (C.c_int32 * 3)(*[int(v) for v in hi])
        counts = (C.c_int64 * 3)()
        K.check(self._L.vdo_distance_compute(self._h, mapper._h, clo, chi, int(min_weight), int(radius), counts))
        return counts[0], counts[1], counts[2]

    def compute_all(self, mapper, min_weight=2, radius=40):
        o = mapper.origin()
        return self.compute(mapper, o, [o[a] + mapper.n[a] for a in range(3)], min_weight, radius)

    def box(self):
        """(lo, hi) of the snapshot, global voxels"""
        lo = (C.c_int32 * 3)(); hi = (C.c_int32 * 3)()
        K.check(self._L.vdo_distance_get(self._h, None, 0, lo, hi))
        return tuple(lo), tuple(hi)

    def field(self):
        """-> (words uint32 [bz, by, bx], lo, hi)"""
        lo, hi = self.box()
        words = np.zeros([hi[a] - lo[a] for a in (2, 1, 0)], np.uint32)
        K.check(self._L.vdo_distance_get(self._h, words.ctypes.data if words.size else None, 0, None, None))
        return words, lo, hi

    def field_to_device(self, ptr):
        """Copies the snapshot's words to device memory at ``ptr``"""
        K.check(self._L.vdo_distance_get(self._h, C.c_void_p(ptr), 1, None, None))

    def device_field(self):
        p = C.c_void_p()
        K.check(self._L.vdo_distance_device_field(self._h, C.byref(p)))
        return p.value

    def sample_raw(self, n, xyz_ptr, words_ptr, is_device):
        """The C entry as it is, on addresses; returns the number of points inside the box."""
        inside = C.c_int64()
        K.check(self._L.vdo_distance_sample(self._h, int(n), C.c_void_p(xyz_ptr or None), C.c_void_p(words_ptr or None), int(bool(is_device)), C.byref(inside)))
        return inside.value

    def sample(self, xyz):
        """World points float32 [m, 3] -> words uint32 [m]; ``self.n_inside`` is the number inside the box"""
        p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
        words = np.zeros(len(p), np.uint32)
        self.n_inside = self.sample_raw(len(p), p.ctypes.data if len(p) else None, words.ctypes.data if len(p) else None, False)
        return words

    def set_method(self, method):
        K.check(self._L.vdo_distance_set_method(self._h, int(method)))


def d2(words):
    """Bits 0-27: the squared distance in voxels, or FAR (of an OUTSIDE word: FAR)"""
    return np.asarray(words, np.uint32) & np.uint32(FAR)


def state(words):
    """Bits 28-29: UNKNOWN, FREE or INSIDE; 255 for an OUTSIDE word"""
    w = np.asarray(words, np.uint32)
    return np.where(w == np.uint32(OUTSIDE), 255, (w >> np.uint32(28)) & np.uint32(3)).astype(np.uint8)


def metres(words, voxel):
    """sqrt(d2) in float64 times the voxel size, narrowed to float32; +inf for FAR, NaN for an OUTSIDE word"""
    w = np.asarray(words, np.uint32)
    d = d2(w)
    m = (np.sqrt(d.astype(np.float64)) * float(np.float32(voxel))).astype(np.float32)
    m = np.where(d == np.uint32(FAR), np.float32(np.inf), m)
    return np.where(w == np.uint32(OUTSIDE), np.float32(np.nan), m).astype(np.float32)
