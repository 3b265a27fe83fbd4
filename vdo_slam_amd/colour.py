"""Colourer: a colour per voxel beside a dense mapper's TSDF volume, fused from the image a frame's depth belongs to and read back at points or along
a depth image (``vdo_colour_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h, "Colourer").  A ``Colourer`` borrows its ``DenseMapper``:
close it before the mapper.  ``FollowingColourMesh`` is ``mesh.FollowingMesh`` with ``Dense.Colour: 1``: what it keeps before a move is coloured
before the move, while its voxels are still in the volume."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import dense as _dense
from . import mesh as _mesh


class ColourParamsC(C.Structure):
    _fields_ = [("band", C.c_float), ("max_weight", C.c_int32), ("stage_points", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(_dense._lib(), "vdo_colour_", {
        "create": [vp, C.POINTER(ColourParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "integrate": [vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp],
        "integrate_frame": [vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp],
        "sample": [vp, C.c_int64, vp, C.c_int, vp, C.c_int, vp],
        "render": [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp],
        "clear": [vp],
        "get_volume": [vp, vp, vp],
        "set_volume": [vp, vp],
        "set_voxels_per_thread": [vp, C.c_int],
        "last_timing": [vp, K.c_double_p],
    })


class Colourer(K.StageHandle):
    """``vdo_colour`` handle over ``mapper`` (a ``dense.DenseMapper``): ``band`` metres (None: half the map's truncation), ``max_weight`` (None: the
    map's).  Every device buffer is allocated here."""
    _prefix = "vdo_colour_"

    def __init__(self, mapper, band=None, max_weight=None, stage_points=1 << 20):
        super().__init__(_lib())
        self._mapper = mapper                                   # the colourer borrows the map: keep it alive
        band = float(np.float32(mapper.params.trunc) / np.float32(2)) if band is None else band
        max_weight = mapper.params.max_weight if max_weight is None else max_weight
        self.params = ColourParamsC(float(band), int(max_weight), int(stage_points))
        self.n = mapper.n
        self.width, self.height = mapper.width, mapper.height
        K.check(self._L.vdo_colour_create(mapper._h, C.byref(self.params), C.byref(self._h)))

    def integrate_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, image_ptr, image_stride, channels, rgb_order, src_is_device, label, T):
        """The C entry as it is, on addresses (mask_ptr may be 0 / None); returns (updated, skipped by the label rule, skipped by the band rule)."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = (C.c_int64 * 3)()
        K.check(self._L.vdo_colour_integrate(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), C.c_void_p(image_ptr or None),
                                             int(image_stride), int(channels), int(rgb_order), int(bool(src_is_device)), int(label), T.ctypes.data, out))
        return out[0], out[1], out[2]

    def integrate(self, depth, mask, image, T, label=0, rgb_order=0):
        """Host images: depth float32 [height, width] metres, mask int32 [height, width] or None, image uint8 [height, width] or [height, width, 1 | 3 |
        4]; row strides are honoured."""
        H, W = self.height, self.width
        d, pd, sd = K.rows(depth, "depth", np.float32, (H, W))
        m, pm, sm = K.rows(mask, "mask", np.int32, (H, W)) if mask is not None else (None, None, 0)
        image = np.asarray(image)
        ch = 1 if image.ndim == 2 else image.shape[2]
        im, pi, si = K.rows(image, "image", np.uint8, (H, W) if image.ndim == 2 else (H, W, ch))
        return self.integrate_raw(pd, sd, pm, sm, pi, si, ch, rgb_order, False, label, T)

    def integrate_frame(self, frame_handle, image_ptr, image_stride, channels, rgb_order, image_is_device, T, label=0):
        """From the resident depth and mask of a ``vdo_frame_images`` (its address) and an image at an address."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        out = (C.c_int64 * 3)()
        fh = frame_handle if isinstance(frame_handle, C.c_void_p) else C.c_void_p(frame_handle or None)
        K.check(self._L.vdo_colour_integrate_frame(self._h, fh, C.c_void_p(image_ptr or None), int(image_stride), int(channels), int(rgb_order), int(bool(image_is_device)), int(label),
                                                   T.ctypes.data, out))
        return out[0], out[1], out[2]

    def sample_raw(self, n, xyz_ptr, min_weight, rgba_ptr, is_device):
        """The C entry as it is, on addresses; returns the number of coloured points."""
        c = C.c_int64()
        K.check(self._L.vdo_colour_sample(self._h, int(n), C.c_void_p(xyz_ptr or None), int(min_weight), C.c_void_p(rgba_ptr or None), int(bool(is_device)), C.byref(c)))
        return c.value

    def sample(self, xyz, min_weight=1):
        """xyz float32 [n, 3] world points -> (rgba uint8 [n, 4], the number of coloured points)"""
        p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
        rgba = np.zeros((len(p), 4), np.uint8)
        c = self.sample_raw(len(p), p.ctypes.data if len(p) else None, min_weight, rgba.ctypes.data if len(p) else None, False)
        return rgba, c

    def render_raw(self, depth_ptr, width, height, K4, T, min_weight, rgba_ptr, is_device):
        """The C entry as it is, on addresses; returns (pixels coloured, pixels with depth but no colour)."""
        T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        Kc = (C.c_float * 4)(*[float(v) for v in K4])
        out = (C.c_int64 * 2)()
        K.check(self._L.vdo_colour_render(self._h, C.c_void_p(depth_ptr or None), int(width), int(height), Kc, T.ctypes.data, int(min_weight), C.c_void_p(rgba_ptr or None),
                                          int(bool(is_device)), out))
        return out[0], out[1]

    def render(self, depth, K4, T, min_weight=1):
        """depth float32 [h, w] as ``Raycaster.render`` gives it, at the K4 and T it was rendered with -> (rgba uint8 [h, w, 4], counts)"""
        d = np.ascontiguousarray(depth, np.float32)
        rgba = np.zeros(d.shape + (4,), np.uint8)
        counts = self.render_raw(d.ctypes.data, d.shape[1], d.shape[0], K4, T, min_weight, rgba.ctypes.data, False)
        return rgba, counts

    def clear(self):
        K.check(self._L.vdo_colour_clear(self._h))

    def volume(self):
        """(words uint32 [nz, ny, nx] in slot order, origin (x, y, z)), after the colour volume followed the map"""
        w = np.zeros(self.n[::-1], np.uint32)
        o = (C.c_int32 * 3)()
        K.check(self._L.vdo_colour_get_volume(self._h, w.ctypes.data, o))
        return w, (o[0], o[1], o[2])

    def set_volume(self, words):
        w = np.ascontiguousarray(words, np.uint32)
        if w.shape != self.n[::-1]:
            raise ValueError(f"words: {w.shape}, expected {self.n[::-1]}")
        K.check(self._L.vdo_colour_set_volume(self._h, w.ctypes.data))

    def set_voxels_per_thread(self, v):
        K.check(self._L.vdo_colour_set_voxels_per_thread(self._h, int(v)))

    def close(self):
        super().close()
        self._mapper = None


class FollowingColourMesh(_mesh.FollowingMesh):
    """``mesh.FollowingMesh`` with ``Dense.Colour: 1``: every frame's image is fused after its depth with the same pose; the points and mesh vertices
    kept before a move are sampled BEFORE the volume moves - after it their voxels are gone."""

    def __init__(self, ctx, width, height, n, voxel, K4, band=None, colour_max_weight=None, colour_min_weight=1, **prm):
        super().__init__(ctx, width, height, n, voxel, K4, **prm)
        self.colourer = Colourer(self.mapper, band, colour_max_weight)
        self.colour_min_weight = int(colour_min_weight)
        self.rgba, self.m_rgba = [], []

    def _before_move(self, origin, new_origin):
        super()._before_move(origin, new_origin)                # the seam piece of the mesh, then its colours
        self.m_rgba.append(self.colourer.sample(self.m_xyz[-1], self.colour_min_weight)[0])

    def _keep(self, lo, hi):
        super()._keep(lo, hi)                                   # (fuse calls it before mapper.recenter: the volume has not moved yet)
        self.rgba.append(self.colourer.sample(self.xyz[-1], self.colour_min_weight)[0])

    def fuse(self, depth, mask, image, Tcw, rgb_order=0):
        counts = super().fuse(depth, mask, Tcw)
        return counts, self.colourer.integrate(depth, mask, image, Tcw, 0, rgb_order)

    def coloured_points(self):
        """``points()`` and their colours uint8 [m, 4]"""
        X, N, Wt = self.points()
        now = self.colourer.sample(X[sum(len(a) for a in self.xyz):], self.colour_min_weight)[0]
        return X, N, Wt, np.concatenate(self.rgba + [now])

    def coloured_mesh(self):
        """``mesh()`` and the vertex colours uint8 [v, 4]"""
        X, N, Wt, T = self.mesh()
        now = self.colourer.sample(X[self.m_vertices:], self.colour_min_weight)[0]
        return X, N, Wt, T, np.concatenate(self.m_rgba + [now])

    def close(self):
        self.colourer.close()
        super().close()


PLY_COLOUR_DTYPE = np.dtype(_dense.PLY_DTYPE.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def write_ply(path, xyz, normals, weight, tri, rgba=None):
    """``mesh.write_ply``, and its very bytes, when rgba is None; else the vertices also carry red green blue alpha (uchar)"""
    if rgba is None:
        return _mesh.write_ply(path, xyz, normals, weight, tri)
    v = np.zeros(len(xyz), PLY_COLOUR_DTYPE)
    for c, name in enumerate(("x", "y", "z")):
        v[name] = np.asarray(xyz, np.float32)[:, c]; v["n" + name] = np.asarray(normals, np.float32)[:, c]
    v["weight"] = weight
    for c, name in enumerate(("red", "green", "blue", "alpha")):
        v[name] = np.asarray(rgba, np.uint8).reshape(-1, 4)[:, c]
    f = np.zeros(len(tri), _mesh.FACE_DTYPE)
    f["n"] = 3; f["v"] = np.asarray(tri, np.int32).reshape(-1, 3)
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
            f"property float nz\nproperty int weight\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face {len(f)}\n"
            f"property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(head.encode("ascii")); out.write(v.tobytes()); out.write(f.tobytes())


def read_ply(path):
    """A mesh or point PLY of this library, with or without colours -> (xyz, normals float32 [v, 3], weight int32 [v], tri int32 [t, 3], rgba uint8
    [v, 4] or None); a file without faces gives an empty tri"""
    with open(path, "rb") as f:
        nv, nf, coloured = None, 0, False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            if line.startswith(b"element vertex"):
                nv = int(line.split()[2])
            if line.startswith(b"element face"):
                nf = int(line.split()[2])
            if line.strip() == b"property uchar red":
                coloured = True
            if line.strip() == b"end_header":
                break
        dt = PLY_COLOUR_DTYPE if coloured else _dense.PLY_DTYPE
        v = np.frombuffer(f.read(nv * dt.itemsize), dt, nv)
        fc = np.frombuffer(f.read(nf * _mesh.FACE_DTYPE.itemsize), _mesh.FACE_DTYPE, nf)
    if nf and not np.all(fc["n"] == 3):
        raise ValueError(f"{path}: a face that is not a triangle")
    rgba = np.stack([v["red"], v["green"], v["blue"], v["alpha"]], -1) if coloured else None
    return np.stack([v["x"], v["y"], v["z"]], -1), np.stack([v["nx"], v["ny"], v["nz"]], -1), v["weight"].copy(), fc["v"].copy().reshape(-1, 3), rgba
