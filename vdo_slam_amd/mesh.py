"""Mesher: surface-nets triangles from a dense mapper's TSDF volume (``vdo_mesh_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h,
"Mesher").  One ``Mesher`` serves every ``DenseMapper`` of its context with no more voxels than it was made for.  ``FollowingMesh`` is the flow of a
volume that follows the camera: before it moves, the quads that will not be wholly inside the staying box are kept, so that the kept pieces and the
last volume hold every quad exactly once."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import dense as _dense


class MeshParamsC(C.Structure):
    _fields_ = [("n", C.c_int32 * 3), ("stage_vertices", C.c_int32), ("stage_triangles", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(_dense._lib(), "vdo_mesh_", {
        "create": [vp, C.POINTER(MeshParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "extract": [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_int, vp],
        "last_timing": [vp, K.c_double_p],
    })


class Mesher(K.StageHandle):
    """``vdo_mesh`` handle for volumes of up to nx * ny * nz voxels; every device buffer is allocated here."""
    _prefix = "vdo_mesh_"

    def __init__(self, ctx, n, stage_vertices=1 << 20, stage_triangles=1 << 21):
        super().__init__(_lib())
        self._ctx = ctx
        self.params = MeshParamsC((C.c_int32 * 3)(*[int(v) for v in n]), int(stage_vertices), int(stage_triangles))
        K.check(self._L.vdo_mesh_create(ctx._h, C.byref(self.params), C.byref(self._h)))

    def extract_raw(self, mapper, lo, hi, outside, min_weight, vertex_capacity, xyz_ptr, grad_ptr, weight_ptr, triangle_capacity, tri_ptr, out_is_device):
        """The C entry as it is, on addresses (each may be 0 / None); returns (vertices, triangles), the totals."""
        clo = (C.c_int32 * 3)(*[int(v) for v in lo]); chi = (C.c_int32 * 3)(*[int(v) for v in hi])
        counts = (C.c_int64 * 2)()
        K.check(self._L.vdo_mesh_extract(self._h, mapper._h, clo, chi, int(outside), int(min_weight), int(vertex_capacity), C.c_void_p(xyz_ptr or None), C.c_void_p(grad_ptr or None),
                                         C.c_void_p(weight_ptr or None), int(triangle_capacity), C.c_void_p(tri_ptr or None), int(bool(out_is_device)), counts))
        return counts[0], counts[1]

    def count(self, mapper, lo, hi, outside=0, min_weight=2):
        return self.extract_raw(mapper, lo, hi, outside, min_weight, 0, None, None, None, 0, None, False)

    def extract(self, mapper, lo, hi, outside=0, min_weight=2, vertex_capacity=None, triangle_capacity=None):
        """-> (xyz float32 [v, 3], grad int32 [v, 3], weight int32 [v], tri int32 [t, 3], (vertices, triangles)); a capacity None: all of them."""
        if vertex_capacity is None or triangle_capacity is None:
            nv, nt = self.count(mapper, lo, hi, outside, min_weight)
            vertex_capacity = nv if vertex_capacity is None else vertex_capacity
            triangle_capacity = nt if triangle_capacity is None else triangle_capacity
        cv, ct = int(vertex_capacity), int(triangle_capacity)
        xyz = np.zeros((cv, 3), np.float32); grad = np.zeros((cv, 3), np.int32); wgt = np.zeros(cv, np.int32); tri = np.zeros((ct, 3), np.int32)
        nv, nt = self.extract_raw(mapper, lo, hi, outside, min_weight, cv, xyz.ctypes.data if cv else None, grad.ctypes.data if cv else None, wgt.ctypes.data if cv else None, ct,
                                  tri.ctypes.data if ct else None, False)
        v, t = min(cv, nv), min(ct, nt)
        return xyz[:v], grad[:v], wgt[:v], tri[:t], (nv, nt)

    def extract_all(self, mapper, min_weight=2):
        o = mapper.origin()
        return self.extract(mapper, o, [o[a] + mapper.n[a] for a in range(3)], 0, min_weight)


def staying_box(origin, new_origin, n):
    """The box [lo, hi) of global voxels a volume moved from origin to new_origin keeps (empty when it moves by n or more on an axis)"""
    lo = [max(origin[a], new_origin[a]) for a in range(3)]
    hi = [min(origin[a], new_origin[a]) + n[a] for a in range(3)]
    if any(hi[a] <= lo[a] for a in range(3)):
        return [0, 0, 0], [0, 0, 0]
    return lo, hi


class FollowingMesh(_dense.FollowingMap):
    """``dense.FollowingMap`` with ``Dense.Mesh: 1``: before the volume moves, one ``outside`` call with the STAYING box; the piece is appended to the
    kept mesh, its triangles rebased by the running vertex count.  The leaving slabs' points are kept as before."""

    def __init__(self, ctx, width, height, n, voxel, K4, **prm):
        super().__init__(ctx, width, height, n, voxel, K4, **prm)
        self.mesher = Mesher(ctx, self.n)
        self.m_xyz, self.m_grad, self.m_wgt, self.m_tri = [], [], [], []
        self.m_vertices = 0

    def _keep_mesh(self, lo, hi, outside):
        xyz, grad, wgt, tri, _ = self.mesher.extract(self.mapper, lo, hi, outside, self.min_weight)
        self.m_xyz.append(xyz); self.m_grad.append(grad); self.m_wgt.append(wgt); self.m_tri.append(tri + np.int32(self.m_vertices))
        self.m_vertices += len(xyz)

    def _before_move(self, origin, new_origin):
        lo, hi = staying_box(origin, new_origin, self.n)
        self._keep_mesh(lo, hi, 1)

    def mesh(self):
        """The kept pieces and the whole current volume: (xyz, normals float32 [v, 3], weight int32 [v], tri int32 [t, 3])"""
        xyz, grad, wgt, tri, _ = self.mesher.extract_all(self.mapper, self.min_weight)
        X = np.concatenate(self.m_xyz + [xyz]); G = np.concatenate(self.m_grad + [grad]); Wt = np.concatenate(self.m_wgt + [wgt])
        T = np.concatenate(self.m_tri + [tri + np.int32(self.m_vertices)])
        return X, _normals(G), Wt, T

    def close(self):
        self.mesher.close()
        super().close()


def write_ply(path, xyz, normals, weight, tri):
    """Binary little-endian PLY: vertex x y z nx ny nz (float) weight (int) as a saved dense map has them, face as uchar-counted int lists of 3"""
    v = np.zeros(len(xyz), _dense.PLY_DTYPE)
    for c, name in enumerate(("x", "y", "z")):
        v[name] = np.asarray(xyz, np.float32)[:, c]; v["n" + name] = np.asarray(normals, np.float32)[:, c]
    v["weight"] = weight
    f = np.zeros(len(tri), FACE_DTYPE)
    f["n"] = 3; f["v"] = np.asarray(tri, np.int32).reshape(-1, 3)
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
            f"property float nz\nproperty int weight\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(head.encode("ascii")); out.write(v.tobytes()); out.write(f.tobytes())


FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def read_ply(path):
    """What write_ply wrote -> (xyz float32 [v, 3], normals float32 [v, 3], weight int32 [v], tri int32 [t, 3])"""
    with open(path, "rb") as f:
        nv = nf = None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            if line.startswith(b"element vertex"):
                nv = int(line.split()[2])
            if line.startswith(b"element face"):
                nf = int(line.split()[2])
            if line.strip() == b"end_header":
                break
        v = np.frombuffer(f.read(nv * _dense.PLY_DTYPE.itemsize), _dense.PLY_DTYPE, nv)
        fc = np.frombuffer(f.read(nf * FACE_DTYPE.itemsize), FACE_DTYPE, nf)
    if nf and not np.all(fc["n"] == 3):
        raise ValueError(f"{path}: a face that is not a triangle")
    return np.stack([v["x"], v["y"], v["z"]], -1), np.stack([v["nx"], v["ny"], v["nz"]], -1), v["weight"].copy(), fc["v"].copy().reshape(-1, 3)


def _normals(grad):
    """The gradient normalised in float64 and narrowed, or 0 (as a saved map's normals)"""
    g = np.asarray(grad, np.float64).reshape(-1, 3)
    n = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    with np.errstate(all="ignore"):
        return np.where(n[:, None] > 0, g / n[:, None], 0.0).astype(np.float32)
