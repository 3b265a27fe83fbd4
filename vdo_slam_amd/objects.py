"""Object mapper: a TSDF volume per tracked object (``vdo_objects_*`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h).  ``ObjectStage`` is
the device stage - the per-label statistics of a frame and one label-selecting fusion launch over a batch of ``DenseMapper`` volumes.
``ObjectMaps`` is the per-frame lifecycle on top of it: a model per tracking id in a frame of the object's own, whose pose is chained from the
tracker's world-frame motions, started at the label's centroid, fused while the label is seen and kept as points when the object is gone."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .dense import PLY_DTYPE, DenseMapper

STAT_COLS = 8            # count, x0, y0, x1, y1, sum qx, sum qy, sum qz (2^-10 m)


class ObjectsParamsC(C.Structure):
    _fields_ = [("K", C.c_float * 4), ("min_depth", C.c_float), ("max_depth", C.c_float), ("max_labels", C.c_int32), ("max_batch", C.c_int32)]


def _lib():
    vp = C.c_void_p
    return K.declare(K.lib(), "vdo_objects_", {
        "create": [vp, C.c_int, C.c_int, C.POINTER(ObjectsParamsC), C.POINTER(vp)],
        "destroy": [vp],
        "stats": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp],
        "stats_frame": [vp, vp, vp],
        "integrate": [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp],
        "integrate_frame": [vp, vp, C.c_int, vp, vp, vp, vp],
        "set_cull": [vp, C.c_int],
        "last_stats": [vp, vp],
        "last_timing": [vp, K.c_double_p],
    })


def clear(mapper: DenseMapper):
    """``vdo_dense_clear``: every word 0, the origin kept"""
    mapper.clear()


class ObjectStage(K.StageHandle):
    """``vdo_objects`` handle for width x height images; it owns the tables, the counters and the image staging, and no volume."""
    _prefix = "vdo_objects_"

    def __init__(self, ctx, width, height, K4, min_depth=0.0, max_depth=25.0, max_labels=1023, max_batch=16):
        super().__init__(_lib())
        self.width, self.height, self.max_labels, self.max_batch = int(width), int(height), int(max_labels), int(max_batch)
        self.params = ObjectsParamsC((C.c_float * 4)(*[float(v) for v in K4]), float(min_depth), float(max_depth), int(max_labels), int(max_batch))
        self._ctx = ctx
        K.check(self._L.vdo_objects_create(ctx._h, self.width, self.height, C.byref(self.params), C.byref(self._h)))

    def _table(self):
        return np.zeros((self.max_labels + 1, STAT_COLS), np.int64)

    def stats_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device):
        t = self._table()
        K.check(self._L.vdo_objects_stats(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)), t.ctypes.data))
        return t

    def stats(self, depth, mask):
        """Host images (row strides are honoured) -> int64 [max_labels + 1, 8]"""
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width))
        return self.stats_raw(pd, sd, pm, sm, False)

    def stats_frame(self, frame_handle):
        t = self._table()
        fh = frame_handle if isinstance(frame_handle, C.c_void_p) else C.c_void_p(frame_handle or None)
        K.check(self._L.vdo_objects_stats_frame(self._h, fh, t.ctypes.data))
        return t

    @staticmethod
    def _batch(maps, labels, T):
        n = len(maps)
        hs = (C.c_void_p * max(n, 1))(*[m._h.value if isinstance(m, DenseMapper) else m for m in maps])
        lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(n))
        Ts = np.ascontiguousarray(np.asarray(T, np.float32).reshape(n, 16))
        out = np.zeros((n, 3), np.int64)
        return n, hs, lab, Ts, out

    def integrate_raw(self, depth_ptr, depth_stride, mask_ptr, mask_stride, src_is_device, maps, labels, T):
        """The C entry as it is, on addresses -> int64 [n, 3]: updated, occluded, the label's pixel count"""
        n, hs, lab, Ts, out = self._batch(maps, labels, T)
        K.check(self._L.vdo_objects_integrate(self._h, C.c_void_p(depth_ptr or None), int(depth_stride), C.c_void_p(mask_ptr or None), int(mask_stride), int(bool(src_is_device)), n,
                                              hs, lab.ctypes.data, Ts.ctypes.data, out.ctypes.data))
        return out

    def integrate(self, depth, mask, maps, labels, T):
        """Host images; maps: DenseMapper objects, labels: their mask labels, T: [n, 4, 4] object frame -> camera"""
        d, pd, sd = K.rows(depth, "depth", np.float32, (self.height, self.width))
        m, pm, sm = K.rows(mask, "mask", np.int32, (self.height, self.width))
        return self.integrate_raw(pd, sd, pm, sm, False, maps, labels, T)

    def integrate_frame(self, frame_handle, maps, labels, T):
        n, hs, lab, Ts, out = self._batch(maps, labels, T)
        fh = frame_handle if isinstance(frame_handle, C.c_void_p) else C.c_void_p(frame_handle or None)
        K.check(self._L.vdo_objects_integrate_frame(self._h, fh, n, hs, lab.ctypes.data, Ts.ctypes.data, out.ctypes.data))
        return out

    def set_cull(self, on):
        K.check(self._L.vdo_objects_set_cull(self._h, int(on)))

    def last_stats(self):
        t = self._table()
        K.check(self._L.vdo_objects_last_stats(self._h, t.ctypes.data))
        return t


def mul44(A, B):
    """A * B, 4 x 4 float64, every entry ((a0*b0 + a1*b1) + a2*b2) + a3*b3 - the order of host/ObjectMapper.cc, so that both chain the same bits"""
    A = np.asarray(A, np.float64).reshape(4, 4); B = np.asarray(B, np.float64).reshape(4, 4)
    return ((A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]) + A[:, 3:4] * B[3:4, :]


def rigid_inverse(T):
    """[R | t] -> [R^T | -R^T t] in float64, the translation -((r0a*t0 + r1a*t1) + r2a*t2)"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    for a in range(3):
        out[a, 3] = -((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3])
    return out


def centroid_pose(Tcw, row):
    """Two of a model started on a label with the stats row `row`: world axes, the origin at the world position of the label's centroid
    Twc * (sx, sy, sz) / (1024 * count)"""
    den = 1024.0 * float(row[0])
    c = [float(row[5]) / den, float(row[6]) / den, float(row[7]) / den]
    Twc = rigid_inverse(Tcw)
    Two = np.eye(4)
    for a in range(3):
        Two[a, 3] = ((Twc[a, 0] * c[0] + Twc[a, 1] * c[1]) + Twc[a, 2] * c[2]) + Twc[a, 3]
    return Two


class _Model:
    def __init__(self, mod_label, sem_label, Two, mapper):
        self.mod_label, self.sem_label, self.Two, self.mapper = int(mod_label), int(sem_label), Two, mapper
        self.frames = 0
        self.traj = []                                                       # (frame, Two 4 x 4 float64)
        self.xyz = self.grad = self.wgt = None                               # a finished model's points, object frame


class ObjectMaps:
    """The per-frame flow: ``fuse(f, depth, mask, Tcw, motions)`` with motions = [(mod_label, sem_label, H 4 x 4)] in the tracker's order, H the
    world-frame motion from the last frame to this one.  All pose algebra is float64; T_i = Tcw * Two is rounded to float32 once per entry."""

    def __init__(self, ctx, width, height, K4, voxel, size=(96, 64, 96), trunc=None, min_depth=0.0, max_depth=25.0, max_weight=64, max_objects=16, min_pixels=200, min_frames=3,
                 min_weight=2, max_labels=1023, stage_points=1 << 18):
        if not 1 <= int(max_objects) <= 64:
            raise ValueError("max_objects outside 1..64")
        self.ctx, self.width, self.height, self.K4 = ctx, int(width), int(height), tuple(float(v) for v in K4)
        self.size, self.voxel = tuple(int(v) for v in size), float(voxel)
        self.prm = dict(trunc=trunc, min_depth=min_depth, max_depth=max_depth, max_weight=max_weight, stage_points=stage_points)
        self.max_objects, self.min_pixels, self.min_frames, self.min_weight = int(max_objects), int(min_pixels), int(min_frames), int(min_weight)
        self.stage = ObjectStage(ctx, width, height, K4, min_depth=min_depth, max_depth=max_depth, max_labels=max_labels, max_batch=self.max_objects)
        self.origin = tuple(-(n // 2) for n in self.size)
        self.live, self.finished, self.pool = [], [], []
        self.dropped = self.skipped = 0
        self.last_counts = {}                                                # mod_label -> (updated, occluded, pixels) of the last frame

    def _count(self, stats, sem):
        return int(stats[sem, 0]) if 1 <= sem <= self.stage.max_labels else 0

    def _retire(self, m):
        xyz, grad, wgt, _ = m.mapper.extract_all(self.min_weight)
        if m.frames >= self.min_frames:
            m.xyz, m.grad, m.wgt = xyz, grad, wgt
            self.finished.append(m)
        else:
            self.dropped += 1
        clear(m.mapper)
        self.pool.append(m.mapper)
        m.mapper = None

    def fuse(self, f, depth, mask, Tcw, motions):
        Tcw = np.asarray(Tcw).reshape(4, 4).astype(np.float64)
        stats = self.stage.stats(depth, mask)
        present = {int(mo[0]) for mo in motions}
        for m in [m for m in self.live if m.mod_label not in present]:
            self.live.remove(m)
            self._retire(m)
        seen_mod, seen_sem = set(), set()
        by_label = {m.mod_label: m for m in self.live}
        for mod, sem, H in motions:
            mod, sem = int(mod), int(sem)
            if mod in seen_mod or sem in seen_sem:
                continue
            seen_mod.add(mod); seen_sem.add(sem)
            m = by_label.get(mod)
            if m is not None:
                m.Two = mul44(H, m.Two)
                m.sem_label = sem
            elif len(self.live) < self.max_objects and self._count(stats, sem) >= self.min_pixels:
                mapper = self.pool.pop() if self.pool else DenseMapper(self.ctx, self.width, self.height, self.size, self.voxel, self.K4, origin=self.origin, **self.prm)
                m = _Model(mod, sem, centroid_pose(Tcw, stats[sem]), mapper)
                self.live.append(m); by_label[mod] = m
            else:
                self.skipped += 1
        batch = [m for m in self.live if self._count(stats, m.sem_label) >= self.min_pixels]
        T = np.array([mul44(Tcw, m.Two).astype(np.float32) for m in batch], np.float32).reshape(len(batch), 4, 4)
        out = self.stage.integrate(depth, mask, [m.mapper for m in batch], [m.sem_label for m in batch], T)
        self.last_counts = {}
        for m, o in zip(batch, out):
            m.frames += 1
            self.last_counts[m.mod_label] = tuple(int(v) for v in o)
        for m in self.live:
            m.traj.append((int(f), m.Two.copy()))
        return stats

    def models(self):
        """Finished models, then the live ones as they stand: dicts of mod_label, live, frames, xyz, grad, weight (object frame), trajectory"""
        out = []
        for m in self.finished + self.live:
            if m.mapper is None:
                xyz, grad, wgt = m.xyz, m.grad, m.wgt
            else:
                xyz, grad, wgt, _ = m.mapper.extract_all(self.min_weight)
            out.append(dict(mod_label=m.mod_label, live=m.mapper is not None, frames=m.frames, xyz=xyz, grad=grad, weight=wgt, trajectory=list(m.traj)))
        return out

    def info(self):
        """[(mod_label, live, frames fused, points)] - finished first, then live"""
        return [(m["mod_label"], m["live"], m["frames"], len(m["xyz"])) for m in self.models()]

    def save(self, prefix):
        """<prefix>_<mod_label>.ply per model (object frame; the binary layout of a saved static map) and <prefix>_poses.txt: frame, mod_label and
        the 16 entries of Two per row, fixed with 9 digits"""
        rows = []
        for m in self.models():
            g = m["grad"].astype(np.float64)
            nrm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
            with np.errstate(all="ignore"):
                N = np.where(nrm[:, None] > 0, g / nrm[:, None], 0.0).astype(np.float32)
            a = np.zeros(len(m["xyz"]), PLY_DTYPE)
            for k, name in enumerate(("x", "y", "z")):
                a[name] = m["xyz"][:, k]; a["n" + name] = N[:, k]
            a["weight"] = m["weight"]
            with open(f"{prefix}_{m['mod_label']}.ply", "wb") as fo:
                fo.write(f"ply\nformat binary_little_endian 1.0\ncomment object {m['mod_label']}, object frame, TSDF zero crossings\nelement vertex {len(a)}\n".encode())
                fo.write(b"property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty int weight\nend_header\n")
                fo.write(a.tobytes())
            rows += [(fr, m["mod_label"], Two) for fr, Two in m["trajectory"]]
        with open(f"{prefix}_poses.txt", "w") as fo:
            for fr, mod, Two in rows:
                fo.write(f"{fr} {mod} " + " ".join(f"{v:.9f}" for v in Two.reshape(16)) + "\n")

    def close(self):
        for m in self.live:
            m.mapper.close()
        for mp in self.pool:
            mp.close()
        self.live, self.pool = [], []
        self.stage.close()
