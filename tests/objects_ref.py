"""NumPy restatement of the object mapper's contract (include/vdo_slam_hip.h, vdo_objects_*): the label statistics in int64 with the fp32 steps in
the header's order, the label-selecting fusion on tests/dense_ref.Volume (the mask image is `mask != label`), and the per-frame lifecycle of
vdo_slam_amd/objects.py's ObjectMaps in pure NumPy.  The device must equal the first two bit for bit."""
import numpy as np

from tests import dense_ref as R

F = np.float32


def stats(depth, mask, K4, min_depth, max_depth, max_labels):
    """-> int64 [max_labels + 1, 8]: count, x0, y0, x1, y1, sum qx, sum qy, sum qz"""
    depth = np.asarray(depth, F); mask = np.asarray(mask, np.int32)
    H, W = depth.shape
    fx, fy, cx, cy = (F(v) for v in K4)
    out = np.zeros((max_labels + 1, 8), np.int64)
    out[:, 1] = W; out[:, 2] = H; out[:, 3] = -1; out[:, 4] = -1
    with np.errstate(all="ignore"):
        ok = R._finite(depth) & (depth > F(min_depth)) & (depth <= F(max_depth))
        ys, xs = np.mgrid[0:H, 0:W]
        d = np.where(ok, depth, F(0))
        qx = np.floor((((xs.astype(F) - cx) * d) / fx) * F(1024) + F(0.5))
        qy = np.floor((((ys.astype(F) - cy) * d) / fy) * F(1024) + F(0.5))
        qz = np.floor(d * F(1024) + F(0.5))
        assert qx.dtype == F and qy.dtype == F and qz.dtype == F
    inside = ok & (mask >= 1) & (mask <= max_labels)
    out[0, 0] = int((ok & (mask != 0) & ~inside).sum())
    for l in np.unique(mask[inside]):
        sel = inside & (mask == l)
        out[l] = [sel.sum(), xs[sel].min(), ys[sel].min(), xs[sel].max(), ys[sel].max(), qx[sel].astype(np.int64).sum(), qy[sel].astype(np.int64).sum(), qz[sel].astype(np.int64).sum()]
    return out


def integrate(V, depth, mask, label, T, K4, trunc, min_depth, max_depth, max_weight):
    """The label-selecting fusion into a dense_ref.Volume -> (updated, occluded)"""
    upd, _, occ = V.integrate(depth, (np.asarray(mask) != label).astype(np.int32), T, K4, trunc, min_depth, max_depth, max_weight)
    return upd, occ


def mul44(A, B):
    """A * B in float64 with every entry summed left to right (no BLAS, no contraction): what the device-side flow and the host class chain"""
    A = np.asarray(A, np.float64).reshape(4, 4); B = np.asarray(B, np.float64).reshape(4, 4)
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def rigid_inverse(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    for a in range(3):
        out[a, 3] = -((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3])
    return out


class RefModel:
    def __init__(self, mod_label, sem_label, Two, V):
        self.mod_label, self.sem_label, self.Two, self.V = mod_label, sem_label, Two, V
        self.frames = 0
        self.traj = []
        self.xyz = self.grad = self.wgt = None


class RefMaps:
    """The lifecycle flow of the issue, step by step, on dense_ref volumes"""

    def __init__(self, width, height, K4, voxel, size=(96, 64, 96), trunc=None, min_depth=0.0, max_depth=25.0, max_weight=64, max_objects=16, min_pixels=200, min_frames=3,
                 min_weight=2, max_labels=1023):
        self.K4, self.voxel, self.size = K4, F(voxel), tuple(size)
        self.trunc = F(4.0) * F(voxel) if trunc is None else F(trunc)
        self.min_depth, self.max_depth, self.max_weight = min_depth, max_depth, max_weight
        self.max_objects, self.min_pixels, self.min_frames, self.min_weight, self.max_labels = max_objects, min_pixels, min_frames, min_weight, max_labels
        self.origin = tuple(-(n // 2) for n in self.size)
        self.live, self.finished = [], []
        self.dropped = self.skipped = 0

    def _count(self, st, sem):
        return int(st[sem, 0]) if 1 <= sem <= self.max_labels else 0

    def _extract(self, V):
        o = V.origin
        return V.extract(o, o + np.array(V.n), self.min_weight)

    def fuse(self, f, depth, mask, Tcw, motions):
        Tcw = np.asarray(Tcw).reshape(4, 4).astype(np.float64)
        st = stats(depth, mask, self.K4, self.min_depth, self.max_depth, self.max_labels)                  # 1
        present = {int(mo[0]) for mo in motions}
        for m in [m for m in self.live if m.mod_label not in present]:                                     # 2
            self.live.remove(m)
            if m.frames >= self.min_frames:
                m.xyz, m.grad, m.wgt = self._extract(m.V)
                self.finished.append(m)
            else:
                self.dropped += 1
            m.V = None
        seen_mod, seen_sem = set(), set()
        for mod, sem, H in motions:                                                                        # 3
            mod, sem = int(mod), int(sem)
            if mod in seen_mod or sem in seen_sem:
                continue
            seen_mod.add(mod); seen_sem.add(sem)
            hit = [m for m in self.live if m.mod_label == mod]
            if hit:
                hit[0].Two = mul44(H, hit[0].Two)
                hit[0].sem_label = sem
            elif len(self.live) < self.max_objects and self._count(st, sem) >= self.min_pixels:
                c = st[sem, 5:8].astype(np.float64) / (1024.0 * float(st[sem, 0]))
                Twc = rigid_inverse(Tcw)
                Two = np.eye(4)
                for a in range(3):
                    Two[a, 3] = ((Twc[a, 0] * c[0] + Twc[a, 1] * c[1]) + Twc[a, 2] * c[2]) + Twc[a, 3]
                self.live.append(RefModel(mod, sem, Two, R.Volume(self.size, self.voxel, self.origin)))
            else:
                self.skipped += 1
        for m in self.live:                                                                                # 4
            if self._count(st, m.sem_label) >= self.min_pixels:
                T = mul44(Tcw, m.Two).astype(F)
                integrate(m.V, depth, mask, m.sem_label, T, self.K4, self.trunc, self.min_depth, self.max_depth, self.max_weight)
                m.frames += 1
            m.traj.append((int(f), m.Two.copy()))
        return st

    def models(self):
        out = []
        for m in self.finished + self.live:
            xyz, grad, wgt = (m.xyz, m.grad, m.wgt) if m.V is None else self._extract(m.V)
            out.append(dict(mod_label=m.mod_label, live=m.V is not None, frames=m.frames, xyz=xyz, grad=grad, weight=wgt, trajectory=list(m.traj)))
        return out

    def info(self):
        return [(m["mod_label"], m["live"], m["frames"], len(m["xyz"])) for m in self.models()]
