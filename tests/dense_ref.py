"""NumPy restatement of the dense mapper's contract (include/vdo_slam_hip.h, vdo_dense_*): the geometry in float32 with one rounded operation per
step in the header's order, the fusion, the recentring and the extraction in integers.  The device must equal it bit for bit."""
import numpy as np

F = np.float32
FLT_MIN = np.finfo(np.float32).tiny


def _finite(a):
    return np.abs(a) <= np.finfo(np.float32).max                # false for NaN and the infinities


def floor_div(a, d):
    """floor(a / d) towards -inf for d > 0, on int64 arrays - written out as the kernel does it, not with Python's //"""
    a = np.asarray(a, np.int64)
    return np.where(a >= 0, np.abs(a) // d, -((np.abs(a) + d - 1) // d))


class Volume:
    """The volume of the contract.  words: uint32 [nz, ny, nx] in slot order; origin: int [3] (x, y, z)"""

    def __init__(self, n, voxel, origin=(0, 0, 0)):
        self.n = tuple(int(v) for v in n)
        self.voxel = F(voxel)
        self.origin = np.array(origin, np.int64)
        assert np.all(self.origin > -(1 << 22)) and np.all(self.origin + self.n <= (1 << 22))
        self.words = np.zeros(self.n[::-1], np.uint32)

    def t(self):
        return (self.words & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)

    def w(self):
        return (self.words >> 16).astype(np.int64)

    def globals_of_slots(self, a):
        """the global voxel index of every slot on axis a: the one g in [o, o + n) with g mod n == slot"""
        n, o = self.n[a], int(self.origin[a])
        s = np.arange(n)
        return o + (s - o % n) % n

    def integrate(self, depth, mask, T, K4, trunc, min_depth, max_depth, max_weight):
        """-> (updated, masked, occluded)"""
        depth = np.asarray(depth, F)
        H, W = depth.shape
        T = np.asarray(T, F).reshape(4, 4)
        fx, fy, cx, cy = (F(v) for v in K4)
        trunc, min_depth, max_depth = F(trunc), F(min_depth), F(max_depth)
        gx, gy, gz = (self.globals_of_slots(a) for a in range(3))
        px = ((gx.astype(F) + F(0.5)) * self.voxel)[None, None, :]
        py = ((gy.astype(F) + F(0.5)) * self.voxel)[None, :, None]
        pz = ((gz.astype(F) + F(0.5)) * self.voxel)[:, None, None]
        with np.errstate(all="ignore"):
            Xc = (T[0, 0] * px + T[0, 1] * py) + (T[0, 2] * pz + T[0, 3])
            Yc = (T[1, 0] * px + T[1, 1] * py) + (T[1, 2] * pz + T[1, 3])
            Zc = (T[2, 0] * px + T[2, 1] * py) + (T[2, 2] * pz + T[2, 3])
            assert Zc.dtype == F and Zc.shape == self.words.shape
            ok = _finite(Zc) & (Zc > max(min_depth, FLT_MIN))
            u = (fx * Xc) / Zc + cx
            v = (fy * Yc) / Zc + cy
            xq = np.floor(u + F(0.5)); yq = np.floor(v + F(0.5))
            ok &= _finite(u) & _finite(v) & (xq >= F(0)) & (xq <= F(W - 1)) & (yq >= F(0)) & (yq <= F(H - 1))
            xi = np.where(ok, xq, 0).astype(np.int64); yi = np.where(ok, yq, 0).astype(np.int64)
            d = depth[yi, xi]
            ok &= _finite(d) & (d > min_depth) & (d <= max_depth)
            masked = ok & (np.asarray(mask)[yi, xi] != 0) if mask is not None else np.zeros_like(ok)
            ok &= ~masked
            s = d - Zc
            occluded = ok & (s < -trunc)
            ok &= ~occluded
            s = np.minimum(s, trunc)
            q = np.floor((s / trunc) * F(32767.0) + F(0.5))
            assert q.dtype == F
            q = np.where(ok, q, 0).astype(np.int64)
        t, w = self.t(), self.w()
        t1 = floor_div(2 * (t * w + q) + (w + 1), 2 * (w + 1))
        w1 = np.minimum(w + 1, int(max_weight))
        new = ((w1.astype(np.uint32) << 16) | (t1.astype(np.int16).view(np.uint16).astype(np.uint32))).astype(np.uint32)
        self.words = np.where(ok, new, self.words)
        return int(ok.sum()), int(masked.sum()), int(occluded.sum())

    def recenter(self, new_origin):
        new_origin = np.array(new_origin, np.int64)
        assert np.all(new_origin > -(1 << 22)) and np.all(new_origin + self.n <= (1 << 22))
        g = [self.globals_of_slots(a) for a in range(3)]
        stay = [(g[a] >= new_origin[a]) & (g[a] < new_origin[a] + self.n[a]) for a in range(3)]
        keep = stay[2][:, None, None] & stay[1][None, :, None] & stay[0][None, None, :]
        self.words = np.where(keep, self.words, np.uint32(0))
        self.origin = new_origin

    def at(self, g):
        """word of the global voxel g = (x, y, z), which must be inside the volume"""
        assert all(self.origin[a] <= g[a] < self.origin[a] + self.n[a] for a in range(3))
        return self.words[g[2] % self.n[2], g[1] % self.n[1], g[0] % self.n[0]]

    def extract(self, lo, hi, min_weight):
        """-> (xyz float32 [m, 3], grad int32 [m, 3], weight int32 [m]) in the visiting order"""
        o, n = self.origin, np.array(self.n, np.int64)
        lo = np.maximum(np.array(lo, np.int64), o); hi = np.minimum(np.array(hi, np.int64), o + n)
        xyz, grad, wgt = [], [], []
        if np.all(hi > lo):
            # the box and its +1 neighbours as dense arrays in GLOBAL order, then a vectorised pass per axis
            rng = [np.arange(lo[a], hi[a]) for a in range(3)]
            G = np.meshgrid(rng[2], rng[1], rng[0], indexing="ij")                    # z, y, x
            gz, gy, gx = G
            g = [gx, gy, gz]

            def word(gg):
                return self.words[gg[2] % n[2], gg[1] % n[1], gg[0] % n[0]]
            w0 = word(g)
            ta = (w0 & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64); wa = (w0 >> 16).astype(np.int64)
            tb, usable = [], []
            for k in range(3):
                inside = g[k] + 1 < o[k] + n[k]
                gg = [g[0], g[1], g[2]]
                gg[k] = np.where(inside, g[k] + 1, g[k])
                w1 = word(gg)
                t1 = np.where(inside, (w1 & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64), 0)
                wb = np.where(inside, (w1 >> 16).astype(np.int64), 0)
                tb.append((t1, wb))                                                   # a neighbour outside the volume: t = 0, w = 0
                usable.append(inside & (wb >= min_weight))
            all_in = usable[0] & usable[1] & usable[2]
            cross = [usable[k] & (wa >= min_weight) & ((ta < 0) != (tb[k][0] < 0)) for k in range(3)]
            centre = [(g[c].astype(F) + F(0.5)) for c in range(3)]
            pts = []                                                                  # (order key, xyz, grad, weight) per axis
            idx = np.arange(ta.size).reshape(ta.shape)
            for k in range(3):
                sel = cross[k]
                if not sel.any():
                    continue
                with np.errstate(all="ignore"):
                    frac = ta[sel].astype(F) / (ta[sel] - tb[k][0][sel]).astype(F)
                p = np.stack([(centre[c][sel] + frac if c == k else centre[c][sel]) * self.voxel for c in range(3)], -1).astype(F)
                gr = np.stack([np.where(all_in[sel], tb[c][0][sel] - ta[sel], 0) for c in range(3)], -1).astype(np.int32)
                ww = np.minimum(wa[sel], tb[k][1][sel]).astype(np.int32)
                pts.append((idx[sel] * 3 + k, p, gr, ww))
            if pts:
                key = np.concatenate([p[0] for p in pts]); order = np.argsort(key, kind="stable")
                xyz = np.concatenate([p[1] for p in pts])[order]; grad = np.concatenate([p[2] for p in pts])[order]; wgt = np.concatenate([p[3] for p in pts])[order]
                return np.ascontiguousarray(xyz), np.ascontiguousarray(grad), np.ascontiguousarray(wgt)
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros(0, np.int32)


def normals(grad):
    """What a saved map holds beside a point: the gradient normalised in float64 and narrowed, or 0"""
    g = np.asarray(grad, np.float64)
    n = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    with np.errstate(all="ignore"):
        out = np.where(n[:, None] > 0, g / n[:, None], 0.0)
    return out.astype(F)
