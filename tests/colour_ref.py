"""NumPy restatement of the colourer's contract (include/vdo_slam_hip.h, "Colourer", vdo_colour_*): pack, follow, integrate, sample and render.  The
geometry in float32 with one rounded operation per step in the header's order, the integer parts in int64.  The device must equal it bit for bit."""
import numpy as np

from tests.dense_ref import F, FLT_MIN, _finite


def pack(image, rgb_order=0):
    """uint8 [H, W] or [H, W, 1 | 3 | 4] -> uint32 [H, W]: R | G << 8 | B << 16, grey replicated, a fourth channel ignored"""
    im = np.asarray(image, np.uint8)
    if im.ndim == 2:
        im = im[:, :, None]
    if im.shape[2] == 1:
        r = g = b = im[:, :, 0].astype(np.uint32)
    else:
        assert im.shape[2] in (3, 4)
        r = im[:, :, 2 if rgb_order else 0].astype(np.uint32); g = im[:, :, 1].astype(np.uint32); b = im[:, :, 0 if rgb_order else 2].astype(np.uint32)
    return r | (g << 8) | (b << 16)


class ColourVolume:
    """The colour volume of the contract.  words: uint32 [nz, ny, nx] in slot order; origin: the map origin it stands at"""

    def __init__(self, n, voxel, origin=(0, 0, 0)):
        self.n = tuple(int(v) for v in n)
        self.voxel = F(voxel)
        self.origin = np.array(origin, np.int64)
        self.words = np.zeros(self.n[::-1], np.uint32)

    def globals_of_slots(self, a):
        n, o = self.n[a], int(self.origin[a])
        s = np.arange(n)
        return o + (s - o % n) % n

    def follow(self, map_origin):
        """The slots whose global voxel changes are set to 0 (everything after a shift of n or more on an axis), no other word is touched"""
        new = np.array(map_origin, np.int64)
        g = [self.globals_of_slots(a) for a in range(3)]
        stay = [(g[a] >= new[a]) & (g[a] < new[a] + self.n[a]) for a in range(3)]
        keep = stay[2][:, None, None] & stay[1][None, :, None] & stay[0][None, None, :]
        self.words = np.where(keep, self.words, np.uint32(0))
        self.origin = new

    def clear(self, map_origin):
        self.words[:] = 0
        self.origin = np.array(map_origin, np.int64)

    def integrate(self, depth, mask, image, T, K4, min_depth, max_depth, band, max_weight, label=0, rgb_order=0, map_origin=None):
        """-> (updated, skipped by the label rule, skipped by the band rule)"""
        if map_origin is not None:
            self.follow(map_origin)
        depth = np.asarray(depth, F)
        H, W = depth.shape
        img = pack(image, rgb_order)
        assert img.shape == (H, W)
        T = np.asarray(T, F).reshape(4, 4)
        fx, fy, cx, cy = (F(v) for v in K4)
        min_depth, max_depth, band = F(min_depth), F(max_depth), F(band)
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
            m = np.asarray(mask)[yi, xi].astype(np.int64) if mask is not None else np.zeros(ok.shape, np.int64)
            if label == 0:
                skip = m != 0
            elif label > 0:
                skip = m != label
            else:
                skip = np.zeros(ok.shape, bool)
            labelled = ok & skip
            ok &= ~labelled
            s = d - Zc
            assert s.dtype == F
            out_band = ok & ~(np.abs(s) <= band)
            ok &= ~out_band
        q = img[yi, xi].astype(np.int64)
        w = self.words.astype(np.int64)
        cw = w >> 24
        new = np.minimum(cw + 1, int(max_weight)) << 24
        for c in range(3):
            old = (w >> (8 * c)) & 0xFF; obs = (q >> (8 * c)) & 0xFF
            new |= ((2 * (old * cw + obs) + (cw + 1)) // (2 * (cw + 1))) << (8 * c)
        self.words = np.where(ok, new.astype(np.uint32), self.words)
        return int(ok.sum()), int(labelled.sum()), int(out_band.sum())

    def sample(self, xyz, min_weight=1):
        """xyz float32 [..., 3] -> rgba uint8 [..., 4]"""
        p = np.asarray(xyz, F)
        shape = p.shape[:-1]
        p = p.reshape(-1, 3)
        n = np.array(self.n, np.int64); o = self.origin
        ok = np.ones(len(p), bool)
        b, fi = [], []
        with np.errstate(all="ignore"):
            for a in range(3):
                u = p[:, a] / self.voxel
                u = u - F(0.5)
                fl = np.floor(u)
                f = u - fl
                assert f.dtype == F
                ok &= _finite(p[:, a]) & (fl >= F(-4194304.0)) & (fl <= F(4194303.0))
                b.append(fl); fi.append(np.floor(f * F(256.0)))
        b = [np.where(ok, b[a], 0).astype(np.int64) for a in range(3)]
        fi = [np.where(ok, fi[a], 0).astype(np.int64) for a in range(3)]
        S = np.zeros(len(p), np.int64); C = [np.zeros(len(p), np.int64) for _ in range(3)]
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    off = (dx, dy, dz)
                    g = [b[a] + off[a] for a in range(3)]
                    inside = ok.copy()
                    wgt = np.ones(len(p), np.int64)
                    for a in range(3):
                        inside &= (g[a] >= o[a]) & (g[a] < o[a] + n[a])
                        wgt = wgt * (fi[a] if off[a] else 256 - fi[a])
                    word = self.words[np.where(inside, g[2], o[2]) % n[2], np.where(inside, g[1], o[1]) % n[1], np.where(inside, g[0], o[0]) % n[0]].astype(np.int64)
                    counts = inside & ((word >> 24) >= int(min_weight))
                    wgt = np.where(counts, wgt, 0)
                    S += wgt
                    for c in range(3):
                        C[c] += wgt * ((word >> (8 * c)) & 0xFF)
        Sd = np.where(S == 0, 1, S)
        out = np.zeros((len(p), 4), np.uint8)
        for c in range(3):
            out[:, c] = np.where(S == 0, 0, (2 * C[c] + S) // (2 * Sd))
        out[:, 3] = np.where(S == 0, 0, np.maximum(1, (255 * S + (1 << 23)) >> 24))
        return out.reshape(shape + (4,))

    def render(self, depth, K4, T, min_weight=1):
        """depth float32 [H, W] -> (rgba uint8 [H, W, 4], (pixels coloured, pixels with depth but no colour))"""
        depth = np.asarray(depth, F)
        H, W = depth.shape
        fx, fy, cx, cy = (F(v) for v in K4)
        T = np.asarray(T, F).reshape(4, 4)
        with np.errstate(all="ignore"):
            c = [-((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3]) for a in range(3)]
            x = np.broadcast_to(np.arange(W).astype(F)[None, :], (H, W)); y = np.broadcast_to(np.arange(H).astype(F)[:, None], (H, W))
            dx = (x - cx) / fx; dy = (y - cy) / fy
            r = [(T[0, a] * dx + T[1, a] * dy) + T[2, a] for a in range(3)]
            has = _finite(depth) & (depth > F(0))
            p = np.stack([c[a] + depth * r[a] for a in range(3)], -1)
            assert p.dtype == F
        p = np.where(has[..., None], p, F(np.nan))
        rgba = self.sample(p, min_weight)
        col = rgba[..., 3] != 0
        return rgba, (int(col.sum()), int((has & ~col).sum()))
