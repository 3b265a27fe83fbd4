"""NumPy restatement of the raycaster's contract (include/vdo_slam_hip.h, "Raycaster", vdo_raycast_*) over dense_ref.Volume: float32 throughout, one
rounded operation per step in the header's order, vectorised over the pixels with a Python loop over the samples k.  It knows nothing of the
empty-space skipping.  The device must equal it bit for bit."""
import numpy as np

from tests.dense_ref import F, _finite


def _lerp(u, v, f):
    return u + f * (v - u)


class _Sampler:
    """The volume as the samples see it: bounds as floats, the eight corner words of a base cell, the trilinear value"""

    def __init__(self, vol, min_weight):
        self.vol = vol
        self.n = np.array(vol.n, np.int64)
        self.o = np.array(vol.origin, np.int64)
        self.lo = [F(int(self.o[a])) for a in range(3)]
        self.hi = [F(int(self.o[a] + self.n[a] - 2)) for a in range(3)]
        self.t = vol.t().astype(F)
        self.w = vol.w()
        self.min_weight = int(min_weight)

    def cell(self, g):
        """g: three float32 arrays (voxel coordinates) -> (b, f): the base cell as floats and the fractions"""
        b = [np.floor(g[a]) for a in range(3)]
        f = [g[a] - b[a] for a in range(3)]
        return b, f

    def in_bounds(self, b):
        ok = np.ones(b[0].shape, bool)
        for a in range(3):
            ok &= (self.lo[a] <= b[a]) & (b[a] <= self.hi[a])           # a NaN fails
        return ok

    def value(self, b, f, ok):
        """The trilinear form at base cell b (floats, used where ok) with the fractions f -> (valid, F, smallest corner weight)"""
        bi = [np.where(ok, b[a], self.lo[a]).astype(np.int64) for a in range(3)]
        s0 = [bi[a] % self.n[a] for a in range(3)]
        s1 = [(s0[a] + 1) % self.n[a] for a in range(3)]
        sx, sy, sz = (s0[0], s1[0]), (s0[1], s1[1]), (s0[2], s1[2])
        t = {}
        wmin = np.full(ok.shape, 1 << 20, np.int64)
        for k in (0, 1):
            for j in (0, 1):
                for i in (0, 1):
                    t[i, j, k] = self.t[sz[k], sy[j], sx[i]]
                    wmin = np.minimum(wmin, self.w[sz[k], sy[j], sx[i]])
        valid = ok & (wmin >= self.min_weight)
        a00 = _lerp(t[0, 0, 0], t[1, 0, 0], f[0]); a10 = _lerp(t[0, 1, 0], t[1, 1, 0], f[0])
        a01 = _lerp(t[0, 0, 1], t[1, 0, 1], f[0]); a11 = _lerp(t[0, 1, 1], t[1, 1, 1], f[0])
        b0 = _lerp(a00, a10, f[1]); b1 = _lerp(a01, a11, f[1])
        val = _lerp(b0, b1, f[2])
        assert val.dtype == F
        return valid, val, wmin


def render(vol, width, height, K4, near, step, n_steps, min_weight, T):
    """-> (depth float32 [H, W], grad float32 [H, W, 3], weight int32 [H, W], counts (hit, missed, no valid sample))"""
    W, H = int(width), int(height)
    fx, fy, cx, cy = (F(v) for v in K4)
    near, step, voxel = F(near), F(step), F(vol.voxel)
    T = np.asarray(T, F).reshape(4, 4)
    S = _Sampler(vol, min_weight)
    with np.errstate(all="ignore"):
        c = [-((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3]) for a in range(3)]
        x = np.broadcast_to(np.arange(W).astype(F)[None, :], (H, W)); y = np.broadcast_to(np.arange(H).astype(F)[:, None], (H, W))
        dx = (x - cx) / fx; dy = (y - cy) / fy
        r = [(T[0, a] * dx + T[1, a] * dy) + T[2, a] for a in range(3)]
        assert all(v.dtype == F for v in r) and all(np.asarray(v).dtype == F for v in c)

        def sample(lam):
            g = [(c[a] + lam * r[a]) / voxel - F(0.5) for a in range(3)]
            b, f = S.cell(g)
            ok = _finite(g[0]) & _finite(g[1]) & _finite(g[2]) & S.in_bounds(b)
            return g, b, f, ok

        depth = np.zeros((H, W), F); weight = np.zeros((H, W), np.int32)
        done = np.zeros((H, W), bool); any_valid = np.zeros((H, W), bool)
        pv = np.zeros((H, W), bool); pF = np.zeros((H, W), F)
        for k in range(int(n_steps)):
            lam = near + F(k) * step
            _, b, f, ok = sample(lam)
            v, Fk, wmin = S.value(b, f, ok)
            any_valid |= v
            if k >= 1:
                hit = ~done & pv & v & (pF > F(0)) & (Fk <= F(0))
                lam0 = near + F(k - 1) * step
                d = lam0 + step * (pF / (pF - Fk))
                depth = np.where(hit, d, depth).astype(F)
                weight = np.where(hit, wmin, weight).astype(np.int32)
                done |= hit
            pv, pF = v, Fk
            if done.all():
                break
        # the gradient at the hit point: central differences of the trilinear form, base cells b +- e_a, the fractions of b
        g = [(c[a] + depth * r[a]) / voxel - F(0.5) for a in range(3)]
        b, f = S.cell(g)
        ok = done & _finite(g[0]) & _finite(g[1]) & _finite(g[2]) & S.in_bounds(b)
        good, _, _ = S.value(b, f, ok)
        comp = []
        for a in range(3):
            side = []
            for sgn in (F(1), F(-1)):
                bb = list(b); bb[a] = b[a] + sgn
                v, val, _ = S.value(bb, f, ok & S.in_bounds(bb))
                good = good & v
                side.append(val)
            comp.append(side[0] - side[1])
        grad = np.stack([np.where(good, comp[a], F(0)) for a in range(3)], -1).astype(F)
    n_hit = int(done.sum()); n_miss = int((~done & any_valid).sum())
    return depth, grad, weight, (n_hit, n_miss, W * H - n_hit - n_miss)


def normals(grad):
    """The gradient image normalised in float64 and narrowed, or 0 - what a saved map holds beside a point (dense_ref.normals), per pixel"""
    g = np.asarray(grad, np.float64)
    n = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2])
    with np.errstate(all="ignore"):
        out = np.where(n[..., None] > 0, g / n[..., None], 0.0)
    return out.astype(F)
