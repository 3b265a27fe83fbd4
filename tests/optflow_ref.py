"""The dense optical-flow contract of include/vdo_slam_hip.h (vdo_optflow_compute) restated in NumPy: 2 x 2 mean pyramid, 9 x 7 census per level,
coarse-to-fine block search over the census words with the packed-key argmin, 3 x 3 median between levels, integer sub-pixel at level 0 and the
forward-backward check.  Integer arithmetic throughout; written from the contract's text.  Arrays are [H, W] / [H, W, 2] (u then v)."""
import numpy as np

from tests.stereo_ref import CENSUS_OFFSETS  # noqa: F401  (the census is the stereo section's step 1)

DEFAULTS = dict(levels=6, radius=2, window=2, median=1, fb_max_diff=1, subpixel=1)


def census(img):
    """uint64 [H, W]: the stereo contract's census, restated here on its own (tests/test_optflow_ref.py compares it with tests/stereo_ref.py)"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((H, W), np.uint64)
    k = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            out |= (img[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)] < img).astype(np.uint64) << np.uint64(k)
            k += 1
    return out


def level_sizes(W, H, levels):
    """[(W_l, H_l)]: level l + 1 is (ceil(W_l / 2), ceil(H_l / 2))"""
    out = [(int(W), int(H))]
    for _ in range(1, levels):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def downsample(a):
    """(a + b + c + d + 2) >> 2 over the 2 x 2 block at (2x, 2y), the + 1 coordinates clamped"""
    a = np.asarray(a, np.int64)
    H, W = a.shape
    ys, xs = 2 * np.arange((H + 1) // 2), 2 * np.arange((W + 1) // 2)
    y1, x1 = np.minimum(ys + 1, H - 1), np.minimum(xs + 1, W - 1)
    s = a[ys][:, xs] + a[ys][:, x1] + a[y1][:, xs] + a[y1][:, x1]
    return ((s + 2) >> 2).astype(np.uint8)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, levels):
        out.append(downsample(out[-1]))
    return out


def candidates(r):
    """[(du, dv)] in rank order k = 0, 1, ...: ascending (du^2 + dv^2, dv, du)"""
    return sorted(((du, dv) for dv in range(-r, r + 1) for du in range(-r, r + 1)), key=lambda c: (c[0] * c[0] + c[1] * c[1], c[1], c[0]))


def _popcount64(v):
    return np.bitwise_count(v).astype(np.int64)


def block_costs(c0, c1, prior, r, w):
    """A [K, H, W] int64: the block sum of every candidate, the centre pixel's prior moving the whole block"""
    H, W = c0.shape
    ys, xs = np.mgrid[0:H, 0:W]
    u0, v0 = prior[..., 0].astype(np.int64), prior[..., 1].astype(np.int64)
    cand = candidates(r)
    A = np.zeros((len(cand), H, W), np.int64)
    for j in range(-w, w + 1):
        for i in range(-w, w + 1):
            a = c0[np.clip(ys + j, 0, H - 1), np.clip(xs + i, 0, W - 1)]
            for k, (du, dv) in enumerate(cand):
                b = c1[np.clip(ys + j + v0 + dv, 0, H - 1), np.clip(xs + i + u0 + du, 0, W - 1)]
                A[k] += _popcount64(a ^ b)
    return A


def median3(F):
    """Each component replaced by the fifth of the nine sorted values of its clamped 3 x 3 neighbourhood"""
    H, W = F.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    nb = np.stack([F[np.clip(ys + j, 0, H - 1), np.clip(xs + i, 0, W - 1)] for j in (-1, 0, 1) for i in (-1, 0, 1)])
    return np.sort(nb, axis=0)[4]


def _subpixel_offset(Am, A0, Ap, inner):
    den = Am + Ap - 2 * A0
    num = 128 * (Am - Ap)
    use = inner & (den > 0)
    den1 = np.where(use, den, 1)
    return np.where(use, np.sign(num) * ((2 * np.abs(num) + den1) // (2 * den1)), 0)


def search(cen0, cen1, r, w, median, subpixel):
    """Steps 3 and 4 from image 0 to image 1 over the census pyramids: (per-level integer flows [level] -> [H_l, W_l, 2] int32 as the level below
    reads them, offsets [H, W, 2] int64 of level 0 in 1/256 px)"""
    L = len(cen0)
    cand = candidates(r)
    cd = np.array(cand, np.int64)
    rank = np.zeros((2 * r + 1, 2 * r + 1), np.int64)               # rank[dv + r, du + r]
    rank[cd[:, 1] + r, cd[:, 0] + r] = np.arange(len(cand))
    flows = [None] * L
    off = None
    for l in range(L - 1, -1, -1):
        H, W = cen0[l].shape
        if l == L - 1:
            prior = np.zeros((H, W, 2), np.int64)
        else:
            ys, xs = np.mgrid[0:H, 0:W]
            prior = 2 * flows[l + 1][ys >> 1, xs >> 1].astype(np.int64)
        A = block_costs(cen0[l], cen1[l], prior, r, w)
        assert A.max() <= 62 * 81
        key = (A << 8) | np.arange(len(cand), dtype=np.int64)[:, None, None]
        ks = key.argmin(axis=0)
        d = cd[ks]                                                   # [H, W, 2]: (du*, dv*)
        F = (prior + d).astype(np.int32)
        if l == 0:
            off = np.zeros((H, W, 2), np.int64)
            if subpixel:
                A0 = np.take_along_axis(A, ks[None], 0)[0]
                for comp in (0, 1):
                    inner = np.abs(d[..., comp]) < r
                    lo, hi = d.copy(), d.copy()                      # the two neighbours along this component (clipped where there is none: unused)
                    lo[..., comp] = np.maximum(lo[..., comp] - 1, -r); hi[..., comp] = np.minimum(hi[..., comp] + 1, r)
                    Am = np.take_along_axis(A, rank[lo[..., 1] + r, lo[..., 0] + r][None], 0)[0]
                    Ap = np.take_along_axis(A, rank[hi[..., 1] + r, hi[..., 0] + r][None], 0)[0]
                    off[..., comp] = _subpixel_offset(Am, A0, Ap, inner)
        elif median:
            F = median3(F)
        flows[l] = F
    return flows, off


def stages(im0, im1, **prm):
    """Every stage of one compute: pyramid0 / pyramid1 / census0 / census1 (lists by level), forward / backward (lists of int32 [H_l, W_l, 2];
    backward is None with fb_max_diff = -1), flow float32 [H, W, 2], valid uint8 [H, W], n_valid"""
    p = dict(DEFAULTS); p.update(prm)
    L, r, w = p["levels"], p["radius"], p["window"]
    p0, p1 = pyramid(im0, L), pyramid(im1, L)
    c0, c1 = [census(a) for a in p0], [census(a) for a in p1]
    fwd, off = search(c0, c1, r, w, p["median"], p["subpixel"])
    H, W = p0[0].shape
    F = fwd[0].astype(np.int64)
    flow = ((256 * F + off).astype(np.float32) * np.float32(1.0 / 256.0)).astype(np.float32)
    bwd = None
    valid = np.ones((H, W), np.uint8)
    if p["fb_max_diff"] >= 0:
        bwd, _ = search(c1, c0, r, w, p["median"], 0)
        ys, xs = np.mgrid[0:H, 0:W]
        xp, yp = xs + F[..., 0], ys + F[..., 1]
        inside = (xp >= 0) & (xp < W) & (yp >= 0) & (yp < H)
        B = bwd[0][np.clip(yp, 0, H - 1), np.clip(xp, 0, W - 1)].astype(np.int64)
        diff = np.maximum(np.abs(F[..., 0] + B[..., 0]), np.abs(F[..., 1] + B[..., 1]))
        valid = (inside & (diff <= p["fb_max_diff"])).astype(np.uint8)
    return dict(pyramid0=p0, pyramid1=p1, census0=c0, census1=c1, forward=fwd, backward=bwd, flow=flow, valid=valid, n_valid=int(valid.sum()))


def compute(im0, im1, **prm):
    s = stages(im0, im1, **prm)
    return s["flow"], s["valid"], s["n_valid"]


# ---- the scenes of the accuracy conditions -------------------------------------------------------------------------------------------
def texture(seed, H, W, k):
    """k = 3 or 5: box-smoothed noise, (H + 64) x (W + 64)"""
    from numpy.lib.stride_tricks import sliding_window_view as swv
    t = np.random.default_rng(seed).integers(0, 256, (H + 64, W + 64)).astype(np.float64)
    t = swv(np.pad(t, k // 2, mode="edge"), (k, k)).mean((-1, -2))
    return t if k == 3 else (t - t.min()) / (t.max() - t.min()) * 255


def bil(T, ys, xs):
    """bilinear sample"""
    y0 = np.floor(ys).astype(int); x0 = np.floor(xs).astype(int); fy = ys - y0; fx = xs - x0
    return T[y0, x0] * (1 - fy) * (1 - fx) + T[y0, x0 + 1] * (1 - fy) * fx + T[y0 + 1, x0] * fy * (1 - fx) + T[y0 + 1, x0 + 1] * fy * fx


def shifted_pair(dx, dy, H=64, W=96, seed=0):
    """Condition A: I1 is I0 moved by the integer (dx, dy)"""
    big = np.clip(texture(seed, H, W, 3), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(big[32:32 + H, 32:32 + W]), np.ascontiguousarray(big[32 - dy:32 - dy + H, 32 - dx:32 - dx + W])


def two_motion_pair(seed, bg, ob, H=64, W=96):
    """Condition B: a rectangle moving by ob = (ox, oy) over a background moving by bg = (bx, by).  (I0, I1 uint8, truth [H, W, 2] float)"""
    (bx, by), (ox, oy) = bg, ob
    big = texture(seed, H, W, 5)
    tex2 = np.roll(big, (17, 23), (0, 1))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def rect(y, x):
        return (20 <= y) & (y < 44) & (30 <= x) & (x < 66)
    rect0, rect1 = rect(yy, xx), rect(yy - oy, xx - ox)
    I0 = np.rint(np.where(rect0, bil(tex2, yy + 32, xx + 32), bil(big, yy + 32, xx + 32)))
    I1 = np.rint(np.where(rect1, bil(tex2, yy + 32 - oy, xx + 32 - ox), bil(big, yy + 32 - by, xx + 32 - bx)))
    truth = np.where(rect0[..., None], np.array([ox, oy], np.float64), np.array([bx, by], np.float64))
    return I0.astype(np.uint8), I1.astype(np.uint8), truth
