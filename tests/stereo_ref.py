"""The stereo contract of include/vdo_slam_hip.h (vdo_stereo_compute) restated in NumPy: 9 x 7 census, Hamming cost, semi-global
aggregation over 4 / 8 paths, winner-takes-all with the uniqueness, left-right and sub-pixel rules.  Integer arithmetic throughout,
vectorised across the axis orthogonal to each path; tests/test_stereo_ref.py checks it against a per-pixel scalar transcription.
Arrays are [H, W] / [H, W, D]."""
import numpy as np

CENSUS_OFFSETS = [(dx, dy) for dy in range(-3, 4) for dx in range(-4, 5) if (dx, dy) != (0, 0)]      # raster order, bit k = k-th entry
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]                   # (dx, dy); predecessor of p is p - r
NO_COST = 62
INF = 1 << 30

DEFAULTS = dict(max_disparity=128, p1=10, p2=120, paths=8, uniqueness=5, lr_max_diff=1, subpixel=1)


def census(img):
    """uint64 [H, W]: bit k set iff the k-th window pixel (border clamped) is darker than the centre"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    pad = np.pad(img, ((3, 3), (4, 4)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for k, (dx, dy) in enumerate(CENSUS_OFFSETS):
        out |= (pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W] < img).astype(np.uint64) << np.uint64(k)
    return out


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _popcount64(v):
    return _POP8[np.ascontiguousarray(v).view(np.uint8).reshape(v.shape + (8,))].sum(axis=-1)


def cost_volume(cl, cr, D):
    """uint8 [H, W, D]: popcount(cL(x, y) ^ cR(x - d, y)), 62 where x - d < 0"""
    H, W = cl.shape
    C = np.full((H, W, D), NO_COST, np.uint8)
    for d in range(min(D, W)):
        C[:, d:, d] = _popcount64(cl[:, d:] ^ cr[:, :W - d])
    return C


def _step(c, prev, p1, p2):
    """One step of the recurrence for a batch of pixels: c, prev [n, D]"""
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, INF); lo[:, 1:] = prev[:, :-1]
    hi = np.full_like(prev, INF); hi[:, :-1] = prev[:, 1:]
    return c + np.minimum(np.minimum(prev, m + p2), np.minimum(lo, hi) + p1) - m


def aggregate_path(C, dx, dy, p1, p2):
    """L_r [H, W, D] int64 of one direction"""
    C = C.astype(np.int64)
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]
            continue
        prev = L[y - dy]
        if dx == 0:
            L[y] = _step(C[y], prev, p1, p2)
            continue
        L[y] = C[y]                                     # the column whose predecessor is outside keeps C
        if W > 1:
            if dx > 0: L[y, 1:] = _step(C[y, 1:], prev[:-1], p1, p2)
            else: L[y, :-1] = _step(C[y, :-1], prev[1:], p1, p2)
    return L


def aggregate(C, p1, p2, paths):
    """S = sum of L_r over the first `paths` directions, uint16 [H, W, D]"""
    S = np.zeros(C.shape, np.int64)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate_path(C, dx, dy, p1, p2)
    assert S.max() < 1 << 16
    return S.astype(np.uint16)


def right_disparity(S):
    """dR [H, W]: argmin over d with x' + d < W of S(x' + d, y, d), lowest d on ties"""
    H, W, D = S.shape
    R = np.full((H, W, D), INF, np.int64)
    for d in range(min(D, W)):
        R[:, :W - d, d] = S[:, d:, d]
    return R.argmin(axis=2)


def select(S, uniqueness, lr_max_diff, subpixel):
    """float32 [H, W]: 256 d* + off, or 0"""
    S = S.astype(np.int64)
    H, W, D = S.shape
    dstar = S.argmin(axis=2)
    s0 = np.take_along_axis(S, dstar[..., None], 2)[..., 0]
    x = np.arange(W)[None, :]
    ok = (dstar >= 1) & (x - dstar >= 0)
    if uniqueness > 0:
        far = np.abs(np.arange(D)[None, None, :] - dstar[..., None]) > 1
        s2 = np.where(far, S, INF).min(axis=2)
        ok &= (s2 == INF) | (100 * s0 < (100 - uniqueness) * s2)
    if lr_max_diff >= 0:
        dR = right_disparity(S)
        xr = np.clip(x - dstar, 0, W - 1)
        ok &= np.abs(np.take_along_axis(dR, xr, 1) - dstar) <= lr_max_diff
    off = np.zeros((H, W), np.int64)
    if subpixel:
        inner = (dstar >= 1) & (dstar <= D - 2)
        dm = np.clip(dstar - 1, 0, D - 1)[..., None]; dp = np.clip(dstar + 1, 0, D - 1)[..., None]
        sm = np.take_along_axis(S, dm, 2)[..., 0]; sp = np.take_along_axis(S, dp, 2)[..., 0]
        den = sm + sp - 2 * s0
        num = 128 * (sm - sp)
        use = inner & (den > 0)
        den1 = np.where(use, den, 1)
        off = np.where(use, np.sign(num) * ((2 * np.abs(num) + den1) // (2 * den1)), 0)
    return np.where(ok, 256 * dstar + off, 0).astype(np.float32)


def stages(left, right, **prm):
    """Every stage of one compute: dict with census_l, census_r, cost, aggregated, disparity256, n_valid"""
    p = dict(DEFAULTS); p.update(prm)
    cl, cr = census(left), census(right)
    C = cost_volume(cl, cr, p["max_disparity"])
    S = aggregate(C, p["p1"], p["p2"], p["paths"])
    out = select(S, p["uniqueness"], p["lr_max_diff"], p["subpixel"])
    return dict(census_l=cl, census_r=cr, cost=C, aggregated=S, disparity256=out, n_valid=int(np.count_nonzero(out)))


def compute(left, right, **prm):
    r = stages(left, right, **prm)
    return r["disparity256"], r["n_valid"]


def warp_right(left, disp, right):
    """Forward warp of `left` by the integer disparity map `disp` into `right` (modified in place) with a z-buffer: left pixel (x, y) lands on
    (x - disp, y), the larger disparity wins.  Returns visible [H, W]: the pixel's target is inside the image and it won the z-buffer."""
    H, W = left.shape
    zbuf = np.full((H, W), -1, np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    for d in np.unique(disp):                           # ascending: the larger disparity overwrites
        m = (disp == d) & (xs - d >= 0)
        right[ys[m], xs[m] - d] = left[m]
        zbuf[ys[m], xs[m] - d] = d
    xr = xs - disp
    return (xr >= 0) & (zbuf[ys, np.clip(xr, 0, W - 1)] == disp)


def scene(H, W, D, seed):
    """A textured rectified pair with known disparity: (left, right, gt [H, W] int, visible [H, W] bool).  The truth is a ramp
    D//4 .. D//2 down the image with a nearer box; right is noise overwritten by the forward warp of left (the nearer pixel wins)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W + D)).astype(np.float64)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0)) / 3
    left = base[:, :W].astype(np.uint8)
    gt = (D // 4 + (np.arange(H) * (D // 4)) // H)[:, None] * np.ones((1, W), np.int64)
    gt[H // 4:H // 2, W // 3:W // 2] = D // 2 + 3
    right = rng.integers(0, 256, (H, W)).astype(np.uint8)
    visible = warp_right(left, gt, right)
    return left, right, gt, visible


def recovery(out, gt, visible):
    """Share of the visible pixels that are valid and within 1 px of the truth"""
    good = (out > 0) & (np.abs(out / 256.0 - gt) <= 1.0)
    return float((good & visible).sum()) / float(visible.sum())
