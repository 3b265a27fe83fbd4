"""Plain NumPy restatements (np.float32 / np.int32) of the image-indexing operations of Frame::Frame and Tracking, written from the
reference's statements, plus the constructive inputs that tests/test_frame_envelope_gpu.py and tests/test_tracking_envelope_gpu.py
share.  The restatements are checked against the CPU oracle without a GPU (the ``not gpu`` tests of those two files).

Every float position built here is finite and far below 2^30: ``(int)`` of anything else is undefined in the reference."""
import functools

import numpy as np

F = np.float32
TH_BG, TH_OBJ = F(40.0), F(25.0)
# the depth values every K1 / ingest case carries: negative, both zeros, inf, NaN, the largest finite float, 1e-30
SPECIAL_DEPTH = np.array([-1.0, -0.0, 0.0, np.inf, np.nan, np.finfo(np.float32).max, 1e-30, -np.inf, 1.0, 5000.0, 65535.0, 0.5], np.float32)


def bits_equal(a, b):
    """Same bit patterns wherever ``b`` (the reference) is not NaN, NaN wherever it is."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def raw_depth(n, seed):
    """n raw depth values: the special ones first (as many as fit), then plausible 16-bit disparities with a few negatives."""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 60000, n).astype(np.float32)
    d[rng.random(n) < 0.1] *= F(-1)
    k = min(n, SPECIAL_DEPTH.size)
    d[:k] = SPECIAL_DEPTH[:k]
    if n > 300:                       # and once more behind the first workgroup / in the tail
        d[n - k:] = SPECIAL_DEPTH[:k][::-1]
    return d


# ---- K1 / ingest (src/Tracking.cc:180-204): d < 0 -> 0, else bf / (d / factor), two fp32 divisions ---------------------------
def depth_preprocess(d, bf, factor):
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        return np.where(d < 0, F(0), F(bf) / (d / F(factor))).astype(np.float32)


def ingest(depth, flow, mask, bf, factor, convert):
    return (depth_preprocess(depth, bf, factor) if convert else np.array(depth, np.float32)), np.array(flow, np.float32), np.array(mask, np.int32)


# ---- K2: cvtColor 8u, (R*4899 + G*9617 + B*1868 + 8192) >> 14 ----------------------------------------------------------------
def rgb2gray(img, rgb_order=True):
    p = np.asarray(img, np.uint8).astype(np.int32)
    r, g, b = (p[..., 0], p[..., 1], p[..., 2]) if rgb_order else (p[..., 2], p[..., 1], p[..., 0])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def gray_step_pixels():
    """(r, g, b) whose weighted sum sits exactly ON a step of the >> 14 (residue 0) or one short of it (residue 16383): brute force over
    all 2^24 colours, a few hundred of each kept, (255, 255, 255) among them (4899 + 9617 + 1868 = 16384: residue 8192 - the rounding
    constant alone - is the white pixel's; it is added by hand)."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    on, short = [], []
    for r in range(256):
        res = (r * 4899 + g * 9617 + b * 1868 + 8192) & 16383
        for lst, val in ((on, 0), (short, 16383)):
            gg, bb = np.nonzero(res == val)
            lst += [(r, int(x), int(y)) for x, y in zip(gg[:3], bb[:3])]
    px = np.array(on + short + [(0, 0, 0), (255, 255, 255)], np.uint8)
    assert len(on) > 100 and len(short) > 100
    return px


# ---- K9 (src/Frame.cc:100-128 ORB branch, :132-166 sampled branch, depth gather :178-194) -----------------------------------
def static_filter(kx, ky, mask, depth, flow, th, sampled):
    kx, ky = np.asarray(kx, np.float32), np.asarray(ky, np.float32)
    h, w = mask.shape
    x, y = kx.astype(np.int32), ky.astype(np.int32)
    d = depth[y, x]
    fx, fy = flow[y, x, 0], flow[y, x, 1]
    keep = (mask[y, x] == 0) & ~((d > F(th)) | (d <= 0)) & (fx != 0) & (fy != 0)
    cx, cy = kx + fx, ky + fy
    if sampled:
        keep &= (cx < F(w)) & (cy < F(h)) & (cx > 0) & (cy > 0)
    else:
        keep &= (cx < F(w)) & (cy < F(h)) & (kx < F(w)) & (ky < F(h))
    idx = np.nonzero(keep)[0].astype(np.int32)
    return dict(keep_idx=idx, corr_x=cx[idx], corr_y=cy[idx], flow_x=fx[idx], flow_y=fy[idx], depth=np.where(d[idx] > 0, d[idx], F(-1)).astype(np.float32))


# ---- K10 (src/Frame.cc:201-228): every step-th pixel in raster order --------------------------------------------------------
def object_sample(mask, depth, flow, th, step=4):
    h, w = mask.shape
    ii, jj = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    d, lab = depth[ii, jj], mask[ii, jj]
    fx, fy = flow[ii, jj, 0], flow[ii, jj, 1]
    cx, cy = jj.astype(np.float32) + fx, ii.astype(np.float32) + fy
    keep = (lab != 0) & (d < F(th)) & (d > 0) & (cx < F(w)) & (cx > 0) & (cy < F(h)) & (cy > 0)
    k = np.nonzero(keep)[0]
    return dict(key_x=jj[k].astype(np.float32), key_y=ii[k].astype(np.float32), corr_x=cx[k], corr_y=cy[k], flow_x=fx[k], flow_y=fy[k],
                depth=d[k], label=lab[k].astype(np.int32))


# ---- K11 (src/Tracking.cc:259-305) and the label gather of UpdateMask (:3015-3040) ------------------------------------------
def gather(mode, kx, ky, depth, mask, th=TH_OBJ):
    """mode 0: static depth (-1 when outside / not positive); mode 1: object (depth, label) or (0.1, 0); mode 2: label or -1."""
    h, w = mask.shape
    u, v = np.asarray(kx, np.float32).astype(np.int32), np.asarray(ky, np.float32).astype(np.int32)
    if mode == 2:
        inside = (u < w) & (u > 0) & (v < h) & (v > 0)
    else:
        inside = (u < w - 1) & (u > 0) & (v < h - 1) & (v > 0)
    uc, vc = np.where(inside, u, 0), np.where(inside, v, 0)
    d, lab = depth[vc, uc], mask[vc, uc]
    if mode == 0:
        return np.where(inside & (d > 0), d, F(-1)).astype(np.float32)
    if mode == 1:
        ok = inside & (d < F(th)) & (d > 0)
        return np.where(ok, d, F(0.1)).astype(np.float32), np.where(ok, lab, 0).astype(np.int32)
    return np.where(inside, lab, -1).astype(np.int32)


# ---- the warp of one label (src/Tracking.cc:3045-3065) -----------------------------------------------------------------------
def mask_warp(mask_last, flow_last, lab, mask_cur):
    h, w = mask_last.shape
    out = np.array(mask_cur, np.int32)
    j, k = np.nonzero(mask_last == lab)
    fx, fy = flow_last[j, k, 0].astype(np.int32), flow_last[j, k, 1].astype(np.int32)
    ok = (k + fx < w) & (k + fx > 0) & (j + fy < h) & (j + fy > 0)
    out[(j + fy)[ok], (k + fx)[ok]] = lab
    return out


# =============================================================================================================================
# constructive inputs
# =============================================================================================================================
def below(v):
    return np.nextafter(F(v), F(-np.inf))


def above(v):
    return np.nextafter(F(v), F(np.inf))


def flow_landing(j, target):
    """fx with float(j) + fx == target exactly (asserted): target and j are multiples of ulp(target) and |target - j| <= max(|target|, j)."""
    fx = F(target) - F(j)
    assert F(j) + fx == F(target) and np.isfinite(fx)
    return fx


def flow_just_inside_zero(j):
    """fx with float(j) + fx the smallest positive sum there is: the smallest float for j == 0, else the neighbour of -j towards zero."""
    fx = above(0.0) if j == 0 else np.nextafter(F(-j), F(0))
    assert F(j) + fx > 0 and (j == 0 or F(j) + np.nextafter(fx, F(-np.inf)) == 0)
    return fx


# K10 probe categories: (kept?, what it pins)
K10_CATS = [
    (1, "positive label, interior"), (0, "mask 0"), (1, "negative label"), (0, "depth == th_obj"), (1, "depth just below th_obj"),
    (0, "depth 0"), (0, "depth negative"), (0, "j + fx == 0"), (1, "j + fx just above 0"), (0, "j + fx == w"), (1, "j + fx just below w"),
    (0, "i + fy == 0"), (1, "i + fy just above 0"), (0, "i + fy == h"), (1, "i + fy just below h"),
]


def k10_image(w, h, step, th=TH_OBJ):
    """Image whose probe p (raster order over the probes) is of category p % 15.  Returns mask, depth, flow, expected kept count."""
    mask = np.zeros((h, w), np.int32); depth = np.full((h, w), 10.0, np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 0.5, 0.25
    mask[:] = 3                                             # off-probe pixels are object too: only the probes may be read
    kept = 0
    p = 0
    for i in range(0, h, step):
        for j in range(0, w, step):
            c = p % len(K10_CATS)
            kept += K10_CATS[c][0]
            mask[i, j] = 1 + p % 7
            if c == 1: mask[i, j] = 0
            elif c == 2: mask[i, j] = -1 - p % 3
            elif c == 3: depth[i, j] = th
            elif c == 4: depth[i, j] = below(th)
            elif c == 5: depth[i, j] = 0.0
            elif c == 6: depth[i, j] = -3.0
            elif c == 7: flow[i, j, 0] = flow_landing(j, 0.0)
            elif c == 8: flow[i, j, 0] = flow_just_inside_zero(j)
            elif c == 9: flow[i, j, 0] = flow_landing(j, w)
            elif c == 10: flow[i, j, 0] = flow_landing(j, below(w))
            elif c == 11: flow[i, j, 1] = flow_landing(i, 0.0)
            elif c == 12: flow[i, j, 1] = flow_just_inside_zero(i)
            elif c == 13: flow[i, j, 1] = flow_landing(i, h)
            elif c == 14: flow[i, j, 1] = flow_landing(i, below(h))
            p += 1
    return mask, depth, flow, kept


K10_SHAPES = [(1242, 375, 4), (640, 480, 4), (61, 37, 1), (61, 37, 2), (61, 37, 3), (61, 37, 5), (61, 37, 7), (64, 64, 1), (4, 4, 4), (1, 1, 4)]


def k10_count_image(kept):
    """512 x 320, all object, step 4 = 10 240 probes; exactly ``kept`` of them left on (the others switched off through their depth).
    The probes that stay on are spread over the whole image: probe p stays iff p * kept // 10240 changes at p."""
    w, h, step = 512, 320, 4
    mask = np.full((h, w), 2, np.int32); depth = np.zeros((h, w), np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 0.5, 0.75
    depth[:] = 7.0                                          # off-probe pixels would be kept: only the probes may be read
    n = (w // step) * (h // step)
    p = np.arange(n, dtype=np.int64)
    on = ((p + 1) * kept // n) != (p * kept // n)
    assert int(on.sum()) == kept
    pr = depth[::step, ::step]
    pr[~on.reshape(h // step, w // step)] = 0.0
    pr[on.reshape(h // step, w // step)] = (1.0 + (p[on] % 97) * 0.125).astype(np.float32)
    return mask, depth, flow


def k10_big_image():
    """2048 x 2052 at step 4: 512 x 513 = 262 656 probes = 1026 workgroups of 256 - the scan of the workgroup counts runs a second
    chunk with a carry.  Kept probes only in workgroups 0, 1023, 1024 and 1025 (the last)."""
    w, h, step = 2048, 2052, 4
    ncol = w // step
    mask = np.zeros((h, w), np.int32); depth = np.full((h, w), 5.0, np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 1.5, 0.5
    probes = []
    for blk, offs in ((0, (0, 63, 64, 255)), (1023, (0, 1, 255)), (1024, (0, 100, 255)), (1025, (0, 64, 255))):
        probes += [blk * 256 + o for o in offs]
    for k, p in enumerate(probes):
        i, j = (p // ncol) * step, (p % ncol) * step
        mask[i, j] = 1 + k
        depth[i, j] = 2.0 + k
    return mask, depth, flow, probes


# K9: n points on distinct pixels (while they last), pixel index q = i % (w*h) -> (q % w, q // w), sub-pixel offset (.25, .5)
K9_N = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000]
K9_PATTERNS = ["all", "none", "alternating", "last_of_wave", "first_of_chunk", "random"]


def k9_keep_pattern(name, n):
    i = np.arange(n)
    if name == "all": return np.ones(n, bool)
    if name == "none": return np.zeros(n, bool)
    if name == "alternating": return i % 2 == 0
    if name == "last_of_wave": return i % 64 == 63
    if name == "first_of_chunk": return i % 1024 == 0
    return np.random.default_rng(n).random(n) < 0.5


def k9_case(w, h, n, pattern):
    """Points + images under them that realise the keep pattern: a dropped point i is dropped through (i % 4) mask != 0, depth 0,
    depth above the threshold, fx == 0.  Returns kx, ky, mask, depth, flow, keep (bool per point)."""
    assert n <= w * h
    keep = k9_keep_pattern(pattern, n)
    q = np.arange(n)
    x, y = q % w, q // w
    mask = np.full((h, w), 9, np.int32); depth = np.full((h, w), 12.0, np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = -0.125, 0.125
    mask[y, x] = 0
    depth[y, x] = (1.0 + (q % 311) * 0.125).astype(np.float32)              # <= 39.75 < th_depth = 40
    flow[y, x, 0] = np.where(x > w // 2, -1.5, 0.375 + (q % 5)).astype(np.float32)   # lands inside on every side
    flow[y, x, 1] = np.where(y > h // 2, -2.25, 0.5 + (q % 3)).astype(np.float32)
    dr = ~keep
    why = q % 4
    s = dr & (why == 0); mask[y[s], x[s]] = 4
    s = dr & (why == 1); depth[y[s], x[s]] = 0.0
    s = dr & (why == 2); depth[y[s], x[s]] = 40.5
    s = dr & (why == 3); flow[y[s], x[s], 0] = 0.0
    kx, ky = (x + 0.25).astype(np.float32), (y + 0.5).astype(np.float32)
    return kx, ky, mask, depth, flow, keep


def k9_boundary_case(w=320, h=200, th=TH_BG):
    """One point per boundary row.  Returns kx, ky, mask, depth, flow, names, kept-in-ORB-branch, kept-in-sampled-branch."""
    mask = np.zeros((h, w), np.int32); depth = np.full((h, w), 10.0, np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 0.5, 0.5
    rows = []

    def add(name, x, y, orb, smp, d=None, fx=None, fy=None, sub=(0.0, 0.0)):
        if d is not None: depth[y, x] = d
        if fx is not None: flow[y, x, 0] = fx
        if fy is not None: flow[y, x, 1] = fy
        rows.append((name, F(x + sub[0]), F(y + sub[1]), orb, smp))

    add("interior", 10, 10, 1, 1)
    add("depth == th", 20, 10, 1, 1, d=th)
    add("depth just above th", 30, 10, 0, 0, d=above(th))
    add("depth 0", 40, 10, 0, 0, d=0.0)
    add("depth negative", 50, 10, 0, 0, d=-2.0)
    add("fx == 0, fy != 0", 60, 10, 0, 0, fx=0.0)
    add("fx != 0, fy == 0", 70, 10, 0, 0, fy=0.0)
    add("fx == -0.0", 75, 10, 0, 0, fx=-0.0)
    add("px + fx == w", 300, 20, 0, 0, fx=flow_landing(300, w))
    add("px + fx just below w", 301, 20, 1, 1, fx=flow_landing(301, below(w)))
    add("px + fx < 0", 5, 20, 1, 0, fx=-9.5)
    add("px + fx == 0", 6, 20, 1, 0, fx=flow_landing(6, 0.0))
    add("px + fx just above 0", 7, 20, 1, 1, fx=flow_just_inside_zero(7))
    add("py + fy == h", 100, 190, 0, 0, fy=flow_landing(190, h))
    add("py + fy just below h", 101, 190, 1, 1, fy=flow_landing(190, below(h)))
    add("py + fy < 0", 102, 3, 1, 0, fy=-7.25)
    add("py + fy == 0", 103, 3, 1, 0, fy=flow_landing(3, 0.0))
    add("sub-pixel: px + fx == w", 310, 30, 0, 0, fx=flow_landing(310.5, w), sub=(0.5, 0.0))
    add("mask != 0", 110, 30, 0, 0)
    mask[30, 110] = 2
    names = [r[0] for r in rows]
    kx = np.array([r[1] for r in rows], np.float32); ky = np.array([r[2] for r in rows], np.float32)
    return kx, ky, mask, depth, flow, names, np.array([r[3] for r in rows], bool), np.array([r[4] for r in rows], bool)


# K11 / mask_at: positions around every bound
def _at(t, frac):
    """a float whose (int) is t: t + frac for t >= 0, t - frac below (truncation is towards zero)."""
    return t + frac if t >= 0 else t - frac


def gather_points(w, h, n, seed=0):
    """n positions: the cross product of truncated coordinates {-1, 0, 1, w-2, w-1, w} x {-1, 0, 1, h-2, h-1, h}, the fractional edge
    values -0.5 (truncates to 0) / 0.999 / w-1+0.999 (truncates to w-1), then uniform ones over [-2, w+2) x [-2, h+2); a spread of the
    special ones when n is smaller than their number."""
    xs = sorted({-1, 0, 1, w - 2, w - 1, w}); ys = sorted({-1, 0, 1, h - 2, h - 1, h})
    pts = [(_at(x, 0.25), _at(y, 0.5)) for x in xs for y in ys]
    pts += [(-0.5, 1.0), (1.0, -0.5), (0.999, 1.0), (1.0, 0.999), (w - 1 + 0.999, 1.0), (1.0, h - 1 + 0.999), (-0.5, -0.5), (w - 1 + 0.999, h - 1 + 0.999),
            (w - 1 + 0.999, h - 1.5), (w - 1.5, h - 1 + 0.999)]
    rng = np.random.default_rng(seed)
    kx = np.array([p[0] for p in pts], np.float32); ky = np.array([p[1] for p in pts], np.float32)
    assert F(w - 1 + 0.999) < w and F(h - 1 + 0.999) < h
    if n > kx.size:
        kx = np.concatenate([kx, rng.uniform(-2, w + 2, n - kx.size).astype(np.float32)])
        ky = np.concatenate([ky, rng.uniform(-2, h + 2, n - ky.size).astype(np.float32)])
    else:
        pick = np.linspace(0, kx.size - 1, n).astype(int)
        kx, ky = kx[pick], ky[pick]
    return kx, ky


def gather_images(w, h, seed=0, th=TH_OBJ):
    """Labels on every pixel (so that a wrong bound shows), depth with 0 / negative / exactly th / just below th sprinkled in."""
    rng = np.random.default_rng(seed)
    mask = rng.integers(1, 9, (h, w)).astype(np.int32)
    depth = rng.uniform(1, 30, (h, w)).astype(np.float32)
    r = rng.random((h, w))
    depth[r < 0.1] = 0.0; depth[(r >= 0.1) & (r < 0.2)] = -1.5; depth[(r >= 0.2) & (r < 0.3)] = th; depth[(r >= 0.3) & (r < 0.4)] = below(th)
    return mask, depth


# ---- the single-label warp at its bounds -----------------------------------------------------------------------------------
def warp_case(w, h=120, lab=4):
    """Last mask / flow / current mask with hand-placed pixels of ``lab``; returns also the pixels that must carry ``lab`` afterwards
    and the ones that must not (the current mask is 0 / 6 there before)."""
    rng = np.random.default_rng(w)
    last = np.zeros((h, w), np.int32); flow = rng.uniform(-30, 30, (h, w, 2)).astype(np.float32)
    cur = rng.integers(0, 3, (h, w)).astype(np.int32) * 6                       # 0, 6, 12
    last[60:90, 40:90] = lab; last[70:100, 100:130] = lab + 2                   # a blob of the label and one of another label (stays)
    must, must_not = [], []

    def put(j, k, fx, fy, land, kept):
        last[j, k] = lab; flow[j, k] = (fx, fy)
        (must if kept else must_not).append(land)

    put(10, 5, -0.7, 0.0, (10, 5), True)                 # (int)-0.7 = 0
    put(10, 9, -1.2, 0.0, (10, 8), True)                 # (int)-1.2 = -1
    put(20, 7, -7.0, 0.0, (20, 0), False)                # column 0: dropped
    put(21, 7, -6.5, 0.0, (21, 1), True)
    put(30, w - 5, 4.9, 0.0, (30, w - 1), True)          # column w-1: kept
    put(31, w - 5, 5.0, 0.0, None, False)                # column w: dropped (nothing to look at)
    put(3, 50, 0.0, -3.0, (0, 50), False)                # row 0: dropped
    put(3, 52, 0.0, -2.99, (1, 52), True)
    put(h - 4, 60, 0.0, 3.5, (h - 1, 60), True)          # row h-1: kept
    put(h - 4, 62, 0.0, 4.0, None, False)                # row h: dropped
    put(0, 70, 0.0, 5.0, (5, 70), True)                  # a SOURCE pixel on row 0 / column 0 is fine
    put(50, 0, 3.0, 0.0, (50, 3), True)
    for p in must + [q for q in must_not if q]:
        cur[p] = 6
    return last, flow, cur, must, [q for q in must_not if q]


# ---- UpdateMask scenes ------------------------------------------------------------------------------------------------------
CELL_W, CELL_H, BAND = 12, 10, 60            # a label = one 12 x 10 block (120 pixels = 120 samples); targets lie BAND rows below
LAB_X, LAB_Y = 900, 901                      # current-mask labels that no sample carries


def slot_label(s):
    return 3 + 7 * s


class MaskScene:
    """``n_labels`` last-frame labels slot_label(0..n-1), each a 12 x 10 block in the upper band of the image, warped by a per-label flow
    onto a target area in the lower band; one sample per block pixel, at its flowed position.  The current mask carries label s on the
    target area of s unless s is in ``dropped``; ``paint[s]`` then repaints the columns of s's target area, left to right, with
    (label or None = leave, number of columns); ``target[s]`` = (cell, column shift) moves the target area of s (default: cell s);
    ``outside[s]`` samples of s are moved out of the image.  Samples arrive shuffled."""

    def __init__(self, w, n_labels, dropped=(), paint=None, target=None, outside=None, h=120, seed=0):
        ncx = (w - 2) // CELL_W
        assert n_labels <= 65 and ncx * 5 >= 73 and 70 % ncx <= ncx - 3
        self.w, self.h, self.n = w, h, n_labels
        self.last = np.zeros((h, w), np.int32); self.cur = np.zeros((h, w), np.int32); self.flow = np.zeros((h, w, 2), np.float32)
        self.depth = np.full((h, w), 10.0, np.float32)
        target, paint, outside = dict(target or {}), dict(paint or {}), dict(outside or {})
        sl, cx, cy, kx, ky = [], [], [], [], []
        self.area = {}
        for s in range(n_labels):
            bx, by = 1 + (s % ncx) * CELL_W, 1 + (s // ncx) * CELL_H
            cell, shift = target.get(s, (s, 0))
            tx, ty = 1 + (cell % ncx) * CELL_W + shift, 1 + (cell // ncx) * CELL_H + BAND
            assert tx + CELL_W <= w and ty + CELL_H <= h
            dx, dy = tx - bx, ty - by
            fx, fy = F(dx + 0.3 if dx >= 0 else dx), F(dy + 0.4)      # (a negative flow with a fraction would warp to k + (int)fx but sample (int)(k + fx), one apart)
            self.last[by:by + CELL_H, bx:bx + CELL_W] = slot_label(s)
            self.flow[by:by + CELL_H, bx:bx + CELL_W] = (fx, fy)
            self.area[s] = (tx, ty)
            jj, kk = np.meshgrid(np.arange(by, by + CELL_H), np.arange(bx, bx + CELL_W), indexing="ij")
            px, py = kk.ravel().astype(np.float32) + fx, jj.ravel().astype(np.float32) + fy
            assert np.array_equal(px.astype(np.int32), kk.ravel() + dx) and np.array_equal(py.astype(np.int32), jj.ravel() + dy)
            px[:outside.get(s, 0)] = F(-3.0)
            sl += [slot_label(s)] * px.size; cx += list(px); cy += list(py); kx += list(kk.ravel()); ky += list(jj.ravel())
        for s in range(n_labels):
            tx, ty = self.area[s]
            self.cur[ty:ty + CELL_H, tx:tx + CELL_W] = 0 if s in dropped else slot_label(s)
        for s in sorted(paint):
            tx, ty = self.area[s]
            c = 0
            for lab, ncols in paint[s]:
                if lab is not None:
                    self.cur[ty:ty + CELL_H, tx + c:tx + c + ncols] = lab
                c += ncols
            assert c == CELL_W
        order = np.random.default_rng(seed).permutation(len(sl))
        self.sl = np.array(sl, np.int32)[order]; self.cx = np.array(cx, np.float32)[order]; self.cy = np.array(cy, np.float32)[order]
        self.kx = np.array(kx, np.float32)[order]; self.ky = np.array(ky, np.float32)[order]        # the samples' last-frame pixels

    def samples(self, slots=None):
        if slots is None:
            return self.sl, self.cx, self.cy
        keep = np.isin(self.sl, [slot_label(s) for s in slots])
        return self.sl[keep], self.cx[keep], self.cy[keep]

    def recovered(self, mask_after):
        """slots whose label covers more of ``mask_after`` than of the current mask"""
        return {s for s in range(self.n) if (mask_after == slot_label(s)).sum() > (self.cur == slot_label(s)).sum()}


def scene_plain(w, n_labels, r):
    """label slot r is missing from the current mask, every other label is where its samples land"""
    return MaskScene(w, n_labels, dropped={r}), {r}


def scene_cascade(w, n_labels, a, b, c):
    """a is missing: recovered.  b's samples see X on 70 pixels and background on 50 (alone: X wins, not recovered); a's warp covers 40 of the
    X pixels - background 50, a 40, X 30: recovered.  c's samples see background on 60, X on 50, Y on 10 (alone, or after a only:
    recovered); b's warp covers 30 of the background pixels - X 50, background 30, b 30: NOT recovered."""
    assert a < b < c
    sc = MaskScene(w, n_labels, dropped={a, b, c}, target={a: (70, 0), b: (70, 8), c: (70, 17)},
                   paint={b: [(LAB_X, 7), (0, 5)], c: [(None, 3), (0, 3), (LAB_X, 5), (LAB_Y, 1)]})
    return sc, {a, b}


def scene_top_slot_after_recovery(w, a=10, b=63):
    """64 labels: slot 63 is recovered only because slot a's warp lands under its samples (the first two steps of the cascade)."""
    sc = MaskScene(w, 64, dropped={a, b}, target={a: (70, 0), b: (70, 8)}, paint={b: [(LAB_X, 7), (0, 5)]})
    return sc, {a, b}


def scene_votes(w, n_labels, bad_label=None):
    """The vote's thresholds, all labels missing from the current mask unless said otherwise:
      slot 0: 21 samples outside the image, 99 inside: not recovered       slot 1: 20 outside, 100 inside: recovered
      slot 2: background 60, label 5 60: a tie, the smallest wins: recovered   slot 3: labels 5 and 7 50 each, background 20: not recovered
      slot 4: background 70, label 1023 50: recovered (the last bin)        slot 5: label 1023 70, background 50: not recovered
    the slots from 6 on are in place (not recovered).  ``bad_label``: painted under 10 samples of slot 5 (1024 = out of the bins)."""
    assert n_labels >= 6
    paint = {2: [(0, 6), (5, 6)], 3: [(5, 5), (7, 5), (0, 2)], 4: [(0, 7), (1023, 5)], 5: [(1023, 7), (0, 5)]}
    if bad_label is not None:
        paint[5] = [(1023, 7), (0, 4), (bad_label, 1)]
    sc = MaskScene(w, n_labels, dropped={0, 1, 2, 3, 4, 5}, paint=paint, outside={0: 21, 1: 20})
    return sc, {1, 2, 4}


# ---- RenewFrameInfo, static part --------------------------------------------------------------------------------------------
NEAR = F(1.0) - F(2.0 ** -20)                # a distance whose square rounds below 1


def renew_static_case(n1, n_orb, w=320, h=200):
    """n1 carried candidates and n_orb top-up keypoints on a 320 x 200 image.
    Carried candidate i sits on its own pixel; i % 3 == 0 is invalid (mask, depth 0, depth just above 40, fx == 0 in turn), i % 3 == 1 has
    depth exactly 40 (valid).  The candidates 0, 255, 256 and n1-1 - the first and last slots of 256-wide tiles of the carried list - are
    "hosts" at (2, y): each has a top-up keypoint at distance exactly 1 (not used: it is accepted when the walk reaches it) and one at
    1 - 2^-20 (used: never accepted, although its pixel is the host's, which is valid).  Candidate 100 is INVALID at (5, 190) and has a valid
    top-up keypoint 0.5 px away: the pair must not count as used.  Top-up keypoint i % 4 == 0 is invalid (mask)."""
    assert n1 > 300 and n_orb > 200
    mask = np.zeros((h, w), np.int32); depth = np.full((h, w), 10.0, np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 0.5, -0.5
    q = np.arange(n1)
    x, y = 20 + q % 280, 5 + q // 280
    sx, sy = (x + 0.25).astype(np.float32), (y + 0.5).astype(np.float32)
    valid = q % 3 != 0
    depth[y[q % 3 == 1], x[q % 3 == 1]] = 40.0
    why = (q // 3) % 4
    s = ~valid & (why == 0); mask[y[s], x[s]] = 2
    s = ~valid & (why == 1); depth[y[s], x[s]] = 0.0
    s = ~valid & (why == 2); depth[y[s], x[s]] = above(40.0)
    s = ~valid & (why == 3); flow[y[s], x[s], 0] = 0.0
    hosts = sorted({0, 255, 256, n1 - 1})
    for t, i in enumerate(hosts):
        sx[i], sy[i] = 2.0, 110.0 + 4 * t
        valid[i] = True
    sx[100], sy[100] = 5.0, 190.0
    mask[190, 5] = 7; valid[100] = False
    o = np.arange(n_orb)
    ox, oy = (20 + o % 280 + 0.5).astype(np.float32), (135 + o // 280 + 0.25).astype(np.float32)
    ovalid = o % 4 != 0
    mask[135 + o[~ovalid] // 280, 20 + o[~ovalid] % 280] = 3
    at_one, near = [], []                                     # top-up indices at distance exactly 1 / 1 - 2^-20 from a host
    spots = [0, n_orb - 1] + [19 * k + 7 for k in range(1, 10)]
    for t, i in enumerate(hosts):
        a, b = spots[2 * t], spots[2 * t + 1]
        ox[a], oy[a] = F(2.0) + NEAR, sy[i]; near.append(a)
        ox[b], oy[b] = 3.0, sy[i]; at_one.append(b)
        for k in (a, b):
            mask[135 + k // 280, 20 + k % 280] = 0           # (its generic pixel is not read any more)
            ovalid[k] = True
        ovalid[a] = False                                     # never accepted: used
        assert (sx[i] - ox[a]) ** 2 < 1 and (sx[i] - ox[b]) ** 2 == 1 and int(ox[a]) == 2
    e = spots[2 * len(hosts)]
    ox[e], oy[e] = 4.5, 190.0; ovalid[e] = True               # beside the invalid carried candidate 100
    tm = np.concatenate([[-1], 3 + np.arange(n1 // 2), [-1, -1], 3 + np.arange(n1 // 2, n1)]).astype(np.int32)
    stat_x = np.concatenate([np.zeros(3, np.float32), sx]); stat_y = np.concatenate([np.zeros(3, np.float32), sy])
    return dict(mask=mask, depth=depth, flow=flow, tm=tm, stat_x=stat_x, stat_y=stat_y, orb_x=ox, orb_y=oy, n_valid=int(valid.sum()), n_top=int(ovalid.sum()),
                at_one=at_one, near=near, beside_invalid=e, hosts=hosts)


def renew_static_expected(case, max_num):
    """(carried, topped up) counts of the reference's walk: the carry-over stops once the size EXCEEDS the limit; the top-up runs while
    the size is below it."""
    carried = min(case["n_valid"], max_num + 1)
    top = min(max(max_num - carried, 0), case["n_top"])
    return carried, top


# ---- RenewFrameInfo, objects ------------------------------------------------------------------------------------------------
def renew_object_case(nc0, n_tmp=None, w=320, h=200):
    """Object 0 (label 1, tracked) with nc0 carried points, object 1 (label 5, lost: skipped), object 2 (label 2, tracked) with 40; label 3
    is in the image but not tracked (its samples come out with object label -2).  The first carried points of object 0 truncate onto the
    0 / w-1 / w / h-1 / h bounds; then every 5th has depth exactly 25 or 0 (dropped), the ones after those the float below 25 (kept)."""
    mask = np.ones((h, w), np.int32); depth = np.full((h, w), 10.0, np.float32); flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 0.25, 0.5
    mask[:, 160:300] = 2; mask[120:, 300:316] = 3; mask[0:3, 200:260] = 0
    q = np.arange(nc0)
    x, y = 22 + q % 120, 5 + q // 120
    cx, cy = (x + 0.3).astype(np.float32), (y + 0.6).astype(np.float32)
    valid = np.ones(nc0, bool)
    s = q % 10 == 0; depth[y[s], x[s]] = 25.0; valid[s] = False
    s = q % 10 == 5; depth[y[s], x[s]] = 0.0; valid[s] = False
    s = q % 5 == 1; depth[y[s], x[s]] = below(25.0)
    special = [(0.7, 50.5, 0), (-0.5, 50.0, 0), (w - 1 + 0.3, 50.5, 1), (w + 0.2, 50.5, 0), (50.5, 0.7, 0), (50.5, h - 1 + 0.2, 1), (50.5, h + 0.1, 0),
               (60.9, 12.9, 1), (64.2, 13.7, 1)]              # the last two: keys (60, 12) - ON a sample - and (64, 13) - exactly 1 px from one
    for k, (a, b, v) in enumerate(special):
        cx[k], cy[k], valid[k] = a, b, bool(v)
    depth[5, 22:22 + len(special)] = 10.0
    q2 = np.arange(40)
    cx2, cy2 = (170 + 3 * q2 + 0.5).astype(np.float32), np.full(40, 30.25, np.float32)
    extra = np.array([[1.5, 1.5], [100.5, 100.5]], np.float32)                  # points no object refers to
    cur_x = np.concatenate([extra[:, 0], cx, cx2]); cur_y = np.concatenate([extra[:, 1], cy, cy2])
    inl = [2 + np.arange(nc0, dtype=np.int32), np.array([0, 1], np.int32), 2 + nc0 + np.arange(40, dtype=np.int32)]
    ob = object_sample(mask, depth, flow, TH_OBJ, 4)
    if n_tmp is not None:                                     # a spread over the whole list, the samples at (60, 12), (64, 12) and (24, 8) among them
        must = [int(np.nonzero((ob["key_x"] == a) & (ob["key_y"] == b))[0][0]) for a, b in ((60, 12), (64, 12), (24, 8))]
        pick = np.unique(np.concatenate([np.linspace(0, ob["label"].size - 1, n_tmp - 3).astype(int), must]))
        extra_i = [i for i in range(ob["label"].size) if i not in set(pick)][: n_tmp - pick.size]
        pick = np.sort(np.concatenate([pick, extra_i]).astype(int))
        assert pick.size == n_tmp
        ob = {k: v[pick] for k, v in ob.items()}
    tmp = dict(x=ob["key_x"], y=ob["key_y"], depth=ob["depth"], label=ob["label"], flow_x=ob["flow_x"], flow_y=ob["flow_y"], corr_x=ob["corr_x"], corr_y=ob["corr_y"])
    rng = np.random.default_rng(nc0)
    return dict(mask=mask, depth=depth, flow=flow, inl=inl, stat=np.array([1, 0, 1], np.uint8), sem_pos=np.array([1, 5, 2], np.int32), mod=np.array([11, 12, 13], np.int32),
                cur_x=cur_x, cur_y=cur_y, col=rng.integers(1, 9, cur_x.size).astype(np.int32), tmp=tmp, n_valid0=int(valid.sum()), n_valid2=40)
