"""NumPy restatement of the photometric aligner's contract (include/vdo_slam_hip.h, "Photometric aligner", vdo_photo_*): the grey formula in
integers, the model's packing, the per-sample rows in float32 with one rounded operation per step in the header's order, the terms as exact float64
products, every sum as the aligner's adjacent-pair tree over the aligner's slot vector (tests/align_ref.py), the combine and the joint solve in
float64.  The device must equal the grey image, the packed model, the sums, the counts and the rows bit for bit."""
import math

import numpy as np

from tests import align_ref as A
from tests.dense_ref import F, FLT_MIN, _finite

USED, NO_DEPTH, MASKED, NO_MODEL, FAR = range(5)
TRACE_ROW = 16 + 28 + 5 + 28 + 5


def grey(image, rgb_order=0):
    """uint8 [H, W] or [H, W, 1 | 3 | 4] -> float32 [H, W]: Y = (77 R + 150 G + 29 B + 128) >> 8, the value itself with one channel"""
    a = np.asarray(image, np.uint8)
    if a.ndim == 2 or a.shape[2] == 1:
        return a.reshape(a.shape[0], a.shape[1]).astype(F)
    r, g, b = (a[..., 2 if rgb_order else 0].astype(np.int64), a[..., 1].astype(np.int64), a[..., 0 if rgb_order else 2].astype(np.int64))
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(F)


def valid(i):
    return _finite(i) & (i >= F(0))


def pack_model(depth, intensity):
    """-> float32 [Hm, Wm, 2], both images as they are"""
    return np.stack([np.asarray(depth, F), np.asarray(intensity, F)], -1)


def keep_as_model(D, mask, I, min_depth, max_depth):
    """The current frame as the model: the depth where it passes the frame's depth test and the mask is 0, else 0.0f; the intensity I"""
    D = np.asarray(D, F)
    min_d = max(F(min_depth), F(0)); max_d = F(max_depth)
    with np.errstate(all="ignore"):
        ok = _finite(D) & (D > min_d) & (D <= max_d)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    return pack_model(np.where(ok, D, F(0)).astype(F), I)


def rows(D, mask, I, K4, T, model, Km, Tm, min_depth, max_depth, max_dist, max_diff, subsample=1):
    """model: float32 [Hm, Wm, 2].  -> (rows float32 [Hs, Ws, 8]: J (6), e, w = 1, zeros where skipped; cls int [Hs, Ws]: USED .. FAR)"""
    D = np.asarray(D, F); H, W = D.shape
    I = np.asarray(I, F)
    model = np.asarray(model, F); Hm, Wm = model.shape[:2]
    s = int(subsample)
    Ws, Hs = A.grid(W, H, s)
    fx, fy, cx, cy = (F(v) for v in K4)
    fxm, fym, cxm, cym = (F(v) for v in Km)
    T = np.asarray(T, F).reshape(4, 4); Tm = np.asarray(Tm, F).reshape(4, 4)
    min_d = max(F(min_depth), F(0)); max_d = F(max_depth); md = F(max_dist); mdiff = F(max_diff)
    xi = (np.arange(Ws) * s)[None, :].repeat(Hs, 0); yi = (np.arange(Hs) * s)[:, None].repeat(Ws, 1)
    cls = np.full((Hs, Ws), -1, np.int64)
    with np.errstate(all="ignore"):
        d = D[yi, xi]; iF = I[yi, xi]
        ok = _finite(d) & (d > min_d) & (d <= max_d) & valid(iF)
        cls[~ok] = NO_DEPTH
        if mask is not None:
            m = ok & (np.asarray(mask)[yi, xi] != 0)
            cls[m] = MASKED
            ok &= ~m
        x = xi.astype(F); y = yi.astype(F)
        dx = (x - cx) / fx; dy = (y - cy) / fy
        Pc = [dx * d, dy * d, d]
        q = [Pc[a] - T[a, 3] for a in range(3)]
        Pw = [(T[0, a] * q[0] + T[1, a] * q[1]) + T[2, a] * q[2] for a in range(3)]
        Xm, Ym, Zm = [(Tm[r, 0] * Pw[0] + Tm[r, 1] * Pw[1]) + (Tm[r, 2] * Pw[2] + Tm[r, 3]) for r in range(3)]
        assert Zm.dtype == F
        okz = _finite(Zm) & (Zm > FLT_MIN)
        u = (fxm * Xm) / Zm + cxm; v = (fym * Ym) / Zm + cym
        x0 = np.floor(u); y0 = np.floor(v)
        inside = okz & _finite(u) & _finite(v) & (x0 >= F(0)) & (x0 <= F(Wm - 2)) & (y0 >= F(0)) & (y0 <= F(Hm - 2))
        x0i = np.where(inside, x0, 0).astype(np.int64); y0i = np.where(inside, y0, 0).astype(np.int64)
        x1i = np.minimum(x0i + 1, Wm - 1); y1i = np.minimum(y0i + 1, Hm - 1)                # (only where not inside does the clamp act)
        fa = u - x0; fb = v - y0
        corners = [model[y0i, x0i], model[y0i, x1i], model[y1i, x0i], model[y1i, x1i]]     # 00 10 01 11
        usable = inside
        for c in corners:
            usable = usable & _finite(c[..., 0]) & (c[..., 0] > F(0)) & valid(c[..., 1])
        cls[ok & ~usable] = NO_MODEL
        ok &= usable
        near = np.ones_like(ok)
        for c in corners:
            near &= np.abs(c[..., 0] - Zm) <= md                                              # a NaN fails
        i00, i10, i01, i11 = (c[..., 1] for c in corners)
        dt = i10 - i00; db = i11 - i01
        top = i00 + fa * dt; bot = i01 + fa * db
        im = top + fb * (bot - top)
        gx = dt + fb * (db - dt); gy = bot - top
        e = im - iF
        near &= np.abs(e) <= mdiff
        cls[ok & ~near] = FAR
        ok &= near
        cls[ok] = USED
        iz = F(1.0) / Zm
        ax = (fxm * gx) * iz; ay = (fym * gy) * iz; az = -(((ax * Xm) + (ay * Ym)) * iz)
        gw = [(Tm[0, a] * ax + Tm[1, a] * ay) + Tm[2, a] * az for a in range(3)]
        gc = [(T[a, 0] * gw[0] + T[a, 1] * gw[1]) + T[a, 2] * gw[2] for a in range(3)]
        J = [gc[0], gc[1], gc[2], Pc[1] * gc[2] - Pc[2] * gc[1], Pc[2] * gc[0] - Pc[0] * gc[2], Pc[0] * gc[1] - Pc[1] * gc[0]]
        out = np.stack(J + [e, np.ones_like(e)], -1)
        assert out.dtype == F
        out = np.where(ok[..., None], out, F(0)).astype(F)
    assert (cls >= 0).all()
    return out, cls


def linearise(D, mask, I, K4, T, model, Km, Tm, min_depth, max_depth, max_dist, max_diff, subsample=1):
    """-> (sums float64 [28], counts int64 [5]: used, no depth, masked, no model, far; rows float32 [Hs, Ws, 8])"""
    rw, cls = rows(D, mask, I, K4, T, model, Km, Tm, min_depth, max_depth, max_dist, max_diff, subsample)
    with np.errstate(all="ignore"):
        sums = A.pair_tree(A.slot_vector(A.terms(rw)))          # w is 1 or 0: the aligner's h = w * J is J, its w * e is e
    counts = np.array([(cls == k).sum() for k in range(5)], np.int64)
    assert counts.sum() == cls.size
    return sums, counts, rw


def combine(geo, photo, weight):
    """geo (28, or None for +0.0) + weight^2 * photo, two rounded operations per value"""
    lam = np.float64(weight) * np.float64(weight)
    g = np.zeros(28) if geo is None else np.asarray(geo, np.float64)
    with np.errstate(all="ignore"):
        scaled = lam * np.asarray(photo, np.float64)
        return g + scaled


def step(sums, used, min_pixels, T):
    """align_ref.step with T' = Exp(-xi) * T written out scalar by scalar in the order of vdo_align_step (align_ref multiplies matrices, whose
    summation order is the BLAS's: equal to an ulp of T', not to the bit) -> (status, T' float32 [4, 4], xi float64 [6], rms)"""
    status, Tn, xi, rms = A.step(sums, used, min_pixels, T)
    if status != 0:
        return status, Tn, xi, rms
    T = np.asarray(T, F).reshape(4, 4)
    Td = [[float(T[r, c]) for c in range(4)] for r in range(3)]
    v = [-float(xi[0]), -float(xi[1]), -float(xi[2])]; w = [-float(xi[3]), -float(xi[4]), -float(xi[5])]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]; th = math.sqrt(th2)
    if th < 1e-4:
        ca, cb, cc = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        ca, cb, cc = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    Wx = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    W2 = [[(Wx[r][0] * Wx[0][c] + Wx[r][1] * Wx[1][c]) + Wx[r][2] * Wx[2][c] for c in range(3)] for r in range(3)]
    out = np.zeros((4, 4), F)
    for r in range(3):
        R = [((1.0 if r == c else 0.0) + ca * Wx[r][c]) + cb * W2[r][c] for c in range(3)]
        t = 0.0
        for c in range(3):
            t += (((1.0 if r == c else 0.0) + cb * Wx[r][c]) + cc * W2[r][c]) * v[c]
        for c in range(4):
            s = (R[0] * Td[0][c] + R[1] * Td[1][c]) + R[2] * Td[2][c]
            if c == 3:
                s += t
            if not (abs(s) <= float(np.finfo(F).max)):
                return 2, T.copy(), np.zeros(6), rms
            out[r, c] = F(s)
    out[3] = [0, 0, 0, 1]
    return 0, out, xi, rms


def _rms(chi2, used):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(chi2) / used)) if used > 0 else 0.0


def solve(photo_lin, geo_lin, weight, T_init, min_pixels, geo_min_pixels, max_iterations, eps):
    """The joint solve.  photo_lin(T) -> (sums, counts, ..) the photometric linearisation at T; geo_lin likewise or None.
    -> (T float32 [4, 4], report dict, trace: per round (T, geo sums, geo counts, photo sums, photo counts))"""
    T = np.asarray(T_init, F).reshape(4, 4).copy()
    rep = dict(iterations=0, status=0, used_geo=0, used_photo=0, rms_geo_first=0.0, rms_geo_last=0.0, rms_photo_first=0.0, rms_photo_last=0.0, xi=np.zeros(6))
    trace = []
    for it in range(int(max_iterations)):
        sp, cp = photo_lin(T)[:2]
        sg, cg = geo_lin(T)[:2] if geo_lin is not None else (np.zeros(28), np.zeros(5, np.int64))
        trace.append((T.copy(), sg, cg, sp, cp))
        used_g, used_p = int(cg[0]), int(cp[0])
        rg, rp = _rms(sg[27], used_g), _rms(sp[27], used_p)
        rep.update(iterations=it + 1, used_geo=used_g, used_photo=used_p, rms_geo_last=rg, rms_photo_last=rp)
        if it == 0:
            rep.update(rms_geo_first=rg, rms_photo_first=rp)
        if used_p < min_pixels or (geo_lin is not None and used_g < geo_min_pixels):
            rep.update(status=1, xi=np.zeros(6))
            break
        status, Tn, xi, _ = step(combine(sg if geo_lin is not None else None, sp, weight), used_g + used_p, 6, T)
        rep.update(status=status, xi=xi)
        if status != 0:
            break
        T = Tn
        if (np.abs(xi) <= F(eps)).all():
            break
    return T, rep, trace


def trace_row(t):
    """One round of solve's trace as the library lays it out: [82] float64"""
    T, sg, cg, sp, cp = t
    return np.concatenate([np.asarray(T, np.float64).reshape(16), sg, np.asarray(cg, np.float64), sp, np.asarray(cp, np.float64)])


# ---- the textured wall the accuracy tests share: the plane z = Z0 in the world, seen fronto-parallel; its texture a sum of sinusoids -----------
WALL = dict(W=64, H=48, K4=(60.0, 60.0, 31.5, 23.5), Z0=5.0, base=120.0,
            # (amplitude in grey levels, wave vector in radians per metre (kx, ky), phase); footprint Z0 / fx = 1/12 m: the shortest period, 2 pi / |k| = 1.4 m, is 17 pixels
            waves=((40.0, (4.4, 0.0), 0.3), (30.0, (0.0, 4.2), 1.1), (25.0, (2.4, 2.9), 2.0), (15.0, (-1.9, 2.2), 0.7)),
            max_dist=0.5, max_iterations=20, eps=1e-7)


def wall_texture(X, Y):
    """The wall's grey value at world (X, Y), float64"""
    g = np.full(np.shape(X), WALL["base"], np.float64)
    for amp, (kx, ky), ph in WALL["waves"]:
        g = g + amp * np.sin(kx * np.asarray(X, np.float64) + ky * np.asarray(Y, np.float64) + ph)
    return g


def wall_render(T, W=None, H=None, K4=None):
    """What a camera at T (world -> camera) sees of the wall, analytically: (z-depth float32 [H, W], intensity float32 [H, W], unquantised)"""
    W = W or WALL["W"]; H = H or WALL["H"]; K4 = K4 or WALL["K4"]
    T = np.asarray(T, np.float64).reshape(4, 4)
    Rm, t = T[:3, :3], T[:3, 3]
    c = -Rm.T @ t
    ys, xs = np.mgrid[0:H, 0:W]
    rc = np.stack([(xs - K4[2]) / K4[0], (ys - K4[3]) / K4[1], np.ones((H, W))], -1)
    rw = rc @ Rm
    lam = (WALL["Z0"] - c[2]) / rw[..., 2]
    P = c + lam[..., None] * rw
    return lam.astype(F), wall_texture(P[..., 0], P[..., 1]).astype(F)
