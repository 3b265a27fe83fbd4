"""NumPy restatement of the stereo rectifier's contract (include/vdo_slam_hip.h, vdo_rectify_plan / vdo_rectify_compute / vdo_rectify_gate):
the map in fp64 (or any NumPy float type, for the long-double comparison), one rounded operation per line in the order of the contract, and
the integer remap.  Nothing here is shared with the library."""
import numpy as np

INVALID = np.iinfo(np.int32).min


def valid_bilinear(qmap, ws, hs):
    """bool [H, W]: the bilinear validity of a stored map against a source of ws x hs"""
    q = np.asarray(qmap).astype(np.int64)
    ix, ax, iy, ay = q[..., 0] >> 5, q[..., 0] & 31, q[..., 1] >> 5, q[..., 1] & 31
    return (ix >= 0) & (iy >= 0) & (ix + (ax > 0) <= ws - 1) & (iy + (ay > 0) <= hs - 1)


def valid_nearest(qmap, ws, hs):
    q = np.asarray(qmap).astype(np.int64)
    x, y = (q[..., 0] + 16) >> 5, (q[..., 1] + 16) >> 5
    return (x >= 0) & (y >= 0) & (x < ws) & (y < hs)


def plan(K4, D, R, P4, src_size, dst_size, dtype=np.float64, full=False):
    """(map int32 [H, W, 2], valid uint8 [H, W], n_valid); with full=True also (us, vs) before the rounding."""
    f = dtype
    fx, fy, cx, cy = [f(v) for v in K4]
    D = list(D) + [0.0] * (5 - len(D))
    k1, k2, p1, p2, k3 = [f(v) for v in D]
    R = np.asarray(R, np.float64).reshape(3, 3).astype(f)
    fxp, fyp, cxp, cyp = [f(v) for v in P4]
    (ws, hs), (W, H) = src_size, dst_size
    one, two, c32 = f(1), f(2), f(32)
    u = np.arange(W, dtype=f)[None, :].repeat(H, 0)
    v = np.arange(H, dtype=f)[:, None].repeat(W, 1)
    with np.errstate(all="ignore"):
        x = (u - cxp) / fxp
        y = (v - cyp) / fyp
        X = (R[0, 0] * x + R[1, 0] * y) + R[2, 0]
        Y = (R[0, 1] * x + R[1, 1] * y) + R[2, 1]
        Wc = (R[0, 2] * x + R[1, 2] * y) + R[2, 2]
        front = Wc > 0
        xn = X / Wc
        yn = Y / Wc
        x2 = xn * xn
        y2 = yn * yn
        r2 = x2 + y2
        xy2 = two * (xn * yn)
        t = r2 * k3
        t = k2 + t
        t = r2 * t
        t = k1 + t
        t = r2 * t
        kr = one + t
        xd = (xn * kr + p1 * xy2) + p2 * (r2 + two * x2)
        yd = (yn * kr + p1 * (r2 + two * y2)) + p2 * xy2
        us = fx * xd + cx
        vs = fy * yd + cy
        rx = np.rint(c32 * us)
        ry = np.rint(c32 * vs)
        lim = f(2.0 ** 30)
        ok = front & np.isfinite(rx) & np.isfinite(ry) & (np.abs(rx) < lim) & (np.abs(ry) < lim)
    q = np.stack([np.where(ok, rx, 0).astype(np.int64), np.where(ok, ry, 0).astype(np.int64)], -1)
    ok = ok & valid_bilinear(q, ws, hs)
    qmap = np.where(ok[..., None], q, INVALID).astype(np.int32)
    valid = ok.astype(np.uint8)
    if full:
        return qmap, valid, int(ok.sum()), us, vs
    return qmap, valid, int(ok.sum())


def gray(img, rgb_order=0):
    """vdo_rgb2gray (K2) on uint8 [H, W, 3 | 4]; a [H, W] image passes through"""
    img = np.asarray(img)
    if img.ndim == 2:
        return img
    p = img.astype(np.int64)
    r, g, b = (p[..., 0], p[..., 1], p[..., 2]) if rgb_order else (p[..., 2], p[..., 1], p[..., 0])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def remap(src, qmap, border=0, nearest=False, rgb_order=0):
    """uint8 [H, W] from src uint8 [Hs, Ws] or [Hs, Ws, 3 | 4] (made grey first) through a stored map int32 [H, W, 2]"""
    S = gray(src, rgb_order).astype(np.int64)
    hs, ws = S.shape
    q = np.asarray(qmap).astype(np.int64)
    if nearest:
        ok = valid_nearest(q, ws, hs)
        x, y = np.where(ok, (q[..., 0] + 16) >> 5, 0), np.where(ok, (q[..., 1] + 16) >> 5, 0)
        return np.where(ok, S[y, x], border).astype(np.uint8)
    ok = valid_bilinear(q, ws, hs)
    ix, ax, iy, ay = q[..., 0] >> 5, q[..., 0] & 31, q[..., 1] >> 5, q[..., 1] & 31
    ix, iy = np.where(ok, ix, 0), np.where(ok, iy, 0)
    ix1, iy1 = np.minimum(ix + 1, ws - 1), np.minimum(iy + 1, hs - 1)       # (a clamped tap carries weight 0 wherever the pixel is valid)
    out = ((32 - ax) * (32 - ay) * S[iy, ix] + ax * (32 - ay) * S[iy, ix1] + (32 - ax) * ay * S[iy1, ix] + ax * ay * S[iy1, ix1] + 512) >> 10
    return np.where(ok, out, border).astype(np.uint8)


def gate(image, valid):
    """(the gated float32 image, the number of values whose bits changed)"""
    img = np.array(image, np.float32, copy=True)
    bits = img.view(np.uint32)
    hit = (np.asarray(valid) == 0)
    n = int((hit & (bits != 0)).sum())
    bits[hit] = 0
    return img, n


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------
# EuRoC MAV cam0 as ORB-SLAM2 ships it (Examples/Stereo/EuRoC.yaml: LEFT.K, LEFT.D, LEFT.R, LEFT.P; 752 x 480)
EUROC_K = (458.654, 457.296, 367.215, 248.375)
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)
EUROC_R = (0.999966347530033, -0.001422739138722922, 0.008079580483432283,
           0.001365741834644127, 0.9999741760894847, 0.007055629199258132,
           -0.008089410156878961, -0.007044357138835809, 0.9999424675829176)
EUROC_P = (435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297)
EUROC_SIZE = (752, 480)
# KITTI tracking camera of the reference's example/kitti-0000-0013.yaml (1242 x 375)
KITTI_K = (721.5377, 721.5377, 609.5593, 172.8540)
KITTI_SIZE = (1242, 375)
IDENTITY_R = (1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)


def euroc_small():
    """EuRoC cam0 with K and P divided by 8, 94 x 60: reaches all 32 fractions on both axes (the small fixture of the GPU tests)"""
    return dict(K4=tuple(v / 8 for v in EUROC_K), D=EUROC_D, R=EUROC_R, P4=tuple(v / 8 for v in EUROC_P), src_size=(94, 60), dst_size=(94, 60))


def rotation(axis, angle):
    """Rodrigues, fp64, row-major 9-tuple"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
    return tuple(float(v) for v in R.reshape(-1))
