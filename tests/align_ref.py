"""NumPy restatement of the aligner's contract (include/vdo_slam_hip.h, "Aligner", vdo_align_*): the per-sample rows in float32 with one rounded
operation per step in the header's order, the terms as exact float64 products, every sum as the adjacent-pair tree over the slot vector written
literally, the Gauss-Newton step and the solve loop in float64.  The model comes from dense_ref / raycast_ref.  The device must equal the sums,
the counts and the rows bit for bit."""
import math

import numpy as np

from tests.dense_ref import F, FLT_MIN, _finite

USED, NO_DEPTH, MASKED, NO_MODEL, FAR = range(5)
UPPER = [(r, c) for r in range(6) for c in range(r, 6)]                      # the order of the 21 A terms


def grid(W, H, s):
    Ws, Hs = -(-W // s), -(-H // s)
    return Ws, Hs


def rows(D, mask, K4, T, Dm, Gm, Km, Tm, min_depth, max_depth, max_dist, subsample=1):
    """-> (rows float32 [Hs, Ws, 8]: J (6), e, w, zeros where skipped; cls int [Hs, Ws]: USED .. FAR)"""
    D = np.asarray(D, F); H, W = D.shape
    Dm = np.asarray(Dm, F); Gm = np.asarray(Gm, F); Hm, Wm = Dm.shape
    s = int(subsample)
    Ws, Hs = grid(W, H, s)
    fx, fy, cx, cy = (F(v) for v in K4)
    fxm, fym, cxm, cym = (F(v) for v in Km)
    T = np.asarray(T, F).reshape(4, 4); Tm = np.asarray(Tm, F).reshape(4, 4)
    min_d = max(F(min_depth), F(0)); max_d = F(max_depth); md2 = F(max_dist) * F(max_dist)
    xi = (np.arange(Ws) * s)[None, :].repeat(Hs, 0); yi = (np.arange(Hs) * s)[:, None].repeat(Ws, 1)
    cls = np.full((Hs, Ws), -1, np.int64)
    with np.errstate(all="ignore"):
        d = D[yi, xi]
        ok = _finite(d) & (d > min_d) & (d <= max_d)
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
        xq = np.floor(u + F(0.5)); yq = np.floor(v + F(0.5))
        inside = okz & _finite(u) & _finite(v) & (xq >= F(0)) & (xq <= F(Wm - 1)) & (yq >= F(0)) & (yq <= F(Hm - 1))
        xqi = np.where(inside, xq, 0).astype(np.int64); yqi = np.where(inside, yq, 0).astype(np.int64)
        dm = Dm[yqi, xqi]; g = [Gm[yqi, xqi, a] for a in range(3)]
        gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        model = inside & _finite(dm) & (dm > F(0)) & _finite(gg) & (gg > F(0))
        cls[ok & ~model] = NO_MODEL
        ok &= model
        # the model point by the raycaster's formulas (raycast_ref.render): the centre of Tm, the ray of pixel (xq, yq) with Km
        c = [-((Tm[0, a] * Tm[0, 3] + Tm[1, a] * Tm[1, 3]) + Tm[2, a] * Tm[2, 3]) for a in range(3)]
        dxm = (xq - cxm) / fxm; dym = (yq - cym) / fym
        r = [(Tm[0, a] * dxm + Tm[1, a] * dym) + Tm[2, a] for a in range(3)]
        dl = [Pw[a] - (c[a] + dm * r[a]) for a in range(3)]
        dist2 = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]
        near = dist2 <= md2                                                   # a NaN fails
        cls[ok & ~near] = FAR
        ok &= near
        cls[ok] = USED
        e = (g[0] * dl[0] + g[1] * dl[1]) + g[2] * dl[2]
        w = F(1.0) / gg
        gc = [(T[a, 0] * g[0] + T[a, 1] * g[1]) + T[a, 2] * g[2] for a in range(3)]
        J = [gc[0], gc[1], gc[2], Pc[1] * gc[2] - Pc[2] * gc[1], Pc[2] * gc[0] - Pc[0] * gc[2], Pc[0] * gc[1] - Pc[1] * gc[0]]
        out = np.stack(J + [e, w], -1)
        assert out.dtype == F
        out = np.where(ok[..., None], out, F(0)).astype(F)
    assert (cls >= 0).all()
    return out, cls


def term(rw, k):
    """rows [..., 8] -> term k (0..27) float64 [...]; every product of two floats is exact in double"""
    J = rw[..., :6]; e = rw[..., 6]; w = rw[..., 7]
    if k == 27:
        return (w * e).astype(F).astype(np.float64) * e.astype(np.float64)
    r, c = UPPER[k] if k < 21 else (k - 21, None)
    h = (w * J[..., r]).astype(F).astype(np.float64)
    return h * (J[..., c] if c is not None else e).astype(np.float64)


def terms(rw):
    """rows [..., 8] -> the 28 terms float64 [..., 28]"""
    return np.stack([term(rw, k) for k in range(28)], -1)


def slot_vector(t):
    """terms [Hs, Ws, n] -> [P, n]: the samples at their slots, +0.0 elsewhere, padded to a power of two"""
    Hs, Ws, n = t.shape
    tx, ty = -(-Ws // 8), -(-Hs // 8)
    size = tx * ty * 64
    P = 1
    while P < size:
        P *= 2
    v = np.zeros((P, n), np.float64)
    j, i = np.mgrid[0:Hs, 0:Ws]
    slot = ((j // 8) * tx + i // 8) * 64 + (j % 8) * 8 + (i % 8)
    v[slot.ravel()] = t.reshape(-1, n)
    return v


def pair_tree(v):
    """the adjacent-pair tree over axis 0 (a power of two long)"""
    v = np.array(v, np.float64)
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def linearise(D, mask, K4, T, Dm, Gm, Km, Tm, min_depth, max_depth, max_dist, subsample=1):
    """-> (sums float64 [28], counts int64 [5]: used, no depth, masked, no model, far; rows float32 [Hs, Ws, 8])"""
    rw, cls = rows(D, mask, K4, T, Dm, Gm, Km, Tm, min_depth, max_depth, max_dist, subsample)
    with np.errstate(all="ignore"):
        sums = pair_tree(slot_vector(terms(rw)))
    counts = np.array([(cls == k).sum() for k in range(5)], np.int64)
    assert counts.sum() == cls.size
    return sums, counts, rw


def exp_se3(xi):
    """The SE(3) exponential of xi = (v, omega) -> 4 x 4 float64, the header's closed forms and series"""
    v = np.asarray(xi[:3], np.float64); w = np.asarray(xi[3:], np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]; th = math.sqrt(th2)
    if th < 1e-4:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    W2 = Wx @ Wx
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * Wx + b * W2
    E[:3, 3] = (np.eye(3) + b * Wx + c * W2) @ v
    return E


def step(sums, used, min_pixels, T):
    """-> (status, T' float32 [4, 4], xi float64 [6], rms)"""
    sums = np.asarray(sums, np.float64)
    T = np.asarray(T, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        rms = math.sqrt(sums[27] / used) if used > 0 and sums[27] >= 0 else (float("nan") if used > 0 else 0.0)
    zero = np.zeros(6)
    if used < min_pixels:
        return 1, T.copy(), zero, rms
    if not np.isfinite(sums).all():
        return 2, T.copy(), zero, rms
    A = np.zeros((6, 6)); b = sums[21:27]
    for t, (r, c) in enumerate(UPPER):
        A[r, c] = A[c, r] = sums[t]
    L = np.zeros((6, 6))
    for j in range(6):
        p = A[j, j]
        for k in range(j):
            p -= L[j, k] * L[j, k]
        if not p > 0.0:
            return 2, T.copy(), zero, rms
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 6):
            v = A[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y = np.zeros(6); xi = np.zeros(6)
    for i in range(6):
        v = -b[i]
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k, i] * xi[k]
        xi[i] = v / L[i, i]
    if not np.isfinite(xi).all():
        return 2, T.copy(), zero, rms
    Tn = exp_se3(-xi) @ T.astype(np.float64)
    if not (np.abs(Tn) <= np.finfo(F).max).all():
        return 2, T.copy(), zero, rms
    Tn = Tn.astype(F)
    Tn[3] = [0, 0, 0, 1]
    return 0, Tn, xi, rms


def solve(D, mask, K4, T_init, Dm, Gm, Km, Tm, min_depth, max_depth, max_dist, subsample, min_pixels, max_iterations, eps):
    """-> (T float32 [4, 4], report dict: iterations, status, used, rms_first, rms_last, xi; trace: per iteration (T, sums, counts))"""
    T = np.asarray(T_init, F).reshape(4, 4).copy()
    rep = dict(iterations=0, status=0, used=0, rms_first=0.0, rms_last=0.0, xi=np.zeros(6))
    trace = []
    for it in range(int(max_iterations)):
        sums, counts, _ = linearise(D, mask, K4, T, Dm, Gm, Km, Tm, min_depth, max_depth, max_dist, subsample)
        trace.append((T.copy(), sums, counts))
        status, Tn, xi, rms = step(sums, int(counts[0]), min_pixels, T)
        rep.update(iterations=it + 1, status=status, used=int(counts[0]), rms_last=rms, xi=xi)
        if it == 0:
            rep["rms_first"] = rms
        if status != 0:
            break
        T = Tn
        if (np.abs(xi) <= F(eps)).all():
            break
    return T, rep, trace


# ---- the room-corner scene the accuracy tests share (CPU: tests/test_align_ref.py, device: tests/test_align_gpu.py) ----------------------------
CORNER = dict(n=(48, 40, 48), origin=(-20, -18, -1), voxel=0.1, trunc=0.4, max_depth=8.0, W=64, H=48, K4=(50.0, 50.0, 31.5, 23.5), near=0.4, step=0.2, n_steps=36,
              min_weight=2, planes=(((1.0, 0.0, 0.0), 2.0), ((0.0, 1.0, 0.0), 1.5), ((0.0, 0.0, 1.0), 4.0)), max_dist=0.4, max_iterations=12, eps=1e-5)
# the perturbations: (translation in metres, rotation vector in degrees), 5 cm and 2 degrees each
PERTURBATIONS = [((0.05, 0.0, 0.0), (0.0, 2.0, 0.0)), ((0.0, -0.05, 0.0), (-2.0, 0.0, 0.0)), ((0.0, 0.0, 0.05), (0.0, 0.0, 2.0)),
                 ((0.03, 0.03, -0.0265), (1.2, -1.2, 1.058)), ((-0.04, 0.02, 0.0224), (-1.0, -1.5, -0.866))]


def look_at(eye, target):
    """world -> camera (float32 4 x 4) of a camera at eye looking at target, image y down"""
    eye = np.asarray(eye, np.float64); f = np.asarray(target, np.float64) - eye; f /= np.linalg.norm(f)
    r = np.cross([0.0, 1.0, 0.0], f); r /= np.linalg.norm(r)
    d = np.cross(f, r)
    T = np.eye(4)
    T[:3, :3] = np.stack([r, d, f])
    T[:3, 3] = -T[:3, :3] @ eye
    return T.astype(F)


def plane_depth(planes, T, W, H, K4):
    """The z-depth image a camera at T (world -> camera) measures of the nearest of the planes (n, d): n . p = d; float32, 0 where none is hit"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    Rm, t = T[:3, :3], T[:3, 3]
    c = -Rm.T @ t
    ys, xs = np.mgrid[0:H, 0:W]
    rc = np.stack([(xs - K4[2]) / K4[0], (ys - K4[3]) / K4[1], np.ones((H, W))], -1)
    rw = rc @ Rm                                                               # R^T applied to every ray
    best = np.full((H, W), np.inf)
    for nrm, d in planes:
        nrm = np.asarray(nrm, np.float64)
        with np.errstate(all="ignore"):
            lam = (d - nrm @ c) / (rw @ nrm)
        best = np.where((lam > 0) & (lam < best), lam, best)
    return np.where(np.isfinite(best), best, 0.0).astype(F)


def perturbed(T, trans, rot_deg):
    """Exp((trans, rot)) * T in double, narrowed"""
    xi = np.concatenate([np.asarray(trans, np.float64), np.deg2rad(np.asarray(rot_deg, np.float64))])
    return (exp_se3(xi) @ np.asarray(T, np.float64).reshape(4, 4)).astype(F)


def pose_error(T, T_true):
    """(translation error of the camera centre in metres, rotation error in degrees)"""
    A = np.asarray(T, np.float64).reshape(4, 4); B = np.asarray(T_true, np.float64).reshape(4, 4)
    ca = -A[:3, :3].T @ A[:3, 3]; cb = -B[:3, :3].T @ B[:3, 3]
    cosang = (np.trace(A[:3, :3] @ B[:3, :3].T) - 1.0) / 2.0
    return float(np.linalg.norm(ca - cb)), float(np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))))


CORNER_POSES = [((0.0, 0.0, 0.0), (1.2, 0.9, 4.0)), ((-0.3, -0.2, 0.2), (1.4, 0.8, 4.0)), ((0.3, 0.1, -0.1), (1.0, 1.1, 4.0)), ((0.1, -0.3, 0.4), (1.5, 1.0, 3.5))]
_corner = None


def corner_volume():
    """The inside corner of a room - the planes x = 2, y = 1.5, z = 4 - fused from four poses at 100 mm voxels; -> (dense_ref.Volume, the true frame pose)"""
    global _corner
    if _corner is None:
        from tests.dense_ref import Volume
        c = CORNER
        V = Volume(c["n"], c["voxel"], c["origin"])
        for eye, target in CORNER_POSES:
            T = look_at(eye, target)
            for _ in range(2):
                V.integrate(plane_depth(c["planes"], T, c["W"], c["H"], c["K4"]), None, T, c["K4"], c["trunc"], 0.0, c["max_depth"], 64)
        _corner = (V, look_at((0.05, -0.1, 0.1), (1.25, 0.95, 4.0)))
    return _corner


def corner_case(k):
    """Perturbation k: -> (depth of the frame at its true pose, T_true, T_init, model depth, model gradient rendered at T_init)"""
    from tests import raycast_ref
    c = CORNER
    V, T_true = corner_volume()
    T_init = perturbed(T_true, *PERTURBATIONS[k])
    D = plane_depth(c["planes"], T_true, c["W"], c["H"], c["K4"])
    Dm, Gm, _, _ = raycast_ref.render(V, c["W"], c["H"], c["K4"], c["near"], c["step"], c["n_steps"], c["min_weight"], T_init)
    return D, T_true, T_init, Dm, Gm
