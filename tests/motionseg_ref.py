"""NumPy restatement of the motion segmenter's contract (include/vdo_slam_hip.h, vdo_motionseg_*): stage 1 in float32 with one rounded
operation per step in the header's order, stage 2 in integers, and the sample lists of the ego-motion.  The device must equal it bit for bit."""
import numpy as np

F = np.float32
FLT_MIN = np.finfo(np.float32).tiny

DEFAULTS = dict(sigma_flow=0.5, sigma_disp=0.5, chi2=9.0, min_disparity=0.0, vote_radius=2, vote_num=1, vote_den=2, min_known=6, class_value=1)


def _finite(a):
    return np.abs(a) <= np.finfo(np.float32).max                # false for NaN and the infinities


def _source(disp0, flow, flow_valid, K4, unit, min_disparity):
    """Stage 1's tests on the source pixels: (ok, d0, uo, vo, xi, yi) with xi, yi the int target where ok (0 elsewhere)"""
    H, W = disp0.shape
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    d0 = disp0.astype(F) / F(unit)
    uo = xf + flow[..., 0].astype(F)
    vo = yf + flow[..., 1].astype(F)
    xq = np.floor(uo + F(0.5)); yq = np.floor(vo + F(0.5))
    min_d = max(F(min_disparity), FLT_MIN)
    ok = _finite(d0) & (d0 >= min_d) & _finite(uo) & _finite(vo) & (xq >= F(0)) & (xq <= F(W - 1)) & (yq >= F(0)) & (yq <= F(H - 1))
    if flow_valid is not None:
        ok &= np.asarray(flow_valid) != 0
    xi = np.where(ok, xq, 0).astype(np.int64); yi = np.where(ok, yq, 0).astype(np.int64)
    return ok, d0, uo, vo, xi, yi, xf, yf


def _backproject(d0, xf, yf, K4, bf):
    fx, fy, cx, cy = (F(v) for v in K4)
    Z = F(bf) / d0
    X = (xf - cx) * Z / fx
    Y = (yf - cy) * Z / fy
    return X, Y, Z


def residual(disp0, disp1, flow, flow_valid, T, K4, bf, unit, sigma_flow=0.5, sigma_disp=0.5, chi2=9.0, min_disparity=0.0, **_):
    """-> (state uint8 [H, W]: 0 static, 1 moving, 2 unknown; residual float32 [H, W]: e, or -1 where unknown)"""
    disp0 = np.asarray(disp0, F); disp1 = np.asarray(disp1, F); flow = np.asarray(flow, F)
    T = np.asarray(T, F).reshape(4, 4)
    fx, fy, cx, cy = (F(v) for v in K4)
    with np.errstate(all="ignore"):
        ok, d0, uo, vo, xi, yi, xf, yf = _source(disp0, flow, flow_valid, K4, unit, min_disparity)
        d1 = disp1[yi, xi] / F(unit)
        ok = ok & _finite(d1) & (d1 > F(0))
        X, Y, Z = _backproject(d0, xf, yf, K4, bf)
        Xp = (T[0, 0] * X + T[0, 1] * Y) + (T[0, 2] * Z + T[0, 3])
        Yp = (T[1, 0] * X + T[1, 1] * Y) + (T[1, 2] * Z + T[1, 3])
        Zp = (T[2, 0] * X + T[2, 1] * Y) + (T[2, 2] * Z + T[2, 3])
        up = fx * Xp / Zp + cx
        vp = fy * Yp / Zp + cy
        dp = F(bf) / Zp
        du = uo - up; dv = vo - vp; dd = d1 - dp
        wf = F(1) / (F(sigma_flow) * F(sigma_flow)); wd = F(1) / (F(sigma_disp) * F(sigma_disp))
        e = (du * du + dv * dv) * wf + (dd * dd) * wd
        ok = ok & (Zp > F(0)) & _finite(e)
        assert e.dtype == F
        state = np.where(ok, np.where(e > F(chi2), 1, 0), 2).astype(np.uint8)
        res = np.where(ok, e, F(-1)).astype(F)
    return state, res


def _box(a, r):
    """Sums over the (2r+1)^2 window clipped at the image, int64"""
    H, W = a.shape
    c = np.zeros((H + 1, W + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), 0), 1)
    y0 = np.clip(np.arange(H) - r, 0, H); y1 = np.clip(np.arange(H) + r + 1, 0, H)
    x0 = np.clip(np.arange(W) - r, 0, W); x1 = np.clip(np.arange(W) + r + 1, 0, W)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def vote(state, vote_radius=2, vote_num=1, vote_den=2, min_known=6, class_value=1, **_):
    """-> (cls uint8 [H, W], (moving pixels after the vote, state-0 pixels, state-2 pixels))"""
    m = _box(state == 1, vote_radius); s = _box(state == 0, vote_radius)
    moving = (m + s >= min_known) & (m * vote_den > vote_num * (m + s))
    cls = np.where(moving, class_value, 0).astype(np.uint8)
    return cls, (int(moving.sum()), int((state == 0).sum()), int((state == 2).sum()))


def stages(disp0, disp1, flow, flow_valid, T, K4, bf, unit, **prm):
    p = dict(DEFAULTS); p.update(prm)
    state, res = residual(disp0, disp1, flow, flow_valid, T, K4, bf, unit, **p)
    cls, counts = vote(state, **p)
    return dict(state=state, residual=res, cls=cls, counts=counts)


def samples(disp0, flow, flow_valid, K4, bf, unit, step, min_disparity=0.0, **_):
    """The ego-motion's sample lists: (X float64 [n, 3], uv float64 [n, 2]) of the kept grid positions in raster order"""
    disp0 = np.asarray(disp0, F); flow = np.asarray(flow, F)
    H, W = disp0.shape
    with np.errstate(all="ignore"):
        ok, d0, uo, vo, _, _, xf, yf = _source(disp0, flow, flow_valid, K4, unit, min_disparity)
        X, Y, Z = _backproject(d0, xf, yf, K4, bf)
    gy = np.arange(step // 2, H, step); gx = np.arange(step // 2, W, step)
    if gy.size == 0 or gx.size == 0:
        return np.zeros((0, 3)), np.zeros((0, 2))
    sel = np.ix_(gy, gx)
    k = ok[sel].ravel()
    X3 = np.stack([X[sel].ravel(), Y[sel].ravel(), Z[sel].ravel()], -1).astype(np.float64)[k]
    uv = np.stack([uo[sel].ravel(), vo[sel].ravel()], -1).astype(np.float64)[k]
    return np.ascontiguousarray(X3), np.ascontiguousarray(uv)
