"""CPU: the NumPy restatement of the photometric aligner's contract (tests/photo_ref.py) against cases worked by hand, its gates at their bounds,
its Jacobian against central differences of a float64 evaluation, the exact sum, the grey formula, and the accuracy of a joint solve in front of a
textured wall, where the aligner alone is singular; then the library's host functions (vdo_photo_combine and vdo_align_step need no device) against
the restatement's, bit for bit."""
import math

import numpy as np
import pytest

from tests import align_ref as A
from tests import photo_ref as P

F = np.float32
I4 = np.eye(4, dtype=F)
K1 = (1.0, 1.0, 0.0, 0.0)


def _sums_dict(sums):
    d = {f"A{r}{c}": sums[t] for t, (r, c) in enumerate(A.UPPER)}
    d.update({f"b{r}": sums[21 + r] for r in range(6)})
    d["chi2"] = sums[27]
    return d


def _model(depth, inten):
    return P.pack_model(np.asarray(depth, F), np.asarray(inten, F))


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------------
def test_one_pixel_by_hand():
    """K = Km = (1, 1, 0, 0), T = I, Tm a shift: Xm = Pw0 + 0.25, Ym = Pw1 + 0.5.  Pixel (0, 0) at depth 2 with grey 10: Pc = Pw = (0, 0, 2),
    (Xm, Ym, Zm) = (0.25, 0.5, 2), u = 0.125, v = 0.25, cell (0, 0), fa = 0.125, fb = 0.25.  Model intensities 8 16 / 12 28 (all depths 2):
    top = 8 + 0.125*8 = 9, bot = 12 + 0.125*16 = 14, im = 9 + 0.25*5 = 10.25, gx = 8 + 0.25*(16 - 8) = 10, gy = 5, e = 0.25.
    iz = 0.5: ax = 5, ay = 2.5, az = -((5*0.25 + 2.5*0.5)*0.5) = -1.25; Tm and T rotate nothing: gc = (5, 2.5, -1.25);
    J = (5, 2.5, -1.25, 0*(-1.25) - 2*2.5 = -5, 2*5 - 0 = 10, 0)."""
    Tm = I4.copy(); Tm[0, 3] = 0.25; Tm[1, 3] = 0.5
    model = _model([[2, 2], [2, 2]], [[8, 16], [12, 28]])
    sums, counts, rw = P.linearise(np.array([[2.0]], F), None, np.array([[10.0]], F), K1, I4, model, K1, Tm, 0.0, 10.0, 1.0, 255.0)
    assert counts.tolist() == [1, 0, 0, 0, 0]
    assert rw[0, 0].tolist() == [5.0, 2.5, -1.25, -5.0, 10.0, 0.0, 0.25, 1.0]
    J = [5.0, 2.5, -1.25, -5.0, 10.0, 0.0]
    want = {f"A{r}{c}": J[r] * J[c] for r, c in A.UPPER}
    want.update({f"b{r}": J[r] * 0.25 for r in range(6)}); want["chi2"] = 0.0625
    assert _sums_dict(sums) == want
    status, Tn, xi, rms = P.step(sums, 1, 1, I4)
    assert status == 2 and rms == 0.25 and np.array_equal(Tn, I4)             # one row: five motions unconstrained


def test_two_pixels_and_every_skip_through_its_count():
    """A second pixel (1, 0) at depth 2, grey 20: dx = 1, Pc = (2, 0, 2), (Xm, Ym, Zm) = (2.25, 0.5, 2), u = 1.125, v = 0.25, cell (1, 0) of a 3 x 2 model
    whose third column is 24 / 44: top = 16 + 0.125*8 = 17, bot = 28 + 0.125*16 = 30, im = 17 + 0.25*13 = 20.25, gx = 8 + 0.25*8 = 10, gy = 13, e = 0.25,
    ax = 5, ay = 6.5, az = -((5*2.25 + 6.5*0.5)*0.5) = -7.25, J = (5, 6.5, -7.25, -13, 10 + 14.5 = 24.5, 13)."""
    Tm = I4.copy(); Tm[0, 3] = 0.25; Tm[1, 3] = 0.5
    D = np.array([[2.0, 2.0]], F); I = np.array([[10.0, 20.0]], F)
    dm = np.full((2, 3), 2.0, F); im = np.array([[8, 16, 24], [12, 28, 44]], F)
    args = (K1, I4)
    tail = (K1, Tm, 0.0, 10.0, 1.0, 255.0)
    sums, counts, rw = P.linearise(D, None, I, *args, _model(dm, im), *tail)
    assert counts.tolist() == [2, 0, 0, 0, 0]
    assert rw[0, 1].tolist() == [5.0, 6.5, -7.25, -13.0, 24.5, 13.0, 0.25, 1.0]
    assert sums[0] == 50.0 and sums[27] == 0.125 and sums[21] == 2.5 and sums[5] == 5 * 13.0 and sums[20] == 169.0
    # the mask; a depth out of range, a NaN depth; an invalid grey value of the frame: no depth
    assert P.linearise(D, np.array([[0, 7]], np.int32), I, *args, _model(dm, im), *tail)[1].tolist() == [1, 0, 1, 0, 0]
    assert P.linearise(np.array([[np.nan, 11.0]], F), None, I, *args, _model(dm, im), *tail)[1].tolist() == [0, 2, 0, 0, 0]
    assert P.linearise(D, None, np.array([[-1.0, np.inf]], F), *args, _model(dm, im), *tail)[1].tolist() == [0, 2, 0, 0, 0]
    assert P.linearise(D, np.array([[3, 3]], np.int32), np.array([[np.nan, 20.0]], F), *args, _model(dm, im), *tail)[1].tolist() == [0, 1, 1, 0, 0]      # no depth comes first
    # a hole in either channel at each corner of pixel 1's cell: no model (pixel 0 shares the corners of column 1)
    for (r, c), n_bad in (((0, 1), 2), ((0, 2), 1), ((1, 1), 2), ((1, 2), 1), ((0, 0), 1)):
        for ch, bad in ((0, 0.0), (0, -1.0), (0, np.nan), (0, np.inf), (1, -1.0), (1, np.nan), (1, np.inf)):
            m = _model(dm, im); m[r, c, ch] = bad
            assert P.linearise(D, None, I, *args, m, *tail)[1].tolist() == [2 - n_bad, 0, 0, n_bad, 0], ((r, c), ch, bad)
    m = _model(dm, im); m[0, 1, 1] = 0.0                                     # intensity 0 is valid
    assert P.linearise(D, None, I, *args, m, *tail)[1].tolist() == [2, 0, 0, 0, 0]
    # outside the model: left of column 0, beyond the last cell (one pixel, both), behind the camera, below the last row, above the first
    for shift, want in (((-0.5, 0.5, 0.0), [1, 0, 0, 1, 0]), ((2.25, 0.5, 0.0), [1, 0, 0, 1, 0]), ((4.25, 0.5, 0.0), [0, 0, 0, 2, 0]), ((0.25, 0.5, -2.0), [0, 0, 0, 2, 0]), ((0.25, 2.5, 0.0), [0, 0, 0, 2, 0]),
                        ((0.25, -0.5, 0.0), [0, 0, 0, 2, 0])):
        T2 = I4.copy(); T2[:3, 3] = shift
        assert P.linearise(D, None, I, *args, _model(dm, im), K1, T2, 0.0, 10.0, 5.0, 255.0)[1].tolist() == want, shift
    # a model thinner than one cell has no cell
    for shape in ((1, 3), (2, 1), (1, 1)):
        assert P.linearise(D, None, I, *args, _model(np.full(shape, 2.0, F), np.full(shape, 9.0, F)), *tail)[1].tolist() == [0, 0, 0, 2, 0]
    nan_T = I4.copy(); nan_T[1, 2] = np.nan
    s_nan, c_nan, _ = P.linearise(D, None, I, K1, nan_T, _model(dm, im), *tail)
    assert c_nan.tolist() == [0, 0, 0, 2, 0] and not s_nan.any() and not np.signbit(s_nan).any()


def test_u_exactly_integer_and_the_last_cell():
    """u = 1 exactly is cell 1 with fa = 0: im = i(0, 1) when v is integer too.  x0 = Wm - 2 is the last cell; u = Wm - 1 exactly is outside."""
    D = np.array([[2.0, 2.0, 2.0]], F); I = np.array([[1.0, 2.0, 3.0]], F)
    dm = np.full((2, 3), 2.0, F); im = np.array([[8, 16, 24], [12, 28, 44]], F)
    sums, counts, rw = P.linearise(D, None, I, K1, I4, _model(dm, im), K1, I4, 0.0, 10.0, 1.0, 255.0)
    assert counts.tolist() == [2, 0, 0, 1, 0]                                # pixels 0 and 1: u = 0 and 1 (= Wm - 2); pixel 2: u = 2 = Wm - 1
    assert rw[0, 0, 6] == 8.0 - 1.0 and rw[0, 1, 6] == 16.0 - 2.0 and not rw[0, 2].any()
    assert rw[0, 1, 0] == 8.0 * 0.5 and rw[0, 1, 1] == 12.0 * 0.5           # gx = 24 - 16, gy = 28 - 16 at fa = fb = 0, iz = 1/2


# ---- the gates at their bounds ---------------------------------------------------------------------------------------------------------------------
def test_the_gates_exactly_at_the_bound_and_one_float_beyond():
    Tm = I4.copy(); Tm[0, 3] = 0.25; Tm[1, 3] = 0.5
    D = np.array([[2.0]], F); I = np.array([[10.0]], F)
    im = np.array([[8, 16], [12, 28]], F)                                    # e = 0.25 exactly (test_one_pixel_by_hand)
    for corner in range(4):
        dm = np.full((2, 2), 2.0, F); dm.ravel()[corner] = 2.5               # |2.5 - Zm| = 0.5 exactly
        run = lambda md, mdiff=255.0: P.linearise(D, None, I, K1, I4, _model(dm, im), K1, Tm, 0.0, 10.0, md, mdiff)[1].tolist()
        assert run(0.5) == [1, 0, 0, 0, 0], corner
        assert run(float(np.nextafter(F(0.5), F(0)))) == [0, 0, 0, 0, 1], corner
        dm.ravel()[corner] = 1.5                                             # the gate is two-sided
        assert run(0.5) == [1, 0, 0, 0, 0] and run(float(np.nextafter(F(0.5), F(0)))) == [0, 0, 0, 0, 1], corner
    dm = np.full((2, 2), 2.0, F)
    run = lambda mdiff: P.linearise(D, None, I, K1, I4, _model(dm, im), K1, Tm, 0.0, 10.0, 1.0, mdiff)[1].tolist()
    assert run(0.25) == [1, 0, 0, 0, 0] and run(float(np.nextafter(F(0.25), F(0)))) == [0, 0, 0, 0, 1]
    I[0, 0] = 10.5                                                           # e = -0.25: the gate is on |e|
    assert run(0.25) == [1, 0, 0, 0, 0] and run(float(np.nextafter(F(0.25), F(0)))) == [0, 0, 0, 0, 1]
    # 255 turns the gate off for every pair of valid uint8 values
    I[0, 0] = 255.0
    assert P.linearise(D, None, I, K1, I4, _model(dm, np.zeros((2, 2), F)), K1, Tm, 0.0, 10.0, 1.0, 255.0)[1].tolist() == [1, 0, 0, 0, 0]
    # the depth test's own bounds: d = max_depth is in, d = min_depth is out
    assert P.linearise(np.array([[2.0]], F), None, I, K1, I4, _model(dm, im), K1, Tm, 0.0, 2.0, 1.0, 255.0)[1].tolist() == [1, 0, 0, 0, 0]
    assert P.linearise(np.array([[2.0]], F), None, I, K1, I4, _model(dm, im), K1, Tm, 2.0, 9.0, 1.0, 255.0)[1].tolist() == [0, 1, 0, 0, 0]


# ---- a random smooth scene: the Jacobian, the tree ---------------------------------------------------------------------------------------------
def _smooth(rng, H, W, lo, hi, n_waves=4, max_freq=0.35):
    """A sum of low-frequency sinusoids scaled into [lo, hi]; max_freq in radians per pixel"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.zeros((H, W))
    for _ in range(n_waves):
        kx, ky = rng.uniform(-max_freq, max_freq, 2)
        g += rng.uniform(0.5, 1.0) * np.sin(kx * x + ky * y + rng.uniform(0, 6.28))
    g = (g - g.min()) / (g.max() - g.min())
    return (lo + (hi - lo) * g).astype(F)


def _smooth_scene(seed, W=37, H=29, Wm=41, Hm=23):
    rng = np.random.default_rng(seed)
    D = _smooth(rng, H, W, 2.0, 4.0)
    I = np.rint(_smooth(rng, H, W, 10.0, 240.0)).astype(F)
    Dm = _smooth(rng, Hm, Wm, 2.0, 4.0)
    Im = _smooth(rng, Hm, Wm, 10.0, 240.0)
    K4 = (30.0, 28.0, 18.2, 14.1); Km = (25.0, 26.0, 20.5, 11.0)
    T = A.perturbed(I4, (0.1, -0.05, 0.02), (1.0, 2.0, -1.5)); Tm = A.perturbed(I4, (-0.2, 0.1, 0.0), (-3.0, 1.0, 0.5))
    return D, I, K4, T, Dm, Im, Km, Tm


def _e64(D, I, K4, T, Im, Km, Tm):
    """The residual of every pixel in float64 from the same float32 inputs, no gates: (e, u, v); NaN where the cell is outside the model"""
    D = np.asarray(D, np.float64); H, W = D.shape
    T = np.asarray(T, np.float64); Tm = np.asarray(Tm, np.float64, ).reshape(4, 4)
    Hm, Wm = Im.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Pc = np.stack([(x - K4[0 + 2]) / K4[0] * D, (y - K4[3]) / K4[1] * D, D], -1)
    Pw = (Pc - T[:3, 3]) @ T[:3, :3]
    Pm = Pw @ Tm[:3, :3].T + Tm[:3, 3]
    u = Km[0] * Pm[..., 0] / Pm[..., 2] + Km[2]; v = Km[1] * Pm[..., 1] / Pm[..., 2] + Km[3]
    x0 = np.floor(u); y0 = np.floor(v)
    ok = (x0 >= 0) & (x0 <= Wm - 2) & (y0 >= 0) & (y0 <= Hm - 2)
    xi = np.where(ok, x0, 0).astype(int); yi = np.where(ok, y0, 0).astype(int)
    fa = u - x0; fb = v - y0
    M = np.asarray(Im, np.float64)
    top = M[yi, xi] + fa * (M[yi, xi + 1] - M[yi, xi]); bot = M[yi + 1, xi] + fa * (M[yi + 1, xi + 1] - M[yi + 1, xi])
    e = top + fb * (bot - top) - np.asarray(I, np.float64)
    return np.where(ok, e, np.nan), u, v


def test_the_jacobian_against_central_differences_of_a_float64_residual():
    """e(xi) = e at T' = Exp(-xi) * T.  d_k(h) = (e(+h e_k) - e(-h e_k)) / 2h in float64, h = 1e-4, 2e-4.  What J_k may differ from d_k(h) by, per sample:
      * the truncation of the central difference, h^2/6 |e'''|: estimated a posteriori as |d_k(2h) - d_k(h)| / 3 (Richardson), asserted with 3 x that;
      * the float32 rounding of J: each J_k is a sum of two or three products of magnitude at most |a|_max * (1 + |Pc|_max) with a = (ax, ay, az), about a
        dozen roundings of 2^-24 behind each; 64 * 2^-24 of that magnitude is taken;
      * the float32 rounding of the point J is taken at: u, v carry a few ulps of a coordinate below 64, 2^-16 pixel, and the bilinear gradient
        changes by at most D2 per pixel, D2 the largest second difference of the model image (xx, yy and xy): D2 * 2^-16 * S_k, S_k the pixels the
        projection moves per unit of xi_k (from the same central differences of u and v);
      * where the +-2h stencil leaves the sample's cell the bilinear surface has a crease: its gradient jumps by at most D2 there, and the central
        difference averages the two sides: D2 * S_k.  These samples must be few (h * S_k pixels wide bands): at most 2 % of the used ones.
    The tolerance is small against J: asserted, so that the comparison cannot pass on a J that is wrong."""
    D, I, K4, T, Dm, Im, Km, Tm = _smooth_scene(3)
    rw, cls = P.rows(D, None, I, K4, T, P.pack_model(Dm, Im), Km, Tm, 0.5, 5.5, 100.0, 255.0)
    used = cls == P.USED
    assert used.sum() > 300
    M = Im.astype(np.float64)
    D2 = max(np.abs(np.diff(M, 2, axis=1)).max(), np.abs(np.diff(M, 2, axis=0)).max(), np.abs(np.diff(np.diff(M, 1, axis=0), 1, axis=1)).max())
    e0, u0, v0 = _e64(D, I, K4, T, Im, Km, Tm)
    # the magnitude behind the float32 rounding of J, from the restated rows' own inputs in float64
    H, W = D.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Pc_max = np.maximum(np.abs((x - K4[2]) / K4[0] * D), np.maximum(np.abs((y - K4[3]) / K4[1] * D), D))
    h = 1e-4
    n_crossing = 0
    for k in range(6):
        d = {}
        for hh in (h, 2 * h):
            xi = np.zeros(6); xi[k] = hh
            ep, up, vp = _e64(D, I, K4, A.exp_se3(-xi) @ T.astype(np.float64), Im, Km, Tm)
            em, um, vm = _e64(D, I, K4, A.exp_se3(xi) @ T.astype(np.float64), Im, Km, Tm)
            same_cell = (np.floor(up) == np.floor(u0)) & (np.floor(um) == np.floor(u0)) & (np.floor(vp) == np.floor(v0)) & (np.floor(vm) == np.floor(v0))
            d[hh] = ((ep - em) / (2 * hh), np.hypot(up - um, vp - vm) / (2 * hh), same_cell)
        dk, S, _ = d[h]
        inside = d[2 * h][2]
        # |a|_max from |J_k| itself is circular; take it from the gradient of the float64 residual by the pixel: |a| <= max(fxm, fym) * G / Zm * (1 + |Pm|/Zm), bounded by S-free terms
        G = np.abs(np.stack([rw[..., 0], rw[..., 1], rw[..., 2]], -1).astype(np.float64)).max(-1)        # |gc|_max = |a|_max up to rotation: within sqrt(3)
        tol = 3 * np.abs(d[2 * h][0] - dk) / 3 + 64 * 2.0 ** -24 * (2 * G) * (1 + Pc_max) + D2 * 2.0 ** -16 * S + np.where(inside, 0.0, D2 * S)
        sel = used & np.isfinite(dk) & np.isfinite(d[2 * h][0])
        assert sel.sum() >= 0.98 * used.sum()
        n_crossing += (sel & ~inside).sum()
        err = np.abs(rw[..., k].astype(np.float64) - dk)
        assert (err[sel] <= tol[sel]).all(), (k, float((err[sel] / tol[sel]).max()))
        tight = sel & inside
        assert np.median(tol[tight]) < 1e-3 * np.abs(rw[..., k][tight]).max(), k                       # the tolerance is no loophole
        assert np.median(err[tight]) < 1e-3 * np.median(np.abs(rw[..., k][tight])), k
    assert n_crossing <= 0.02 * 6 * used.sum()


def _random_scene(seed, W=37, H=29, Wm=41, Hm=23):
    """Holes, masks, NaNs, a depth step in the model: every class occurs"""
    rng = np.random.default_rng(seed)
    D = rng.uniform(1.0, 6.0, (H, W)).astype(F)
    D[rng.random((H, W)) < 0.05] = 0.0
    mask = (rng.random((H, W)) < 0.1).astype(np.int32) * 3
    I = rng.integers(0, 256, (H, W)).astype(F)
    Dm = rng.uniform(1.0, 6.0, (Hm, Wm)).astype(F); Dm[rng.random((Hm, Wm)) < 0.03] = 0.0
    Im = rng.uniform(0, 255, (Hm, Wm)).astype(F); Im[rng.random((Hm, Wm)) < 0.02] = np.nan
    K4 = (30.0, 28.0, 18.2, 14.1); Km = (25.0, 26.0, 20.5, 11.0)
    T = A.perturbed(I4, (0.1, -0.05, 0.02), (1.0, 2.0, -1.5)); Tm = A.perturbed(I4, (-0.2, 0.1, 0.0), (-3.0, 1.0, 0.5))
    return D, mask, I, K4, T, P.pack_model(Dm, Im), Km, Tm


@pytest.mark.parametrize("s", [1, 2, 3])
def test_every_tree_sum_is_within_its_bound_of_the_exact_sum_and_the_counts_add_up(s):
    """As the aligner's: a pair tree over N values is off by at most log2(N) * 2^-53 * sum|term|, far inside the N * 2^-52 * sum|term| asserted."""
    D, mask, I, K4, T, model, Km, Tm = _random_scene(5 + s)
    rw, cls = P.rows(D, mask, I, K4, T, model, Km, Tm, 0.5, 5.5, 3.0, 200.0, s)
    sums, counts, _ = P.linearise(D, mask, I, K4, T, model, Km, Tm, 0.5, 5.5, 3.0, 200.0, s)
    Ws, Hs = A.grid(37, 29, s)
    assert counts.sum() == Ws * Hs and (counts > 0).all(), counts
    t = A.terms(rw).reshape(-1, 28)
    N = A.slot_vector(A.terms(rw)).shape[0]
    for k in range(28):
        exact = math.fsum(t[:, k].tolist())
        assert abs(sums[k] - exact) <= N * 2.0 ** -52 * math.fsum(np.abs(t[:, k]).tolist()), k
    assert (t[cls.ravel() != P.USED] == 0).all() and not np.signbit(t[cls.ravel() != P.USED]).any()      # a skipped sample contributes +0.0
    assert (rw[cls == P.USED][:, 7] == 1).all() and (rw[cls != P.USED] == 0).all()


# ---- the grey formula --------------------------------------------------------------------------------------------------------------------------
def test_grey_stays_grey_and_nothing_saturates():
    v = np.arange(256, dtype=np.uint8)
    grey3 = np.stack([v, v, v], -1)[None]
    assert np.array_equal(P.grey(grey3), v[None].astype(F)) and np.array_equal(P.grey(grey3, 1), v[None].astype(F))
    assert np.array_equal(P.grey(np.concatenate([grey3, np.full((1, 256, 1), 77, np.uint8)], -1)), v[None].astype(F))       # the fourth channel is ignored
    assert np.array_equal(P.grey(v[None]), v[None].astype(F)) and np.array_equal(P.grey(v[None, :, None]), v[None].astype(F))
    # all 2^24 colours: within 0 .. 255, the extremes only from black and white's neighbourhood, and the formula is the rounded weighted mean
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    Y = P.grey(np.stack([r, g, b], -1).reshape(256, 65536, 3).astype(np.uint8)).reshape(256, 256, 256)
    assert Y.min() == 0 and Y.max() == 255 and Y[0, 0, 0] == 0 and Y[255, 255, 255] == 255
    assert np.array_equal(Y, np.floor((77 * r + 150 * g + 29 * b) / 256.0 + 0.5).astype(F))
    assert P.grey(np.array([[[255, 0, 0]]], np.uint8))[0, 0] == 77 and P.grey(np.array([[[255, 0, 0]]], np.uint8), 1)[0, 0] == 29
    assert Y.dtype == F and np.array_equal(Y, np.rint(Y))                   # stored as floats, exactly


# ---- accuracy: a textured wall ------------------------------------------------------------------------------------------------------------------
WALL_WEIGHT = 0.01                                                           # metres per grey level
# the frame's true pose against the model's (I): 0.10 m, -0.07 m in the plane (1.46 pixel footprints of 1/12 m), 0.03 m towards it, and a small turn
WALL_XI = (0.10, -0.07, 0.03, 0.01, -0.015, 0.02)


def wall_case():
    """-> (frame depth, frame grey (quantised as a uint8 image is), T_true, T_init = I, model depth, model gradient for the aligner, model grey)"""
    T_true = A.exp_se3(np.array(WALL_XI)).astype(F)
    D, If = P.wall_render(T_true)
    Dm, Im = P.wall_render(I4)
    Gm = np.broadcast_to(np.array([0.0, 0.0, -1000.0], F), Dm.shape + (3,)).copy()      # the wall's gradient as the raycaster would give it: towards the camera
    return D, np.rint(If).astype(F), T_true, I4.copy(), Dm, Gm, np.rint(Im).astype(F)


def _eig_ratio(sums):
    Am = np.zeros((6, 6))
    for t, (r, c) in enumerate(A.UPPER):
        Am[r, c] = Am[c, r] = sums[t]
    ev = np.linalg.eigvalsh(Am)
    return ev[0] / ev[-1]


def wall_solve(geo=True, photo=True):
    w = P.WALL
    D, If, T_true, T_init, Dm, Gm, Im = wall_case()
    K4 = w["K4"]
    geo_lin = (lambda T: A.linearise(D, None, K4, T, Dm, Gm, K4, I4, 0.0, 10.0, w["max_dist"])) if geo else None
    photo_lin = lambda T: P.linearise(D, None, If, K4, T, P.pack_model(Dm, Im), K4, I4, 0.0, 10.0, w["max_dist"], 255.0)
    if not photo:
        return A.solve(D, None, K4, T_init, Dm, Gm, K4, I4, 0.0, 10.0, w["max_dist"], 1, 6, w["max_iterations"], w["eps"]), T_true, T_init
    return P.solve(photo_lin, geo_lin, WALL_WEIGHT, T_init, 6, 6, w["max_iterations"], w["eps"]), T_true, T_init


def test_the_joint_solve_sees_what_the_aligner_cannot_in_front_of_a_wall():
    """A fronto-parallel wall 5 m away, 64 x 48 pixels, fx = 60 (footprint Z / fx = 83.3 mm), textured with four sinusoids whose shortest period is 17
    pixels; frame and model rendered analytically and quantised to whole grey levels; the start is 125.7 mm from the truth (122 mm of it in the
    plane, 1.46 footprints) and 1.54 degrees.
    Geometry only (the restated aligner against the analytic model): three columns of J are exactly 0, eigenvalue ratio 0, status 2 at once.
    Joint, weight 0.01 m per grey level: status 0, stopped by eps after 4 rounds at 0.565 mm (0.0068 footprints) and 0.0145 degrees; eigenvalue ratio
    of the joint A at the start 9.8e-4; RMS 40.07 -> 0.153 mm and 13.69 -> 0.573 grey levels (the quantisation's 0.29 twice over); 2950 + 2869 of 3072
    samples used.  The photometric rows alone reach 4.60 mm (0.055 footprints), 0.048 degrees in 7 rounds.  (Also in DESIGN.md section 4.4.)
    Asserted: the issue's conditions - the aligner alone is singular (ratio below 1e-9 or status 2); the joint system's eigenvalue ratio is at
    least 1e6 times the aligner's; the translation error ends below a tenth of its start and below half a footprint."""
    w = P.WALL
    foot = w["Z0"] / w["K4"][0]
    (Tg, rep_g, trace_g), T_true, T_init = wall_solve(photo=False)
    ratio_g = _eig_ratio(trace_g[0][1])
    print(f"wall, geometry only: status {rep_g['status']}, eigenvalue ratio {ratio_g:.3g}")
    assert ratio_g < 1e-9 or rep_g["status"] == 2
    assert rep_g["status"] == 2 and np.array_equal(Tg, T_init)
    (T, rep, trace), _, _ = wall_solve()
    ratio_j = _eig_ratio(P.combine(trace[0][1], trace[0][3], WALL_WEIGHT))
    dt0, dr0 = A.pose_error(T_init, T_true)
    dt, dr = A.pose_error(T, T_true)
    print(f"wall, joint: from {dt0 * 1e3:.1f} mm ({dt0 / foot:.2f} footprints), {dr0:.3f} deg to {dt * 1e3:.3f} mm ({dt / foot:.4f} footprints), {dr:.4f} deg in "
          f"{rep['iterations']} rounds, status {rep['status']}; eigenvalue ratio {ratio_j:.3g}; rms geo {rep['rms_geo_first'] * 1e3:.2f} -> {rep['rms_geo_last'] * 1e3:.3f} mm, "
          f"photo {rep['rms_photo_first']:.2f} -> {rep['rms_photo_last']:.3f} levels; used {rep['used_geo']} + {rep['used_photo']}")
    assert rep["status"] == 0
    assert ratio_j > 0 and ratio_j >= 1e6 * abs(ratio_g)
    assert dt < 0.1 * dt0 and dt < 0.5 * foot
    (Tp, rep_p, _), _, _ = wall_solve(geo=False)
    dtp, drp = A.pose_error(Tp, T_true)
    print(f"wall, photometric rows alone: to {dtp * 1e3:.3f} mm ({dtp / foot:.4f} footprints), {drp:.4f} deg in {rep_p['iterations']} rounds, status {rep_p['status']}")


# ---- the library's host functions ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_vdo_photo_combine_and_the_joint_step_equal_the_restatement_bit_for_bit_without_a_device():
    from vdo_slam_amd import align as AL
    from vdo_slam_amd import photo as PH
    w = P.WALL
    D, If, T_true, T_init, Dm, Gm, Im = wall_case()
    K4 = w["K4"]
    T = A.perturbed(T_init, (0.01, 0.02, -0.01), (0.3, -0.2, 0.4))           # the aligner's columns are not exactly zero here
    sg, cg, _ = A.linearise(D, None, K4, T, Dm, Gm, K4, I4, 0.0, 10.0, w["max_dist"])
    sp, cp, _ = P.linearise(D, None, If, K4, T, P.pack_model(Dm, Im), K4, I4, 0.0, 10.0, w["max_dist"], 255.0)
    for weight in (WALL_WEIGHT, 0.37, 1.0, 3e-5):
        for geo in (sg, None):
            got = PH.combine(geo, sp, weight); want = P.combine(geo, sp, weight)
            assert np.array_equal(_bits(got), _bits(want)), (weight, geo is None)
            used = int(cp[0]) + (int(cg[0]) if geo is not None else 0)
            g_status, g_T, g_xi, g_rms = AL.step(got, used, 6, T)
            w_status, w_T, w_xi, w_rms = P.step(want, used, 6, T)
            assert g_status == w_status == 0
            assert np.array_equal(_bits(g_xi), _bits(w_xi)) and np.array_equal(_bits(g_T), _bits(w_T)) and g_rms == w_rms
    neg = np.where(np.arange(28) % 3 == 0, -0.0, sp)                          # a -0.0 keeps its sign against a NULL geo's +0.0 only when lam * photo is not -0.0 ...
    assert np.array_equal(_bits(PH.combine(None, neg, 0.5)), _bits(P.combine(None, neg, 0.5))) and not np.signbit(PH.combine(None, neg, 0.5)[0])
    assert np.array_equal(_bits(PH.combine(neg, neg, 0.5)), _bits(P.combine(neg, neg, 0.5))) and np.signbit(PH.combine(neg, neg, 0.5)[0])
    # refusals: nothing is written
    L = PH._lib()
    out = np.full(28, -7.0)
    assert L.vdo_photo_combine(sg.ctypes.data, None, 0.5, out.ctypes.data) == -1 and L.vdo_photo_combine(sg.ctypes.data, sp.ctypes.data, 0.5, None) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.vdo_photo_combine(sg.ctypes.data, sp.ctypes.data, bad, out.ctypes.data) == -1 and (out == -7).all(), bad
    both = sp.copy()
    assert L.vdo_photo_combine(sg.ctypes.data, both.ctypes.data, 0.5, both.ctypes.data) == 0 and np.array_equal(_bits(both), _bits(P.combine(sg, sp, 0.5)))     # out may be photo
