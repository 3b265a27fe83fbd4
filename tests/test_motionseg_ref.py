"""CPU: the properties of the motion segmenter's NumPy restatement (tests/motionseg_ref.py) - hand cases with a known answer, every unknown
rule, the vote at the corners - and its accuracy on two rendered frames with the oracle's RANSAC as the ego-motion.  The device inherits all of
it through array_equal (tests/test_motionseg_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import motionseg_ref as R
from vdo_slam_amd import _capi as K

F = np.float32
K4 = (128.0, 128.0, 8.0, 6.0)                             # powers of two: the hand cases below are exact in fp32
BF, UNIT = 50.0, 4.0
I4 = np.eye(4, dtype=np.float32)


def _scene(H=12, W=16, d=5.0):
    """A fronto-parallel wall at disparity d under the identity motion: zero flow, equal disparities"""
    disp = np.full((H, W), d * UNIT, F)
    return disp, disp.copy(), np.zeros((H, W, 2), F)


def _res(disp0, disp1, flow, T=I4, valid=None, **prm):
    return R.residual(disp0, disp1, flow, valid, T, K4, BF, UNIT, **prm)


def test_an_exact_rigid_motion_has_residual_zero():
    d0, d1, fl = _scene()
    st, e = _res(d0, d1, fl)
    assert (st == 0).all() and (e == 0).all()
    # a pure translation along the axis by tz, chosen so that every number is exact in fp32: Z = 50 / 5 = 10 -> Z' = 8, d' = 6.25; the pixel on the
    # principal point stays where it is
    T = I4.copy(); T[2, 3] = -2.0
    d1 = np.full_like(d0, 6.25 * UNIT)
    st, e = _res(d0, d1, fl, T)
    assert st[6, 8] == 0 and e[6, 8] == 0
    # and its neighbour (x - cx = 1): X = 10 / 128, u' = 128 * X / 8 + 8 = 9.25: a flow of 0.25 puts it there exactly
    fl[6, 9] = (0.25, 0.0)
    st, e = _res(d0, d1, fl, T)
    assert st[6, 9] == 0 and e[6, 9] == 0


def test_a_pure_disparity_change_flags_moving():
    d0, d1, fl = _scene()
    d1[3, 4] = (5.0 + 2.0) * UNIT                         # dd = 2 px at sigma 0.5: e = 16 > 9
    st, e = _res(d0, d1, fl)
    assert st[3, 4] == 1 and e[3, 4] == F(16) and (np.delete(st.ravel(), 3 * 16 + 4) == 0).all()
    fl[2, 2] = (1.0, 0.0)                                 # and a pure flow change of 1 px: e = 4, static; of 2 px: e = 16, moving
    fl[2, 5] = (0.0, -2.0)
    st, e = _res(d0, d1, fl)
    assert (st[2, 2], e[2, 2]) == (0, F(4)) and (st[2, 5], e[2, 5]) == (1, F(16))


def test_e_on_both_sides_of_chi2():
    d0, d1, fl = _scene()
    fl[1, 1] = (1.5, 0.0)                                 # e = 9 exactly: not > chi2
    st, e = _res(d0, d1, fl, chi2=9.0)
    assert e[1, 1] == F(9) and st[1, 1] == 0
    st, _ = _res(d0, d1, fl, chi2=float(np.nextafter(F(9), F(0))))
    assert st[1, 1] == 1
    st, _ = _res(d0, d1, fl, chi2=0.0)                    # chi2 = 0: only an exact fit is static
    assert st[1, 1] == 1 and st[0, 0] == 0


@pytest.mark.parametrize("rule", ["d0 zero", "d0 negative", "d0 nan", "d0 inf", "d0 below min", "flow nan", "flow inf", "left", "right", "up", "down", "flag", "d1 zero",
                                  "d1 negative", "d1 nan", "d1 inf", "behind", "e overflows"])
def test_every_unknown_rule_alone(rule):
    d0, d1, fl = _scene()
    H, W = d0.shape
    y, x = 5, 7
    valid, T, prm = None, I4, {}
    if rule == "d0 zero": d0[y, x] = 0
    elif rule == "d0 negative": d0[y, x] = -4
    elif rule == "d0 nan": d0[y, x] = np.nan
    elif rule == "d0 inf": d0[y, x] = np.inf
    elif rule == "d0 below min":
        d0[y, x] = np.nextafter(F(3.0 * UNIT), F(0)); prm = dict(min_disparity=3.0)
    elif rule == "flow nan": fl[y, x, 1] = np.nan
    elif rule == "flow inf": fl[y, x, 0] = -np.inf
    elif rule == "left": fl[y, x, 0] = -(x + 0.51)
    elif rule == "right": fl[y, x, 0] = W - 1 - x + 0.5   # the tie rounds up, out of the image
    elif rule == "up": fl[y, x, 1] = -(y + 0.51)
    elif rule == "down": fl[y, x, 1] = H - 1 - y + 0.5
    elif rule == "flag":
        valid = np.ones((H, W), np.uint8); valid[y, x] = 0
    elif rule == "d1 zero": d1[y, x] = 0
    elif rule == "d1 negative": d1[y, x] = -1
    elif rule == "d1 nan": d1[y, x] = np.nan
    elif rule == "d1 inf": d1[y, x] = np.inf
    elif rule == "behind":
        T = I4.copy(); T[2, 3] = -10.0                    # Z' = 0 for the whole wall
    elif rule == "e overflows": d1[y, x] = F(3e20)        # finite, and its square is not
    st, e = _res(d0, d1, fl, T, valid, **prm)
    if rule == "behind":
        assert (st == 2).all() and (e == -1).all()
        return
    assert st[y, x] == 2 and e[y, x] == F(-1), rule
    others = np.ones((H, W), bool); others[y, x] = False
    assert (st[others] == 0).all()                        # one rule, one pixel
    if rule == "d0 below min":                            # at the value itself the pixel is known
        d0[y, x] = 3.0 * UNIT
        assert _res(d0, d1, fl, T, valid, **prm)[0][y, x] != 2


def test_targets_on_the_rounding_tie_and_the_last_pixel():
    d0, d1, fl = _scene()
    H, W = d0.shape
    d1[:, W - 1] = 9 * UNIT                               # only a read of the last column sees this
    fl[4, 3] = (W - 1 - 3 - 0.5, 0)                       # uo = W - 1.5: floor(uo + 0.5) = W - 1, the last pixel
    fl[4, 4] = (W - 1 - 4 - 0.5 - 0.25, 0)                # a quarter less: W - 2
    st, e = _res(d0, d1, fl)
    assert st[4, 3] == 1 and st[4, 4] == 1 and e[4, 3] > e[4, 4]


def test_vote_windows_at_the_corners():
    st = np.zeros((5, 6), np.uint8)
    st[0, 0] = 1; st[4, 5] = 1; st[0, 5] = 2
    cls, counts = R.vote(st, vote_radius=1, vote_num=1, vote_den=5, min_known=1, class_value=7)
    # corner windows hold 4 pixels, edge windows 6, inner ones 9: one moving pixel is more than a fifth of 4, not of 6 (6 > 5 holds: 1 * 5 > 1 * 6 is false)
    want = np.zeros((5, 6), np.uint8)
    want[0, 0] = 7; want[4, 5] = 7
    assert np.array_equal(cls, want) and counts == (2, 27, 1)
    cls, _ = R.vote(st, vote_radius=1, vote_num=1, vote_den=5, min_known=4, class_value=7)
    assert cls[0, 0] == 7 and cls[0, 5] == 0
    # the unknown corner has 3 known neighbours of 4: min_known 4 keeps it still even when they all move
    st2 = np.ones((5, 6), np.uint8); st2[0, 5] = 2
    assert R.vote(st2, vote_radius=1, min_known=4)[0][0, 5] == 0 and R.vote(st2, vote_radius=1, min_known=3)[0][0, 5] == 1
    # an unknown hole inside an object is filled, a lone moving pixel is dropped
    st3 = np.zeros((9, 9), np.uint8); st3[2:7, 2:7] = 1; st3[4, 4] = 2; st3[0, 8] = 1
    cls, _ = R.vote(st3, vote_radius=1, vote_num=1, vote_den=2, min_known=6)
    assert cls[4, 4] == 1 and cls[0, 8] == 0
    # radius 0 is the state itself
    assert np.array_equal(R.vote(st3, vote_radius=0, vote_num=0, vote_den=1, min_known=1)[0], (st3 == 1).astype(np.uint8))
    # (2r+1)^2 + 1 known pixels never exist
    assert not R.vote(st2, vote_radius=1, min_known=10)[0].any()


def test_sample_lists():
    d0, d1, fl = _scene(7, 10)
    d0[3, 4] = 0
    X, uv = R.samples(d0, fl, None, K4, BF, UNIT, 3)      # grid x = 1, 4, 7; y = 1, 4: (4, 3) is no grid point
    assert X.shape == (6, 3) and np.array_equal(uv, [[1, 1], [4, 1], [7, 1], [1, 4], [4, 4], [7, 4]])
    assert np.array_equal(X[:, 2], np.full(6, 10.0)) and X[0, 0] == float((F(1) - F(8)) * F(10) / F(128))
    d0[4, 4] = 0
    assert R.samples(d0, fl, None, K4, BF, UNIT, 3)[0].shape == (5, 3)
    assert R.samples(d0, fl, None, K4, BF, UNIT, 40)[0].shape == (0, 3)
    assert R.samples(d0, fl, None, K4, BF, UNIT, 1)[0].shape == (68, 3)


# ---- accuracy on rendered frames -------------------------------------------------------------------------------------------------------------
def _ransac(o, X, uv, K4d, iters, thr, conf=0.98):
    dp = K.c_double_p
    o.vdo_oracle_pnp_ransac_refit.argtypes = [C.c_int, dp, dp, dp, C.c_int, C.c_double, C.c_double, C.c_int, dp, K.c_uint8_p, K.c_int32_p, K.c_int32_p]
    T = np.zeros(16); inl = np.zeros(max(len(X), 1), np.uint8); its = C.c_int32(); bi = C.c_int32()
    K4d = np.array(K4d, np.float64)
    good = o.vdo_oracle_pnp_ransac_refit(len(X), K._dp(X), K._dp(uv), K._dp(K4d), iters, thr, conf, 1, K._dp(T), inl.ctypes.data_as(K.c_uint8_p), C.byref(its), C.byref(bi))
    return T.reshape(4, 4), good, its.value


@pytest.fixture(scope="module")
def rendered():
    from vdo_slam_amd import synth_seq as SQ
    Ts = SQ.camera_poses(2); objs = SQ.default_objects()
    out = {}
    for name, kw in (("exact", {}), ("bench noise", dict(flow_sigma=SQ.BENCH_FLOW_SIGMA, invalid_depth=SQ.BENCH_INVALID_DEPTH, zero_flow=SQ.BENCH_ZERO_FLOW))):
        out[name] = [SQ.render_frame(k, Ts, objs, **kw) for k in range(2)]
    return out


@pytest.mark.parametrize("inputs", ["exact", "quantised", "bench noise"])
def test_accuracy_on_rendered_frames(oracle, rendered, inputs):
    """The issue's conditions on synth_seq frames 0 and 1 at 1242 x 375: at least 50 inliers, translation error <= 5 mm, recall on object pixels
    >= 0.99, false moving pixels <= 0.005 of the others.  Measured (grid step 16, threshold 1.0 px, min_disparity bf / ThDepthBG, defaults
    otherwise), as samples / inliers / iterations / translation error / recall / false rate (false rate before the vote):
      exact        1281 / 1183 / 3 / 0.00 mm / 0.9993 / 0.0014 (0.0015)
      quantised    1283 / 1141 / 6 / 0.87 mm / 0.9993 / 0.0014 (0.0014)
      bench noise  1265 /  969 / 9 / 2.22 mm / 0.9993 / 0.0014 (0.0137)"""
    from vdo_slam_amd import synth, synth_frames as SF
    f0, f1 = rendered["bench noise" if inputs == "bench noise" else "exact"]
    unit = SF.DEPTH_MAP_FACTOR
    if inputs == "exact":                                 # the disparity before render_frame rounds it to 1/256 px
        with np.errstate(divide="ignore"):
            d0, d1 = [np.where(np.isfinite(f["depth_true"]) & (f["depth_true"] < 300), unit * SF.BF / f["depth_true"], 0).astype(F) for f in (f0, f1)]
        flow = f0["flow"]
    elif inputs == "quantised":                           # flow rounded to 1/4 px, integer disparities
        d0, d1 = [(np.rint(f["depth_raw"] / unit) * unit).astype(F) for f in (f0, f1)]
        flow = (np.rint(f0["flow"] * 4) / 4).astype(F)
    else:
        d0, d1, flow = f0["depth_raw"], f1["depth_raw"], f0["flow"]
    K4k = synth.KITTI_K
    prm = dict(min_disparity=SF.BF / SF.TH_DEPTH_BG)
    X, uv = R.samples(d0, flow, None, K4k, SF.BF, unit, 16, **prm)
    T, n_inl, its = _ransac(oracle, X, uv, K4k, 500, 1.0)
    T_true = f0["Tcw_next"] @ np.linalg.inv(f0["Tcw"])
    t_err = float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
    got = R.stages(d0, d1, flow, None, T.astype(F), K4k, SF.BF, unit, **prm)
    obj = f0["mask"] > 0
    moving = got["cls"] > 0
    recall = float(moving[obj].mean()); false = float(moving[~obj].mean())
    raw = got["state"] == 1
    known = got["state"] != 2
    print(f"{inputs}: {len(X)} samples, {n_inl} inliers, {its} iterations, translation error {1e3 * t_err:.2f} mm, recall {recall:.4f}, false {false:.4f}; "
          f"before the vote: recall {float(raw[obj & known].mean()):.4f}, false {float(raw[~obj & known].mean()):.4f}")
    assert n_inl >= 50
    assert t_err <= 5e-3
    assert recall >= 0.99
    assert false <= 0.005
