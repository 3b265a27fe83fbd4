"""CPU: vdo_rectify_plan of libvdo_hip.so (host code; the library loads without a GPU) against the NumPy restatement tests/rectify_ref.py:
map, validity image and count array_equal, on the restatement's fixtures and on the edges - an invalid frame, points behind the camera,
a folding distortion, the validity edge on each side - and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import rectify_ref as R
from vdo_slam_amd import _capi as K
from vdo_slam_amd import rectify as RC

I3 = R.IDENTITY_R
EUROC = dict(K4=R.EUROC_K, D=R.EUROC_D, R=R.EUROC_R, P4=R.EUROC_P, src_size=R.EUROC_SIZE, dst_size=R.EUROC_SIZE)

CASES = {
    "identity_65x17": dict(K4=(60.0, 50.0, 31.5, 8.25), D=(0,) * 5, R=I3, P4=(60.0, 50.0, 31.5, 8.25), src_size=(65, 17), dst_size=(65, 17)),
    "identity_kitti": dict(K4=R.KITTI_K, D=(0,) * 5, R=I3, P4=R.KITTI_K, src_size=R.KITTI_SIZE, dst_size=R.KITTI_SIZE),
    "identity_752x480": dict(K4=R.EUROC_K, D=(0,) * 5, R=I3, P4=R.EUROC_K, src_size=R.EUROC_SIZE, dst_size=R.EUROC_SIZE),
    "shift_65x17": dict(K4=(60.0, 50.0, 31.5, 8.25), D=(0,) * 5, R=I3, P4=(60.0, 50.0, 34.5, 6.25), src_size=(65, 17), dst_size=(65, 17)),
    "euroc": EUROC,
    "euroc_small": R.euroc_small(),
    # the rectified camera sees twice the raw field of view: an invalid frame all around
    "zoomed_out": dict(K4=R.euroc_small()["K4"], D=R.EUROC_D, R=R.EUROC_R, P4=(27.0, 27.0, 46.0, 31.5), src_size=(94, 60), dst_size=(94, 60)),
    # 80 degrees about y with a 120-degree rectified field of view: part of the destination looks behind the raw camera (Wc <= 0)
    "behind": dict(K4=(50.0, 50.0, 47.0, 30.0), D=(0.01, 0, 0, 0, 0), R=R.rotation((0, 1, 0), math.radians(80)), P4=(27.0, 27.0, 46.5, 29.5),
                   src_size=(94, 60), dst_size=(94, 60)),
    # a strong barrel term on a wide destination: the radial polynomial folds over; whatever the formulas give, equal on both sides
    "fold_over": dict(K4=(40.0, 40.0, 100.0, 18.0), D=(-0.5, 0, 0, 0, 0), R=I3, P4=(40.0, 40.0, 100.0, 18.0), src_size=(200, 37), dst_size=(200, 37)),
    "tangential_k3_4values": dict(K4=(70.0, 72.0, 40.0, 20.0), D=(0.1, -0.05, 0.003, -0.002), R=R.rotation((1, 2, 3), 0.05), P4=(65.0, 65.0, 41.0, 19.0),
                                  src_size=(80, 40), dst_size=(67, 45)),
    "all_five": dict(K4=(70.0, 72.0, 40.0, 20.0), D=(0.1, -0.05, 0.003, -0.002, 0.02), R=R.rotation((1, 2, 3), 0.05), P4=(65.0, 65.0, 41.0, 19.0),
                     src_size=(80, 40), dst_size=(257, 33)),
    # fx = 32 and cx' - cx = 1 + 1/32: qx = 32 u - 33 passes -33 and -1 on the left; the destination is wider than the source, so it passes
    # the right edge too.  cx' - cx = 1/32: qx = 32 u - 1 starts at -1; 0: qx = 32 u reaches 0 and 32 (Ws - 1); -1/32: qx = 32 u + 1 reaches
    # 32 (Ws - 1) + 1.  The same in y.
    "edge_a": dict(K4=(32.0, 32.0, 8.0, 4.0), D=(0,) * 5, R=I3, P4=(32.0, 32.0, 8.0 + 33 / 32, 4.0 + 33 / 32), src_size=(17, 9), dst_size=(21, 13)),
    "edge_b": dict(K4=(32.0, 32.0, 8.0, 4.0), D=(0,) * 5, R=I3, P4=(32.0, 32.0, 8.0 + 1 / 32, 4.0 + 1 / 32), src_size=(17, 9), dst_size=(21, 13)),
    "edge_c": dict(K4=(32.0, 32.0, 8.0, 4.0), D=(0,) * 5, R=I3, P4=(32.0, 32.0, 8.0 - 1 / 32, 4.0 - 1 / 32), src_size=(17, 9), dst_size=(21, 13)),
    "edge_0": dict(K4=(32.0, 32.0, 8.0, 4.0), D=(0,) * 5, R=I3, P4=(32.0, 32.0, 8.0, 4.0), src_size=(17, 9), dst_size=(21, 13)),
    "one_pixel": dict(K4=(1.0, 1.0, 0.0, 0.0), D=(0,) * 5, R=I3, P4=(1.0, 1.0, 0.0, 0.0), src_size=(1, 1), dst_size=(1, 1)),
}


def _params(c, n_cams=1):
    cam = RC.camera(c["K4"], c["D"], c["R"], c["src_size"])
    return RC.params(c["P4"], c["dst_size"], [cam] * n_cams)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_restatement(name):
    c = CASES[name]
    exp_m, exp_v, exp_n = R.plan(**c)
    m, v, n = RC.plan(_params(c))
    assert np.array_equal(m, exp_m) and np.array_equal(v, exp_v) and n == exp_n
    m1, v1, n1 = RC.plan(_params(c, 2), cam=1)
    assert np.array_equal(m1, exp_m) and n1 == exp_n


def test_cases_reach_what_they_are_for():
    W, H = 94, 60
    _, v, n = R.plan(**CASES["zoomed_out"])
    assert not v[0].any() and not v[-1].any() and not v[:, 0].any() and not v[:, -1].any() and v[H // 2, W // 2] and 0 < n < W * H
    c = CASES["behind"]
    Rm = np.asarray(c["R"]).reshape(3, 3)
    x = (np.arange(W) - c["P4"][2]) / c["P4"][0]
    assert ((Rm[0, 2] * x + Rm[2, 2]) <= 0).any() and 0 < R.plan(**c)[2] < W * H
    for name in ("edge_a", "edge_b", "edge_c", "edge_0"):
        _, v, _ = R.plan(**CASES[name])
        assert v.any() and not v.all()
    # the four edge values themselves, with validity by the contract's rule: -1 invalid, 0 valid, 32 (Ws - 1) valid, 32 (Ws - 1) + 1 invalid
    ma, va, _ = R.plan(**CASES["edge_a"]); mb, vb, _ = R.plan(**CASES["edge_b"]); mc, vc, _ = R.plan(**CASES["edge_c"])
    assert (ma[2, 1] == R.INVALID).all() and not va[2, 1]                  # qx = 32 - 33 = -1
    assert (mb[1, 0] == R.INVALID).all() and mb[1, 1].tolist() == [31, 31] and vb[1, 1]
    assert mb[1, 16].tolist() == [32 * 16 - 1, 31] and vb[1, 16] and not vb[1, 17]      # 32 * 17 - 1 = 32 (Ws - 1) + 31: invalid
    assert mc[0, 0].tolist() == [1, 1] and vc[0, 0] and mc[0, 15].tolist() == [32 * 15 + 1, 1] and vc[0, 15]
    assert not vc[0, 16]                                                   # qx = 32 (Ws - 1) + 1: one past the last column with weight 1
    mi, vi, _ = R.plan(**CASES["edge_0"])
    assert mi[0, 0].tolist() == [0, 0] and vi[0, 0] and mi[8, 16].tolist() == [32 * 16, 32 * 8] and vi[8, 16] and not vi[8, 17] and not vi[9, 16]


def _refused(prm, cam=0, needle=""):
    m = np.full((max(prm.height, 1), max(prm.width, 1), 2), 77, np.int32)
    v = np.full(m.shape[:2], 77, np.uint8)
    n = C.c_int32(77)
    L = RC._lib()
    rc = L.vdo_rectify_plan(C.byref(prm), cam, m.ctypes.data, v.ctypes.data, C.byref(n))
    msg = K.lib().vdo_last_error().decode()
    assert rc == -1, (rc, msg)
    assert needle in msg, msg
    assert (m == 77).all() and (v == 77).all() and n.value == 77          # a refusal writes nothing


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_parameters_are_refused(bad):
    c = CASES["all_five"]
    for field, count, needle in (("K4", 4, "K["), ("D", 5, "D["), ("R", 9, "R["), ("P4", 4, "P[")):
        for k in range(count):
            vals = list(c[field]); vals[k] = bad
            _refused(_params(dict(c, **{field: tuple(vals)})), needle=f"{needle}{k}]")


def test_other_refusals():
    c = CASES["all_five"]
    for field, k, val in (("K4", 0, 0.0), ("K4", 1, -1.0), ("P4", 0, 0.0), ("P4", 1, -2.0)):
        vals = list(c[field]); vals[k] = val
        _refused(_params(dict(c, **{field: tuple(vals)})), needle="not positive")
    _refused(_params(dict(c, dst_size=(0, 5))), needle="width")
    _refused(_params(dict(c, dst_size=(5, 0))), needle="height")
    _refused(_params(dict(c, src_size=(0, 5))), needle="src_width")
    _refused(_params(dict(c, src_size=(5, -1))), needle="src_height")
    _refused(_params(c), cam=1, needle="cam")
    _refused(_params(c), cam=-1, needle="cam")
    p = _params(c); p.n_cams = 3
    _refused(p, needle="n_cams")
    L = RC._lib()
    assert L.vdo_rectify_plan(None, 0, None, None, None) == -1 and b"params" in K.lib().vdo_last_error()
    assert L.vdo_rectify_plan(C.byref(_params(c)), 0, None, None, None) == -1 and b"map" in K.lib().vdo_last_error()
    big = _params(dict(c, dst_size=(1 << 14, (1 << 12) + 1)))
    assert L.vdo_rectify_plan(C.byref(big), 0, 1, None, None) == -4       # VDO_ERR_UNSUPPORTED before anything is written
