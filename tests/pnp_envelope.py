"""Catalogue of PnP RANSAC problems chosen for the edge of csrc/ransac.hip they sit on (tests/test_pnp_envelope.py asserts from the
oracle that each one is what it claims to be; tests/test_pnp_envelope_gpu.py runs k_ap3p_hyp / k_p3p_hyp / k_ransac_vote and the
host replay on them).  Scenes are seeded NumPy, with the camera as a parameter.  Classes:

  grid      n x max_iterations x (thr, confidence): the tail of the 64-thread hypothesis block (0, 1, 63, 64, 65, 500, 777
            hypotheses), the ballot, the two mask words per wave and the 256-thread stride of the vote (n around 64, 128, 256, and
            513), the clamps of the iteration budget (confidence 0 and 1), a gate nothing passes (0.05 px on 4 or 5 points) and a
            loose one (2 px).  30 % outliers from n >= 63, 0.1 px noise.  AP3P without the refit everywhere; on the (0.4, 0.98)
            column also Grunert's P3P, and both solvers with the EPnP refit.
  camera2   the same kind of scene seen by either of two cameras (fx != fy, another principal point) at either of two thresholds:
            consecutive cases differ in both, so a batch of them has problems with different PnpDev::K and thr2.
  hostile   an otherwise good scene (n = 65 and 257) with one NaN in X, one NaN in uv, one +Inf in X, 8 identical
            correspondences, all points on a line, all points on a plane, or 20 % of the points behind the camera.

MIXED is one call of 40 problems for the offsets (pt_off, hyp_off, mask_off) and the max_hyp-sized grid: sizes and hypothesis
counts that differ from neighbour to neighbour, members with 0 and 3 points and with 0 hypotheses, cameras and thresholds
interleaved.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

from vdo_slam_amd import _capi as K
from vdo_slam_amd.synth import KITTI_K, rotvec_to_R

GRID, CAMERA2, HOSTILE, MIXED_CLS = "grid", "camera2", "hostile", "mixed"

SECOND_K = (650.0, 710.5, 300.25, 410.75)        # fx != fy, principal point far from KITTI's (609.56, 172.85)
CAMERAS = {"kitti": tuple(KITTI_K), "second": SECOND_K}

GRID_N = (4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
GRID_ITERS = (0, 1, 63, 64, 65, 500, 777)
GRID_SETTINGS = ((0.4, 0.98), (0.05, 0.98), (2.0, 0.5), (0.4, 1.0), (0.4, 0.0))
HOSTILE_KINDS = ("nan_X", "nan_uv", "inf_X", "dup8", "collinear", "coplanar", "behind")
# the correspondence a non-finite value is written into: the FOURTH point of hypothesis 0 (n = 65: the point that picks among the
# minimal solver's solutions) and the FIRST point of hypothesis 1 (n = 257) - tests/test_pnp_envelope.py checks both against the draws
NONFINITE_AT = {65: 43, 257: 110}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    cls: str
    n: int
    max_iterations: int
    thr: float
    confidence: float
    solver: str = "ap3p"
    refit: int = 0
    camera: str = "kitti"
    hostile: str | None = None

    @property
    def K(self):
        return CAMERAS[self.camera]

    @property
    def flags(self):                     # vdo_pnp_problem.refit: bit 0 the EPnP refit, bit 1 Grunert's P3P
        return int(self.refit) | (2 if self.solver == "grunert" else 0)

    def scene(self):
        return scene(self.n, self.camera, self.hostile)

    def build(self):
        s = self.scene()
        return s["X"], s["uv"]


@functools.lru_cache(maxsize=None)
def scene(n, camera="kitti", hostile=None):
    """X [n,3], uv [n,2] (read-only, shared), the true pose and which points are outliers / behind the camera / not finite."""
    fx, fy, cx, cy = CAMERAS[camera]
    rng = np.random.default_rng([n, {"kitti": 0, "second": 1}[camera], 0 if hostile is None else 1 + HOSTILE_KINDS.index(hostile)])
    R = rotvec_to_R(rng.normal(0, 0.2, 3)); t = rng.normal(0, 1.0, 3)
    Xc = np.c_[rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)]
    behind = np.zeros(n, bool)
    if hostile == "collinear":
        Xc = np.array([-9.0, 1.5, 12.0]) + rng.uniform(0, 1, (n, 1)) * np.array([17.0, -2.5, 21.0])
    elif hostile == "coplanar":
        Xc[:, 2] = 20.0 + 0.3 * Xc[:, 0] - 0.5 * Xc[:, 1]
    elif hostile == "behind":
        behind = rng.random(n) < 0.2
        Xc[behind, 2] *= -1.0
    X = (Xc - t) @ R                                       # Xc = R X + t
    uv = np.c_[fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy] + rng.normal(0, 0.1, (n, 2))
    outlier = (rng.random(n) < 0.3) if n >= 63 else np.zeros(n, bool)
    uv[outlier] += rng.uniform(-60, 60, (int(outlier.sum()), 2))
    bad = np.zeros(n, bool)
    if hostile in ("nan_X", "nan_uv", "inf_X"):
        k = NONFINITE_AT[n]
        bad[k] = True
        if hostile == "nan_X":
            X[k, 1] = np.nan
        elif hostile == "nan_uv":
            uv[k, 0] = np.nan
        else:
            X[k, 2] = np.inf
    elif hostile == "dup8":
        X[:8] = X[0]; uv[:8] = uv[0]
        outlier[:8] = outlier[0]
    out = dict(X=np.ascontiguousarray(X), uv=np.ascontiguousarray(uv), R=R, t=t, outlier=outlier, behind=behind, bad=bad)
    for a in out.values():
        a.setflags(write=False)
    return out


def _grid():
    out = []
    for solver, refit, settings in (("ap3p", 0, GRID_SETTINGS), ("ap3p", 1, GRID_SETTINGS[:1]), ("grunert", 0, GRID_SETTINGS[:1]), ("grunert", 1, GRID_SETTINGS[:1])):
        for n in GRID_N:
            for m in GRID_ITERS:
                for thr, conf in settings:
                    out.append(Case(f"grid_n{n}_m{m}_t{thr}_c{conf}_{solver}_r{refit}", GRID, n, m, thr, conf, solver, refit))
    return out


def _camera2():
    out = []
    for k, (n, m) in enumerate((n, m) for n in (5, 64, 129, 257) for m in (65, 500)):
        for j, (cam, thr) in enumerate((("second", 0.4), ("kitti", 1.0), ("second", 1.0), ("kitti", 0.4))):
            out.append(Case(f"cam2_n{n}_m{m}_{cam}_t{thr}", CAMERA2, n, m, thr, 0.98, camera=cam, refit=(k + j) & 1))
    return out


def _hostile():
    return [Case(f"hostile_{h}_n{n}", HOSTILE, n, 500, 0.4, 0.98, hostile=h) for h in HOSTILE_KINDS for n in (65, 257)]


def _mixed():
    sizes = list(GRID_N)
    iters = (0, 1, 37, 65, 500, 777)
    out = []
    for k in range(40):
        n = sizes[k % len(sizes)]; m = iters[(5 * k + 1 + k // len(sizes)) % len(iters)]         # (every round of the sizes shifts the counts by one)
        if k == 6: n = 0
        if k == 17: n = 3
        if k == 21: m = 0               # no hypotheses, in the middle of the call (its neighbour 20 has none either, 22 has 500)
        cam = ("kitti", "second")[k & 1]; thr = (0.4, 1.0)[(k // 3) & 1]
        out.append(Case(f"mixed{k:02d}_n{n}_m{m}_{cam}_t{thr}", MIXED_CLS, n, m, thr, 0.98, camera=cam))
    return out


CASES = _grid() + _camera2() + _hostile()
MIXED = _mixed()
BY_NAME = {c.name: c for c in CASES + MIXED}
assert len(BY_NAME) == len(CASES) + len(MIXED)


def cases(cls=None, refit=None, solver=None):
    return [c for c in CASES if (cls is None or c.cls == cls) and (refit is None or c.refit == refit) and (solver is None or c.solver == solver)]


def batches(cs, size=8):
    """Consecutive cases in groups of ``size``; a group ends early where the solver changes (a call names one)."""
    out, cur = [], []
    for c in cs:
        if cur and (len(cur) == size or c.solver != cur[0].solver):
            out.append(cur); cur = []
        cur.append(c)
    if cur:
        out.append(cur)
    return out


# ---------------------------------------------------------------------------------------------- the vote, restated
def reproj_err2_longdouble(T, K4, X, uv):
    """Squared reprojection error of every correspondence under T, in np.longdouble (NaN where the correspondence is not finite)."""
    L = np.longdouble
    T = np.asarray(T, L); X = np.asarray(X, L); uv = np.asarray(uv, L)
    fx, fy, cx, cy = (L(v) for v in K4)
    with np.errstate(all="ignore"):
        Xc = X @ T[:3, :3].T + T[:3, 3]
        du = fx * Xc[:, 0] / Xc[:, 2] + cx - uv[:, 0]
        dv = fy * Xc[:, 1] / Xc[:, 2] + cy - uv[:, 1]
        return du * du + dv * dv


def check_vote(case, res):
    """The flags and the count of a refit-less result are the vote of its own pose: inliers[i] == (e2 <= thr^2) outside a band of
    1e-9 thr^2 around the gate; a correspondence that is not finite is no inlier.  Returns how many points were inside the band."""
    assert case.refit == 0
    X, uv = case.build()
    inl = np.asarray(res["inliers"]).astype(bool)
    assert res["n_inliers"] == int(inl.sum())
    if res["best_iteration"] < 0:
        assert not inl.any() and np.array_equal(res["T"], np.eye(4))
        return 0
    thr2 = np.longdouble(case.thr) * np.longdouble(case.thr)
    e2 = reproj_err2_longdouble(res["T"], case.K, X, uv)
    finite = np.isfinite(X).all(1) & np.isfinite(uv).all(1)
    assert not inl[~finite].any()
    with np.errstate(invalid="ignore"):
        clear = ~(np.abs(e2 - thr2) <= np.longdouble(1e-9) * thr2)        # (NaN: clear, and not an inlier)
        want = e2 <= thr2
    assert np.array_equal(inl[clear], want[clear]), np.flatnonzero(inl != want)
    return int((~clear).sum())


# ---------------------------------------------------------------------------------------------- the C-ABI with per-problem fields
def oracle_run(oracle, case):
    f = oracle.vdo_oracle_pnp_ransac_refit
    f.argtypes = [C.c_int, K.c_double_p, K.c_double_p, K.c_double_p, C.c_int, C.c_double, C.c_double, C.c_int, K.c_double_p, K.c_uint8_p, K.c_int32_p, K.c_int32_p]
    f.restype = C.c_int
    X, uv = case.build()
    n = X.shape[0]
    T = np.zeros(16); inl = np.zeros(max(n, 1), np.uint8); its = C.c_int32(); bi = C.c_int32()
    K4 = np.array(case.K, np.float64)
    good = f(n, K._dp(X), K._dp(uv), K._dp(K4), case.max_iterations, case.thr, case.confidence, case.flags, K._dp(T), inl.ctypes.data_as(K.c_uint8_p), C.byref(its), C.byref(bi))
    return dict(T=T.reshape(4, 4), n_inliers=good, iterations_run=its.value, best_iteration=bi.value, inliers=inl[:n])


def run_cases(ctx, cs, refit_above=None, flags=None):
    """One call of vdo_pnp_ransac_batch (refit_above None) or vdo_pnp_ransac_batch_gated (an int32 array) on the cases ``cs``, every
    vdo_pnp_problem filled from its own case.  ``flags``: vdo_pnp_problem.refit of every member instead of the cases' own."""
    from vdo_slam_amd.ransac import PnpProblemC, PnpResultC, HOOK
    n = len(cs)
    arr = (PnpProblemC * n)()
    keep, inl = [], []
    for i, c in enumerate(cs):
        X, uv = c.build()
        keep.append((X, uv))
        arr[i] = PnpProblemC(X.shape[0], K._dp(X), K._dp(uv), (C.c_double * 4)(*c.K), c.max_iterations, c.thr, c.confidence, c.flags if flags is None else flags[i])
        inl.append(np.zeros(max(X.shape[0], 1), np.uint8))
    res = (PnpResultC * n)()
    ip = (K.c_uint8_p * n)(*[a.ctypes.data_as(K.c_uint8_p) for a in inl])
    L = K.lib()
    if refit_above is None:
        L.vdo_pnp_ransac_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PnpProblemC), C.POINTER(PnpResultC), C.POINTER(K.c_uint8_p)]
        K.check(L.vdo_pnp_ransac_batch(ctx._h, n, arr, res, ip))
    else:
        gate = np.ascontiguousarray(refit_above, np.int32)
        assert gate.size == n
        L.vdo_pnp_ransac_batch_gated.argtypes = [C.c_void_p, C.c_int, C.POINTER(PnpProblemC), C.POINTER(PnpResultC), C.POINTER(K.c_uint8_p), K.c_int32_p, HOOK, C.c_void_p, HOOK, C.c_void_p]
        K.check(L.vdo_pnp_ransac_batch_gated(ctx._h, n, arr, res, ip, gate.ctypes.data_as(K.c_int32_p), HOOK(0), None, HOOK(0), None))
    return [dict(T=np.array(res[i].T).reshape(4, 4), n_inliers=res[i].n_inliers, iterations_run=res[i].iterations_run,
                 best_iteration=res[i].best_iteration, inliers=inl[i][:c.n]) for i, c in enumerate(cs)]
