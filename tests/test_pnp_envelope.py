"""The catalogue of tests/pnp_envelope.py on the CPU oracle: every case is what it is there for (asserted from the oracle's result and
its subset draws), and the flags and count of every refit-less result are the vote of its own pose, restated in np.longdouble."""
import ctypes as C

import numpy as np
import pytest

from tests import pnp_envelope as PE
from vdo_slam_amd import _capi as K

_runs = {}


def oracle_result(oracle, case):
    """What the oracle makes of a catalogue case: computed once, shared, never modified."""
    if case.name not in _runs:
        r = PE.oracle_run(oracle, case)
        for a in (r["T"], r["inliers"]):
            a.setflags(write=False)
        _runs[case.name] = r
    return _runs[case.name]


def _subsets(oracle, n, m):
    oracle.vdo_oracle_ransac_subsets.argtypes = [C.c_int, C.c_int, K.c_int32_p]
    a = np.zeros((m, 4), np.int32)
    oracle.vdo_oracle_ransac_subsets(n, m, a.ctypes.data_as(K.c_int32_p))
    return a


def _plain_grid():
    return PE.cases(PE.GRID, refit=0, solver="ap3p")


# ---------------------------------------------------------------------------------------------- what the catalogue holds
def test_the_grid_is_the_whole_product_of_its_axes():
    g = _plain_grid()
    assert {(c.n, c.max_iterations, c.thr, c.confidence) for c in g} == {(n, m, t, p) for n in PE.GRID_N for m in PE.GRID_ITERS for t, p in PE.GRID_SETTINGS}
    assert set(PE.GRID_N) == {4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513} and set(PE.GRID_ITERS) == {0, 1, 63, 64, 65, 500, 777}
    assert set(PE.GRID_SETTINGS) == {(0.4, 0.98), (0.05, 0.98), (2.0, 0.5), (0.4, 1.0), (0.4, 0.0)}
    for solver, refit in (("ap3p", 1), ("grunert", 0), ("grunert", 1)):      # the (0.4, 0.98) column again
        col = PE.cases(PE.GRID, refit=refit, solver=solver)
        assert {(c.n, c.max_iterations, c.thr, c.confidence) for c in col} == {(n, m, 0.4, 0.98) for n in PE.GRID_N for m in PE.GRID_ITERS}
    assert {(c.hostile, c.n) for c in PE.cases(PE.HOSTILE)} == {(h, n) for h in PE.HOSTILE_KINDS for n in (65, 257)}
    assert all(len({c.solver for c in b}) == 1 and len(b) <= 8 for b in PE.batches(PE.CASES))


def test_camera2_batches_mix_cameras_and_thresholds():
    fx, fy, cx, cy = PE.SECOND_K
    assert fx != fy and abs(cx - PE.CAMERAS["kitti"][2]) > 100 and abs(cy - PE.CAMERAS["kitti"][3]) > 100
    cs = PE.cases(PE.CAMERA2)
    for a, b in zip(cs, cs[1:]):
        assert a.camera != b.camera
    for batch in PE.batches(PE.CASES):
        if batch[0].cls == PE.CAMERA2:
            assert {(c.camera, c.thr) for c in batch} == {("kitti", 0.4), ("kitti", 1.0), ("second", 0.4), ("second", 1.0)}


def test_the_mixed_call_is_laid_out_as_described():
    M = PE.MIXED
    assert len(M) == 40 and {c.max_iterations for c in M} == {0, 1, 37, 65, 500, 777}
    assert {c.n for c in M} == set(PE.GRID_N) | {0, 3}
    assert all((a.n, a.max_iterations) != (b.n, b.max_iterations) and a.n != b.n and a.camera != b.camera for a, b in zip(M, M[1:]))
    assert M[21].max_iterations == 0 and M[21].n >= 4 and 10 <= 21 < 30
    assert {(c.camera, c.thr) for c in M} == {("kitti", 0.4), ("kitti", 1.0), ("second", 0.4), ("second", 1.0)}
    assert max(c.max_iterations for c in M[:21]) == 777 and max(c.max_iterations for c in M[22:]) == 777     # the launch is sized by a member on either side


# ---------------------------------------------------------------------------------------------- what the oracle makes of it
def test_the_grid_reaches_its_four_situations(oracle):
    R = {c.name: oracle_result(oracle, c) for c in _plain_grid()}
    # (1) confidence 1: the budget never shrinks - all hypotheses run - and some winner lands in the last quarter of 777
    full = [c for c in _plain_grid() if c.confidence == 1.0 and c.n >= 63]
    assert all(R[c.name]["iterations_run"] == c.max_iterations for c in full)
    assert any(R[c.name]["best_iteration"] > 3 * 777 // 4 - 1 for c in full if c.max_iterations == 777)
    assert any(500 <= R[c.name]["best_iteration"] for c in full if c.max_iterations == 777)            # (a hypothesis only the 777-case has)
    # (2) confidence 0: the first model with more than 3 inliers ends the loop
    stop = [c for c in _plain_grid() if c.confidence == 0.0 and c.max_iterations >= 63]
    for c in stop:
        r = R[c.name]
        assert r["best_iteration"] >= 0 and r["iterations_run"] == r["best_iteration"] + 1 <= 10, c.name
    assert min(R[c.name]["iterations_run"] for c in stop) == 1 and max(R[c.name]["iterations_run"] for c in stop) >= 3
    # (3) 0.05 px on 4 or 5 noisy points: no hypothesis wins
    tight = [c for c in _plain_grid() if c.thr == 0.05 and c.n in (4, 5)]
    assert len(tight) == 14
    for c in tight:
        r = R[c.name]
        assert r["best_iteration"] == -1 and r["n_inliers"] == 0 and np.array_equal(r["T"], np.eye(4)) and not r["inliers"].any()
        assert r["iterations_run"] == c.max_iterations                       # (every hypothesis was looked at)
    # (4) one hypothesis: some sizes' first draw is no model at any setting, some sizes' is
    one = [c for c in _plain_grid() if c.max_iterations == 1]
    lost = {n for n in PE.GRID_N if n >= 63 and all(R[c.name]["best_iteration"] == -1 for c in one if c.n == n)}
    won = {n for n in PE.GRID_N if all(R[c.name]["best_iteration"] == 0 for c in one if c.n == n)}
    assert lost == {63, 64, 257} and won >= {65, 127, 129, 256, 513}
    # no hypotheses at all
    for c in _plain_grid():
        if c.max_iterations == 0:
            r = R[c.name]
            assert (r["n_inliers"], r["iterations_run"], r["best_iteration"]) == (0, 0, -1)
    # ordinary cases: a consensus near the 70 % of good points, found before the budget is used up
    for c in _plain_grid():
        if (c.thr, c.confidence) == (0.4, 0.98) and c.n >= 63 and c.max_iterations >= 63:
            r = R[c.name]
            assert 0.5 * (~c.scene()["outlier"]).sum() <= r["n_inliers"] <= (~c.scene()["outlier"]).sum() + 2 and r["iterations_run"] < c.max_iterations, c.name


def test_hypothesis_counts_are_a_prefix_of_each_other(oracle):
    """The draws depend on (n, count) through the RNG stream alone: a smaller count is a prefix of a larger one, so a case that stops
    before the smaller count has the same result at both - what lets the 63 / 64 / 65 cases be told apart only by the launch."""
    for n in (65, 257):
        a, b = _subsets(oracle, n, 777), _subsets(oracle, n, 65)
        assert np.array_equal(a[:65], b)
        assert all(len(set(r)) == 4 for r in a.tolist()) and a.min() >= 0 and a.max() < n


def test_solvers_and_refit_can_be_told_apart(oracle):
    diff = moved = checked = 0
    for c in PE.cases(PE.GRID, refit=0, solver="grunert"):
        a = oracle_result(oracle, c); b = oracle_result(oracle, PE.BY_NAME[c.name.replace("grunert", "ap3p")])
        diff += a["best_iteration"] >= 0 and not np.array_equal(a["T"], b["T"])
    for c in PE.cases(refit=1):
        a = oracle_result(oracle, c)
        if c.cls == PE.GRID:
            b = oracle_result(oracle, PE.BY_NAME[c.name.replace("_r1", "_r0")])
            assert (a["n_inliers"], a["iterations_run"], a["best_iteration"]) == (b["n_inliers"], b["iterations_run"], b["best_iteration"]) and np.array_equal(a["inliers"], b["inliers"])
            moved += a["best_iteration"] >= 0 and not np.array_equal(a["T"], b["T"])
        checked += a["n_inliers"] >= 12
    assert diff >= 40 and moved >= 100 and checked >= 100


def test_nonfinite_points_are_drawn_and_never_inliers(oracle):
    s65, s257 = _subsets(oracle, 65, 2), _subsets(oracle, 257, 2)
    assert s65[0, 3] == PE.NONFINITE_AT[65] and s257[1, 0] == PE.NONFINITE_AT[257]
    for c in PE.cases(PE.HOSTILE):
        if c.hostile not in ("nan_X", "nan_uv", "inf_X"):
            continue
        r = oracle_result(oracle, c); s = c.scene()
        X, uv = c.build()
        k = PE.NONFINITE_AT[c.n]
        assert s["bad"].sum() == 1 and s["bad"][k] and not (np.isfinite(X[k]).all() and np.isfinite(uv[k]).all())
        assert np.isfinite(np.delete(X, k, 0)).all() and np.isfinite(np.delete(uv, k, 0)).all()
        assert r["iterations_run"] >= 2                                      # the hypothesis that holds the point was examined ...
        assert r["best_iteration"] > (0 if c.n == 65 else 1)                 # ... and is not the winner
        assert not r["inliers"][k] and np.isfinite(r["T"]).all()
        good = ~s["outlier"] & ~s["bad"]
        assert r["n_inliers"] >= 0.5 * good.sum()


def test_degenerate_scenes(oracle):
    for c in PE.cases(PE.HOSTILE):
        r = oracle_result(oracle, c); s = c.scene()
        X, uv = c.build()
        good = ~s["outlier"] & ~s["behind"] & ~s["bad"]
        if c.hostile == "collinear":
            d = X - X[0]
            assert np.linalg.matrix_rank(d, tol=1e-9) == 1
            # no valid hypothesis: nothing is ever counted, the whole budget is examined
            assert (r["n_inliers"], r["best_iteration"], r["iterations_run"]) == (0, -1, c.max_iterations)
            assert np.array_equal(r["T"], np.eye(4)) and not r["inliers"].any()
        elif c.hostile == "coplanar":
            assert np.linalg.matrix_rank(X - X.mean(0), tol=1e-9) == 2
            assert r["n_inliers"] >= 0.5 * good.sum() and np.abs(r["T"][:3, :3] - s["R"]).max() < 2e-2
        elif c.hostile == "behind":
            Xc = X @ s["R"].T + s["t"]
            assert np.array_equal(Xc[:, 2] < 0, s["behind"]) and 0.1 * c.n <= s["behind"].sum() <= 0.3 * c.n
            assert r["n_inliers"] >= 0.5 * good.sum() and np.abs(r["T"][:3, :3] - s["R"]).max() < 2e-2
        elif c.hostile == "dup8":
            assert (X[:8] == X[0]).all() and (uv[:8] == uv[0]).all() and len(np.unique(X, axis=0)) == c.n - 7
            assert r["n_inliers"] >= 0.5 * good.sum()
            assert len(set(r["inliers"][:8].tolist())) == 1                  # identical correspondences vote alike


def test_the_second_camera_is_the_one_the_points_were_seen_by(oracle):
    for c in PE.cases(PE.CAMERA2):
        if c.n < 64:
            continue
        r = oracle_result(oracle, c); s = c.scene()
        assert r["n_inliers"] >= 0.5 * (~s["outlier"]).sum()
        if c.camera == "second":            # ... and with KITTI's intrinsics the same pixels have no such consensus
            X, uv = c.build()
            e2 = PE.reproj_err2_longdouble(np.r_[np.c_[s["R"], s["t"]], [[0, 0, 0, 1]]], PE.CAMERAS["kitti"], X, uv)
            assert (e2 <= 1.0).sum() < 4


# ---------------------------------------------------------------------------------------------- the vote, restated
@pytest.mark.parametrize("cls", [PE.GRID, PE.CAMERA2, PE.HOSTILE, PE.MIXED_CLS])
def test_flags_and_count_are_the_vote_of_the_returned_pose(oracle, cls):
    cs = [c for c in PE.CASES + PE.MIXED if c.cls == cls and c.refit == 0]
    assert cs
    for c in cs:
        left_out = PE.check_vote(c, oracle_result(oracle, c))
        assert left_out <= 1, (c.name, left_out)        # known here, before any GPU run
