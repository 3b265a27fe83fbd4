"""The catalogue of tests/pose_paths.py on the CPU oracle: every case reaches the branch of the pose-only Levenberg loop it is there
for (asserted from the oracle's statistics: iterations, trials per iteration, stop reason), and every case that the GPU tests
compare trajectory for trajectory with the oracle keeps its trajectory when the inputs move by one ulp."""
import dataclasses

import numpy as np
import pytest

from tests import pose_paths as PP
from tests.pnp_envelope import SECOND_K
from tests.test_oracle_pose_only import run_oracle
from vdo_slam_amd import pose_only as PO

_runs = {}


def oracle_run(oracle, case):
    """(T, inliers, n_inliers, statistics) of a catalogue case: computed once, shared, never modified."""
    if case.name not in _runs:
        T, inl, ninl, st = run_oracle(oracle, case.build())
        T.setflags(write=False); inl.setflags(write=False)
        _runs[case.name] = (T, inl, ninl, st)
    return _runs[case.name]


def trace(st):
    return list(st.trials_trace[:st.iterations])


def point_chi2(prob, T):
    """Squared reprojection error of every correspondence at pose T (plain NumPy; NaN where obs is)."""
    X = prob.Xw @ T[:3, :3].T + T[:3, 3]
    if prob.kind == 0:
        fx, fy, cx, cy = prob.K
        pr = np.stack([X[:, 0] / X[:, 2] * fx + cx, X[:, 1] / X[:, 2] * fy + cy], 1)
    else:
        m = X @ prob.P[:, :3].T + prob.P[:, 3]
        pr = m[:, :2] / m[:, 2:3]
    return ((prob.obs - pr) ** 2).sum(1)


def _ids(cs):
    return [c.name for c in cs]


# ---------------------------------------------------------------------------------------------- which branch a case takes
# iterations, trials, stop reason, inliers and the trials of every iteration (1: accepted at once; k: k - 1 rejected trials - lambda
# *= ni, ni *= 2 each time - then an accepted one, since no iteration here has 10 and every one but the last is followed by another)
REJECTION_TABLE = {
    "rej_cam_n65_s1_t50": (15, 27, 1, 0, "1 1 1 5 2 2 2 1 2 2 1 2 1 2 2"),
    "rej_cam_n65_s4_t2": (43, 61, 1, 0, "1 1 1 1 1 1 1 1 4 1 3 1 2 1 1 1 1 1 3 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 5 1 1 1 4 1 4 1 1"),
    "rej_cam_n257_s8_t50": (10, 18, 1, 0, "1 1 1 5 3 3 1 1 1 1"),
    "rej_cam_n257_s8_t2": (23, 34, 1, 0, "1 1 1 1 1 1 1 1 1 1 1 1 1 1 5 1 3 1 3 1 3 1 2"),
    "rej_cam_n257_s6_t50": (10, 13, 1, 207, "1 2 3 1 1 1 1 1 1 1"),
    "rej_cam_n513_s5_t20": (10, 17, 1, 0, "1 1 1 1 1 1 1 5 1 4"),
    "rej_cam_n513_s0_t50": (12, 18, 1, 403, "1 1 1 3 3 3 1 1 1 1 1 1"),
    "rej_cam_n513_s2_t50": (12, 16, 1, 411, "1 2 4 1 1 1 1 1 1 1 1 1"),
    "rej_obj_n65_s0_t2": (10, 15, 1, 0, "1 1 1 1 5 1 1 1 1 2"),
    "rej_obj_n65_s4_t2": (22, 39, 1, 0, "1 2 1 1 1 1 1 1 2 3 3 2 1 3 4 2 2 1 2 1 2 2"),
    "rej_obj_n257_s0_t2": (8, 18, 1, 0, "2 1 4 2 5 1 2 1"),
    "rej_obj_n257_s3_t20": (14, 21, 1, 0, "1 1 1 1 1 1 5 1 2 1 2 1 1 2"),
    "rej_obj_n257_s7_t50": (17, 21, 1, 79, "1 1 1 1 1 1 1 1 2 3 1 2 1 1 1 1 1"),
    "rej_obj_n513_s6_t50": (29, 48, 1, 0, "1 1 1 1 4 2 2 2 2 2 1 2 2 1 2 2 1 2 2 1 2 1 2 1 2 2 1 2 1"),
    "rej_obj_n513_s10_t2": (6, 12, 1, 0, "1 6 1 1 2 1"),
    "rej_obj_n513_s11_t50": (21, 28, 1, 159, "1 1 1 1 1 1 1 1 1 3 2 2 2 3 1 1 1 1 1 1 1"),
}


def _rejecting_iterations(tr):
    """Indices of the iterations, the last one left out, that rejected at least one trial and then accepted one."""
    return [k for k, q in enumerate(tr[:-1]) if 2 <= q < 10]


@pytest.mark.parametrize("case", PP.cases(PP.REJECTION), ids=_ids(PP.cases(PP.REJECTION)))
def test_rejection_cases_reject_in_runs(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    tr = trace(st)
    assert (st.iterations, st.total_trials, st.stop_reason, ninl, " ".join(map(str, tr))) == REJECTION_TABLE[case.name]
    assert case.n > 64 and max(tr) < 10 and sum(tr) == st.total_trials
    # a second consecutive rejection (lambda *= ni; ni *= 2 twice), then an accepted trial from the state the rejections kept
    assert any(tr[k] >= 3 for k in _rejecting_iterations(tr))
    assert np.isfinite(T).all() and st.final_chi2 < st.initial_chi2


def test_some_large_case_of_each_kind_rejects_in_two_separate_iterations(oracle):
    assert set(REJECTION_TABLE) == {c.name for c in PP.cases(PP.REJECTION)}
    for kind in (0, 1):
        cs = PP.cases(PP.REJECTION, kind=kind)
        assert len(cs) >= 4 and {c.n for c in cs} == {65, 257, 513}
        again = []
        for c in cs:
            r = _rejecting_iterations(trace(oracle_run(oracle, c)[3]))
            if c.n >= 257 and len(r) >= 2 and r[-1] - r[0] >= 2:         # (an iteration of one trial between them: ni went back to 2)
                again.append(c.name)
        assert again, kind


@pytest.mark.parametrize("case", PP.cases(PP.SIZE), ids=_ids(PP.cases(PP.SIZE)))
def test_size_cases_are_ordinary_runs(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    assert st.iterations >= 3 and st.stop_reason == 1 and st.final_chi2 < st.initial_chi2 and np.isfinite(T).all()
    if case.n >= 63:
        assert trace(st) == [1] * st.iterations          # the survey's finding: no rejection on more than one wave at the defaults


@pytest.mark.parametrize("case", PP.cases(PP.ITER_CAP), ids=_ids(PP.cases(PP.ITER_CAP)))
def test_iteration_cap_cases_end_at_their_cap(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    prob = case.build()
    assert st.iterations == st.total_trials == case.max_iterations == prob.max_iterations and st.stop_reason == 0
    free = run_oracle(oracle, dataclasses.replace(prob, max_iterations=100))[3]
    assert free.iterations > 2                            # not a stop that merely coincides with the cap
    if case.max_iterations == 0:
        # the classification is that of the initial pose
        assert st.final_chi2 == st.initial_chi2 and np.abs(T - prob.T0).max() < 1e-7
        chi = point_chi2(prob, prob.T0)
        clear = np.abs(chi - 0.01) > 1e-6
        assert np.array_equal((chi <= np.float32(0.01))[clear], inl.astype(bool)[clear]) and clear.sum() >= case.n - 2
    else:
        assert st.final_chi2 < st.initial_chi2
    assert ninl == {"cap0_cam_n257": 0, "cap1_cam_n257": 69, "cap2_cam_n257": 190, "cap0_obj_n257": 0, "cap1_obj_n257": 80, "cap2_obj_n257": 81}[case.name]


@pytest.mark.parametrize("case", PP.cases(PP.NONFINITE), ids=_ids(PP.cases(PP.NONFINITE)))
def test_nonfinite_cases_never_accept(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    prob = case.build()
    assert np.isnan(prob.obs[case.nan_at, 0]) and np.isfinite(np.delete(prob.obs.ravel(), 2 * case.nan_at)).all() and np.isfinite(prob.Xw).all()
    # one trial per iteration up to the problem's own cap, every chi2 NaN ...
    cap = 100 if case.kind == 0 else 200
    assert st.iterations == st.total_trials == cap == prob.max_iterations and st.stop_reason == 0 and trace(st) == [1] * cap
    assert np.isnan(st.initial_chi2) and np.isnan(st.final_chi2) and np.isnan(np.array(st.chi2_trace[:cap])).all()
    # ... nothing accepted: the pose is the initial one (as the run of no iterations returns it), and finite
    T_init = run_oracle(oracle, dataclasses.replace(prob, max_iterations=0))[0]
    assert np.array_equal(T, T_init) and np.isfinite(T).all()
    # the NaN point counts as an inlier (chi2 > gate is false) - and so does every other one: the stored errors are those of the last
    # trial, whose step came out of a NaN system
    assert inl[case.nan_at] == 1 and inl.all() and ninl == case.n
    assert ninl == int(inl.sum())


@pytest.mark.parametrize("case", PP.cases(PP.SETTINGS), ids=_ids(PP.cases(PP.SETTINGS)))
def test_settings_cases(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    prob = case.build()
    h, g = case.settings
    assert prob.K == SECOND_K and (prob.huber_delta, prob.chi2_gate) == (h, g) and st.iterations >= 3 and st.stop_reason == 1
    base = PO.make_pose_problem(case.n, seed=case.seed, kind=case.kind)
    assert not np.allclose(base.obs, prob.obs, atol=50.0) and (case.kind == 0 or not np.allclose(base.P, prob.P, atol=1.0))
    # the scene IS seen by that camera: the refined pose is near the truth, which it would not be through KITTI's intrinsics
    assert np.abs(T - prob.T_true).max() < (0.2 if h == 0.0 else 0.05)
    if g == 0.0:
        assert ninl == 0 and not inl.any()
    elif g == 1e9:
        assert ninl == case.n and inl.all()
    else:
        assert 0 < ninl < case.n


def test_settings_change_the_run(oracle):
    for kind in ("cam", "obj"):
        a = oracle_run(oracle, PP.BY_NAME[f"set_h0.0_g0.01_{kind}_n257"]); b = oracle_run(oracle, PP.BY_NAME[f"set_h1.0_g0.01_{kind}_n257"])
        c = oracle_run(oracle, PP.BY_NAME[f"set_h0.1_g0_{kind}_n257"]); d = oracle_run(oracle, PP.BY_NAME[f"set_h0.1_g1e+09_{kind}_n257"])
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(b[0], c[0])       # the robust kernel's width moves the minimum ...
        assert np.array_equal(c[0], d[0]) and c[3].total_trials == d[3].total_trials      # ... the gate only the classification


@pytest.mark.parametrize("case", PP.cases(PP.EXACT), ids=_ids(PP.cases(PP.EXACT)))
def test_exact_cases_start_at_the_rounding_floor(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    prob = case.build()
    assert np.array_equal(prob.T0, prob.T_true.astype(np.float32).astype(np.float64))
    assert 0 < st.initial_chi2 < 1e-6 and st.final_chi2 <= st.initial_chi2 and st.stop_reason == 1 and st.iterations >= 1
    assert ninl == case.n and np.abs(T - prob.T_true).max() < 1e-5


@pytest.mark.parametrize("case", PP.cases(PP.TRIAL_CAP), ids=_ids(PP.cases(PP.TRIAL_CAP)))
def test_trial_cap_cases_run_ten_trials_in_one_iteration(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    tr = trace(st)
    assert tr[-1] == 10 and max(tr[:-1]) < 10             # the cap ends the loop
    assert st.stop_reason == (2 if case.name in ("tcap_cam_n6_s1_t5.0", "tcap_cam_n6_s14_t1.0") else 1)


# ---------------------------------------------------------------------------------------------- stability
def ulp_copies(prob, seed, copies=8):
    """prob with every obs / Xw double moved one ulp up or down at random."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(copies):
        moved = {}
        for key in ("obs", "Xw"):
            a = getattr(prob, key)
            moved[key] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
        out.append(dataclasses.replace(prob, **moved))
    return out


def keeps_its_trajectory(oracle, case):
    T, inl, ninl, st = oracle_run(oracle, case)
    for q in ulp_copies(case.build(), seed=1234):
        T2, inl2, ninl2, st2 = run_oracle(oracle, q)
        if (st2.iterations, st2.total_trials, st2.stop_reason) != (st.iterations, st.total_trials, st.stop_reason) or trace(st2) != trace(st):
            return False
        if not np.array_equal(inl2, inl) or ninl2 != ninl or not np.abs(T2 - T).max() <= 1e-11:
            return False
        if np.isfinite(st.final_lambda) and not abs(st2.final_lambda - st.final_lambda) <= 1e-10 * abs(st.final_lambda):
            return False
    return True


@pytest.mark.parametrize("case", PP.cases(stable=True), ids=_ids(PP.cases(stable=True)))
def test_stable_cases_keep_their_trajectory_under_one_ulp(oracle, case):
    assert keeps_its_trajectory(oracle, case)


def test_trial_cap_cases_are_not_stable(oracle):
    assert not any(keeps_its_trajectory(oracle, c) for c in PP.cases(PP.TRIAL_CAP))


def test_catalogue_covers_every_class():
    for cls in PP.CLASSES:
        assert PP.cases(cls), cls
    for c in PP.CASES:
        if c.cls in (PP.REJECTION, PP.ITER_CAP, PP.NONFINITE, PP.SETTINGS) or (c.cls == PP.SIZE and c.n >= 63):
            assert c.stable, c.name
        if c.cls == PP.TRIAL_CAP:
            assert not c.stable
    assert {(c.kind, c.n) for c in PP.cases(PP.SIZE)} == {(k, n) for k in (0, 1) for n in (3, 4, 63, 64, 65, 255, 256, 257, 511, 513)}
    assert {(c.kind, c.max_iterations, c.n) for c in PP.cases(PP.ITER_CAP)} == {(k, m, 257) for k in (0, 1) for m in (0, 1, 2)}
    assert {(c.kind, c.nan_at, c.n) for c in PP.cases(PP.NONFINITE)} == {(k, i, 257) for k in (0, 1) for i in (3, 255, 256)}
    assert {(c.kind, c.settings, c.n) for c in PP.cases(PP.SETTINGS)} == {(k, s, 257) for k in (0, 1) for s in ((0.0, PP.GATE_DEFAULT), (1.0, PP.GATE_DEFAULT), (0.1, 0.0), (0.1, 1e9))}
    assert len(PP.CASES) < 100
