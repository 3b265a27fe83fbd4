"""The catalogue of tests/flow2_paths.py on the CPU oracle: every case reaches the Levenberg branch it is there for (asserted from
the oracle's per-trial log, not inferred from counts), and every case that the GPU tests compare trajectory for trajectory with
the oracle keeps its trajectory when the inputs move by one ulp."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import flow2_paths as FP
from tests.test_oracle_flow2 import run_oracle
from vdo_slam_amd import _capi as K


class Flow2TrialC(C.Structure):      # vdo_flow2_trial, oracle/vdo_oracle.h
    _fields_ = [("iteration", C.c_int32), ("trial", C.c_int32), ("solved", C.c_int32), ("accepted", C.c_int32),
                ("lambda_", C.c_double), ("chi2", C.c_double), ("rho", C.c_double)]


LOG_CAPACITY = 2048       # 200 iterations of at most 10 trials


def run_oracle_log(oracle, prob, capacity=LOG_CAPACITY):
    """vdo_oracle_flow2_optimize_log: (T, flow, inliers, n_inliers, stats, the trials written, number of trials run)."""
    f = oracle.vdo_oracle_flow2_optimize_log
    f.argtypes = [C.POINTER(K.Flow2ProblemC), K.c_double_p, K.c_double_p, K.c_uint8_p, C.POINTER(K.LMStatsC), C.POINTER(Flow2TrialC), C.c_int32, K.c_int32_p]
    f.restype = C.c_int
    pc, keep = K.flow2_to_c(prob)
    T = np.zeros(16); flow = np.zeros((prob.n, 2)); inl = np.zeros(prob.n, np.uint8)
    st = K.LMStatsC()
    log = (Flow2TrialC * max(1, capacity))()
    nlog = C.c_int32(-1)
    ninl = f(C.byref(pc), K._dp(T), K._dp(flow), inl.ctypes.data_as(K.c_uint8_p), C.byref(st), log, capacity, C.byref(nlog))
    return T.reshape(4, 4), flow, inl, ninl, st, [log[i] for i in range(min(nlog.value, capacity))], nlog.value


_runs = {}


def oracle_run(oracle, case):
    """What the oracle makes of a catalogue case, with its trial log: computed once, shared, never modified."""
    if case.name not in _runs:
        _runs[case.name] = run_oracle_log(oracle, case.build())
    return _runs[case.name]


def by_iteration(log):
    return [list(g) for _, g in itertools.groupby(log, key=lambda r: r.iteration)]


def _ids(cs):
    return [c.name for c in cs]


# ---------------------------------------------------------------------------------------------- the log itself
_STATS_BYTES = K.LMStatsC.ms_total.offset      # everything the optimisation fills (the timing fields stay 0)


@pytest.mark.parametrize("case", FP.CASES, ids=_ids(FP.CASES))
def test_log_entry_point_has_the_bits_of_the_plain_one(oracle, case):
    T, flow, inl, ninl, st, log, nlog = oracle_run(oracle, case)
    T0, flow0, inl0, ninl0, st0 = run_oracle(oracle, case.build())
    assert ninl == ninl0 and T.tobytes() == T0.tobytes() and flow.tobytes() == flow0.tobytes() and inl.tobytes() == inl0.tobytes()
    assert bytes(st)[:_STATS_BYTES] == bytes(st0)[:_STATS_BYTES]
    # one record per trial, in order, and the counts the statistics already had
    assert nlog == len(log) == st.total_trials
    its = by_iteration(log)
    assert [g[0].iteration for g in its] == list(range(st.iterations))
    assert [len(g) for g in its] == list(st.trials_trace[:st.iterations])
    for g in its:
        assert [r.trial for r in g] == list(range(len(g)))
        assert all(not r.accepted for r in g[:-1])            # an accepted trial ends its iteration
    for r in log:
        # (a failed solve counts its chi2 as DBL_MAX, which is finite: with a negative scale such a trial IS accepted, as in g2o)
        assert r.accepted == (1 if (r.rho > 0 and np.isfinite(r.chi2)) else 0)
    # lambda: x ni (2, 4, 8, ...) after every rejection, ni back to 2 after an accepted trial
    ni = 2.0
    for a, b in zip(log, log[1:]):
        if a.accepted:
            ni = 2.0
            assert b.lambda_ <= a.lambda_ * (2. / 3.) * (1 + 1e-15) and b.lambda_ >= a.lambda_ / 3. * (1 - 1e-15)
        else:
            assert b.lambda_ == a.lambda_ * ni or np.isnan(a.lambda_)
            ni *= 2
    if log:
        last = log[-1]
        if np.isfinite(st.final_lambda) and not last.accepted:
            assert st.final_lambda == last.lambda_ * ni


def test_log_capacity_is_respected(oracle):
    case = FP.BY_NAME["rej_q0_n260_s0_obj"]
    full = oracle_run(oracle, case)
    T, flow, inl, ninl, st, log, nlog = run_oracle_log(oracle, case.build(), capacity=5)
    assert nlog == full[6] and len(log) == 5
    assert all(bytes(a) == bytes(b) for a, b in zip(log, full[5]))
    assert T.tobytes() == full[0].tobytes()
    assert run_oracle_log(oracle, case.build(), capacity=0)[6] == full[6]


def test_fewer_than_three_points_log_nothing(oracle):
    from vdo_slam_amd import synth
    assert run_oracle_log(oracle, synth.make_flow2_problem(2, seed=1))[5:] == ([], 0)


# ---------------------------------------------------------------------------------------------- which branch a case takes
# iterations, trials, stop reason and every trial of every iteration of the rejection cases (init_sigma_t = 5.0): A accepted,
# r rejected, f the reduced 6x6 solve failed (rejected - the trial the kernel skips - unless the stale step it leaves has a negative
# scale: "fA", accepted as in g2o).  The first 14 are the survey's rows, with its counts.
REJECTION_TABLE = {
    "rej_q0_n260_s0_obj": (23, 30, 1, "A A A A A A A A A A A A A A A A A A A A rrrrrrA A rA"),
    "rej_q0_n260_s1_cam": (12, 18, 1, "A A A A A A A A rrrrrrA A A A"),
    "rej_q0_n260_s7_obj": (14, 19, 1, "A A A A A A A A A A rrrrrA A A A"),
    "rej_q0_n520_s2_cam": (21, 27, 1, "A A A A A A A A A A A A A A A A A A rrrrrrA A A"),
    "rej_q0_n520_s3_cam": (18, 23, 1, "A A A A A A A A A A A A A A A A A rrrrrA"),
    "rej_q0_n2300_s6_obj": (10, 12, 1, "A A rrA A A A A A A A"),
    "rej_q0_n2300_s7_obj": (13, 15, 1, "rrA A A A A A A A A A A A A"),
    "rej_q1_n260_s2_cam": (21, 33, 1, "A A A A A A rrA rA A rA rA rA rA A rA rA A rA A rA rA"),
    "rej_q1_n260_s5_cam": (28, 35, 1, "A A A A A A A A A A A A A A A A A A A rrA rA rA A rA rA A A rA"),
    "rej_q1_n260_s3_obj": (5, 7, 2, "A rrA A A A"),
    "rej_q1_n520_s2_cam": (24, 33, 1, "A A A A A A A A A A A A A A A A A rA rrA A rrrrrrA A A A"),
    "rej_q1_n520_s1_obj": (7, 11, 2, "A A A rA frA fA A"),
    "rej_q1_n2300_s0_cam": (10, 14, 1, "A A A A fA ffA A A rA A"),
    "rej_q1_n2300_s5_obj": (7, 9, 2, "A A A A ffA A A"),
    "rej_q0_n2300_s10_cam": (16, 23, 1, "A A A A A A A A A A A rrrA A rrA A rrA"),
}
# The cases in which an iteration rejects again AFTER an earlier iteration's rejections were followed by an accepted trial.  The
# oracle shows this for these only, not for every row of the survey (the others reject in one iteration alone): it is asserted
# for each of them, and that both modes, the register store and the memory store have one.
REJECTS_AGAIN = ("rej_q0_n260_s0_obj", "rej_q0_n2300_s10_cam", "rej_q1_n260_s2_cam", "rej_q1_n260_s5_cam", "rej_q1_n520_s2_cam",
                 "rej_q1_n520_s1_obj", "rej_q1_n2300_s0_cam")


def pattern(log):
    return " ".join("".join("A" if r.accepted else ("r" if r.solved else "f") for r in g) for g in by_iteration(log))


def _rejects_again(its):
    after = [k for k, g in enumerate(its) if len(g) >= 2 and g[-1].accepted]
    return bool(after) and any(not r.accepted for g in its[after[0] + 1:] for r in g)


@pytest.mark.parametrize("case", FP.cases(FP.REJECTION), ids=_ids(FP.cases(FP.REJECTION)))
def test_rejection_cases_reject_in_runs(oracle, case):
    _, _, _, _, st, log, _ = oracle_run(oracle, case)
    its = by_iteration(log)
    assert (st.iterations, st.total_trials, st.stop_reason, pattern(log)) == REJECTION_TABLE[case.name]
    # a second consecutive rejection (lambda *= ni; ni *= 2 twice) in an iteration of at least 3 trials ...
    assert any(len(g) >= 3 and not g[0].accepted and not g[1].accepted for g in its)
    # ... an accepted trial after rejected ones: the state the rejections kept is what the accepted trial started from ...
    assert any(len(g) >= 2 and g[-1].accepted for g in its)
    # a later iteration rejects again, from the state that accepted trial left
    assert _rejects_again(its) == (case.name in REJECTS_AGAIN)


def test_some_case_rejects_again_in_every_mode_and_store():
    again = [FP.BY_NAME[name] for name in REJECTS_AGAIN]
    assert {c.quirks for c in again} == {0, 1}
    assert {(c.quirks, c.n > 2048) for c in again} == {(0, False), (0, True), (1, False), (1, True)}      # (n > 2048: the memory store)
    assert set(REJECTS_AGAIN) <= set(REJECTION_TABLE) == {c.name for c in FP.cases(FP.REJECTION)}


@pytest.mark.parametrize("case", FP.cases(FP.ITER_CAP), ids=_ids(FP.cases(FP.ITER_CAP)))
def test_iteration_cap_cases_end_at_their_cap(oracle, case):
    T, flow, inl, ninl, st, log, _ = oracle_run(oracle, case)
    assert st.iterations == case.build().max_iterations and st.stop_reason == 0
    if case.max_iterations == 0:
        assert not log and st.final_chi2 == st.initial_chi2 and np.array_equal(flow, case.build().flow)
    else:
        assert log[-1].accepted         # not a stop that merely coincides with the cap


@pytest.mark.parametrize("case", FP.cases(FP.NONFINITE), ids=_ids(FP.cases(FP.NONFINITE)))
def test_nonfinite_cases_never_accept(oracle, case):
    T, flow, inl, ninl, st, log, _ = oracle_run(oracle, case)
    assert log and all(not np.isfinite(r.chi2) for r in log) and not any(r.accepted for r in log)
    # one trial per iteration up to the problem's own cap; the pose never moves (and stays finite), every flag is set (NaN > gate is false)
    assert st.iterations == st.total_trials == 200 and st.stop_reason == 0
    assert np.isfinite(T).all() and ninl == case.n and inl.all()
    assert np.isnan(st.final_chi2) and np.isnan(flow[case.nan_at, 0]) and np.isfinite(np.delete(flow.ravel(), 2 * case.nan_at)).all()


@pytest.mark.parametrize("case", FP.cases(FP.TRIAL_CAP), ids=_ids(FP.cases(FP.TRIAL_CAP)))
def test_trial_cap_cases_run_ten_trials_in_one_iteration(oracle, case):
    _, _, _, _, st, log, _ = oracle_run(oracle, case)
    its = by_iteration(log)
    assert max(len(g) for g in its) == 10
    assert len(its[-1]) == 10 and st.stop_reason == 1           # the cap ends the loop


# ---------------------------------------------------------------------------------------------- stability
def _ulp_copies(prob, seed, copies=8):
    """prob with every obs / flow / depth double moved one ulp up or down at random."""
    import dataclasses
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(copies):
        moved = {}
        for key in ("obs", "flow", "depth"):
            a = getattr(prob, key)
            moved[key] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
        out.append(dataclasses.replace(prob, **moved))
    return out


@pytest.mark.parametrize("case", FP.cases(stable=True), ids=_ids(FP.cases(stable=True)))
def test_stable_cases_keep_their_trajectory_under_one_ulp(oracle, case):
    T, flow, inl, ninl, st, log, _ = oracle_run(oracle, case)
    for k, q in enumerate(_ulp_copies(case.build(), seed=1234)):
        T2, flow2, inl2, ninl2, st2 = run_oracle(oracle, q)
        assert (st2.iterations, st2.total_trials, st2.stop_reason) == (st.iterations, st.total_trials, st.stop_reason), k
        assert list(st2.trials_trace[:st2.iterations]) == list(st.trials_trace[:st.iterations]), k
        assert np.array_equal(inl2, inl) and ninl2 == ninl, k
        assert np.abs(T2 - T).max() <= 1e-11, k


def test_catalogue_covers_every_class_and_only_the_trial_cap_is_unstable():
    for cls in FP.CLASSES:
        assert FP.cases(cls), cls
    assert all(c.cls == FP.TRIAL_CAP for c in FP.cases(stable=False))
    assert len(FP.cases(stable=True)) >= 30
    assert len(FP.cases(FP.REJECTION)) >= 14 and len(FP.cases(FP.TRIAL_CAP)) >= 4
    assert {(c.n, c.quirks, c.max_iterations) for c in FP.cases(FP.ITER_CAP)} >= {(n, q, m) for n in (260, 2300) for q in (0, 1) for m in (0, 1, 3)}
    assert {(c.nan_at, c.quirks) for c in FP.cases(FP.NONFINITE)} == {(i, q) for i in (3, 129, 259) for q in (0, 1)}
