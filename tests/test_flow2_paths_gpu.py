"""k_flow2_lm on the catalogue of tests/flow2_paths.py: runs of rejected trials, the iteration and the trial cap, non-finite chi2
(the only way into the kernel's ``if (!built)``), on the register store and on the memory store, against the CPU oracle where the
trajectory is stable and store against store bit for bit everywhere; and the reserved slots of the frame pipeline
(vdo_flow2_batch_reserve / vdo_flow2_batch_set) reused frame after frame with changing sizes."""
import dataclasses

import numpy as np
import pytest

from tests import flow2_paths as FP
from tests.test_flow2_gpu import _check
from tests.test_flow2_paths import oracle_run
from tests.test_flow2_register_path_gpu import _run, _same_bits
from vdo_slam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def default_env(monkeypatch):
    monkeypatch.delenv("VDO_LM_GENERAL", raising=False)
    monkeypatch.delenv("VDO_LM_CLUSTER_BUDGET", raising=False)
    return monkeypatch


def _check_nonfinite(res, T, flow, inl, ninl, st):
    """A problem whose chi2 is NaN throughout: the pose never moves.  (final_lambda is left out: the kernel's fmax drops a NaN
    where the oracle's std::max keeps the one of the last landmark; nothing reads it.)"""
    assert np.abs(res["T"] - T).max() <= 1e-9
    assert (res["iterations"], res["trials"], res["stop_reason"], res["n_inliers"]) == (st.iterations, st.total_trials, st.stop_reason, ninl)
    assert np.array_equal(res["inliers"], inl)
    assert np.array_equal(res["flow"], flow, equal_nan=True)
    assert np.isnan(res["final_chi2"]) and np.isnan(st.final_chi2)


def _check_case(case, res, ref):
    T, flow, inl, ninl, st = ref[:5]
    if case.cls == FP.NONFINITE:
        _check_nonfinite(res, T, flow, inl, ninl, st)
    else:
        _check(res, T, flow, inl, ninl, st)


@pytest.mark.parametrize("quirks", [1, 0])
def test_stable_cases_match_the_oracle(ctx, oracle, default_env, quirks):
    """(a) every stable case of one mode in one launch: iterations, trials, stop reason, flags exactly, pose, flows, chi2, lambda."""
    cs = FP.cases(stable=True, quirks=quirks)
    (res,) = _run(ctx, [c.build() for c in cs])
    for c, r in zip(cs, res):
        _check_case(c, r, oracle_run(oracle, c))


def test_register_store_has_the_bits_of_the_memory_store(ctx, default_env):
    """(b) the whole catalogue, the unstable trial-cap cases included: what a rejected and what an accepted trial do to the
    per-point state is the one thing the two stores do differently."""
    probs = [c.build() for c in FP.CASES]
    (reg,) = _run(ctx, probs)
    default_env.setenv("VDO_LM_GENERAL", "1")
    (gen,) = _run(ctx, probs)
    for c, r, g in zip(FP.CASES, reg, gen):
        _same_bits(r, g)


def test_one_workgroup_per_problem_on_the_rejection_cases(ctx, oracle, default_env):
    """(c) a budget of one workgroup per problem: 260, 520 and 2300 correspondences are strided over the 256 threads, and only a
    thread's first one takes the Schur sums' hand-over (F2Pre)."""
    cs = FP.cases(FP.REJECTION)
    assert {c.n for c in cs} == {260, 520, 2300}
    probs = [c.build() for c in cs]
    default_env.setenv("VDO_LM_CLUSTER_BUDGET", "1")
    (one,) = _run(ctx, probs)
    for c, r in zip(cs, one):
        _check_case(c, r, oracle_run(oracle, c))
    default_env.setenv("VDO_LM_GENERAL", "1")
    (gen,) = _run(ctx, probs)
    for r, g in zip(one, gen):
        _same_bits(r, g)


def test_trial_cap_cases_end_finite(ctx, oracle, default_env):
    """(d) ten trials in one iteration happen at the rounding floor only, so the trajectory is not the oracle's to the trial;
    the start is, and the end is an ordinary Levenberg stop with finite outputs."""
    cs = FP.cases(FP.TRIAL_CAP)
    (res,) = _run(ctx, [c.build() for c in cs])
    for c, r in zip(cs, res):
        st = oracle_run(oracle, c)[4]
        assert abs(r["initial_chi2"] - st.initial_chi2) <= 1e-10 * abs(st.initial_chi2)
        assert r["stop_reason"] in (1, 2)
        assert all(np.isfinite(r[k]).all() for k in ("T", "flow", "final_chi2", "final_lambda", "initial_chi2"))
        assert 0 <= r["n_inliers"] == int(r["inliers"].sum()) <= c.n


# ---------------------------------------------------------------------------------------------- reserved slots
CAPACITIES = [600, 600, 64, 8, 2300]


def _slot_problem(n, slot):
    """Catalogue cases where the size matches (rejection runs inside reused slots), the generator otherwise."""
    if n is None:
        return None
    if n == 260:
        return FP.BY_NAME["rej_q1_n260_s2_cam"].build()
    if n == 2300:
        return FP.BY_NAME["rej_q1_n2300_s0_cam"].build()
    return synth.make_flow2_problem(n, seed=60 + 7 * slot + n % 5, is_object=bool(slot & 1))


def _empty(like):
    return dataclasses.replace(like, obs=np.zeros((0, 2)), flow=np.zeros((0, 2)), depth=np.zeros(0))


FRAMES = [[600, 260, 64, 2, 2300], [3, 600, None, 8, 257], [None] * 5, [600, 260, 64, 2, 2300]]


def test_reserved_slots_reused_frame_after_frame(ctx, default_env):
    """(e) what the frame pipeline does: capacities fixed once, every slot redefined or emptied before each launch, outputs
    packed by the current sizes.  Every frame equals a fresh batch of the same problems, bit for bit."""
    from vdo_slam_amd.flow2 import Flow2Batch
    some = synth.make_flow2_problem(3, seed=1)
    b = Flow2Batch.reserve(ctx, CAPACITIES)
    seen = []
    for sizes in FRAMES:
        probs = [_slot_problem(n, k) for k, n in enumerate(sizes)]
        for k, p in enumerate(probs):
            b.set(k, p)
        b.run()
        got = b.fetch()
        (fresh,) = _run(ctx, [p if p is not None else _empty(some) for p in probs])
        for n, r, f in zip(sizes, got, fresh):
            _same_bits(r, f)
            assert r["flow"].shape == (n or 0, 2) and r["inliers"].shape == (n or 0,)
            if n is None or n < 3:      # nothing to optimise: identity, no inliers, flows as measured
                assert np.array_equal(r["T"], np.eye(4)) and r["n_inliers"] == 0 and not r["inliers"].any()
            else:
                assert r["iterations"] >= 1
        seen.append(got)
    for r1, r4 in zip(seen[0], seen[3]):
        _same_bits(r1, r4)
    assert seen[0][1]["trials"] > seen[0][1]["iterations"] + 1      # (rejection runs did happen in a reused slot)

    # refusals leave the batch as it was
    from vdo_slam_amd._capi import VDO_ERR_INVALID, VdoError
    with pytest.raises(VdoError) as e:
        b.set(0, synth.make_flow2_problem(CAPACITIES[0] + 1, seed=2))
    assert e.value.code == VDO_ERR_INVALID
    for k in (-1, len(CAPACITIES)):
        with pytest.raises(VdoError) as e:
            b.set(k, some)
        assert e.value.code == VDO_ERR_INVALID
    b.run()
    for r4, r5 in zip(seen[3], b.fetch()):
        _same_bits(r4, r5)
    b.close()
    plain = Flow2Batch(ctx, [some])
    with pytest.raises(VdoError) as e:
        plain.set(0, some)
    assert e.value.code == VDO_ERR_INVALID
    plain.close()
    with pytest.raises(VdoError) as e:
        Flow2Batch.reserve(ctx, [10, -1])
    assert e.value.code == VDO_ERR_INVALID
