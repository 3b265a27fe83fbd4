"""vdo_pnp_ransac_batch_gated against the existing call, bit for bit: a problem whose vote exceeds its gate equals the call with the refit bit on, any other the
call with the bit off - T, n_inliers, iterations_run, best_iteration and the inlier flags.  Sizes: below / at the 4 points a hypothesis needs, around one wave of
the vote (64 / 65) and several; gates: -1 (always), one below / at / one above the vote, and none.  The hooks: host_work once, before the gate is read;
after_replay once, on the calling thread, with the final flags.  And vdo_flow2_batch_set_T0: a slot whose pose is rewritten runs as a slot set with it."""
import copy
import threading

import numpy as np
import pytest

from tests.test_oracle_p3p import _scene
from vdo_slam_amd import synth
from vdo_slam_amd.ba import Context
from vdo_slam_amd.flow2 import Flow2Batch
from vdo_slam_amd.ransac import pnp_ransac_batch, pnp_ransac_batch_gated
from vdo_slam_amd.synth import KITTI_K

pytestmark = pytest.mark.gpu

SIZES = (3, 4, 64, 65, 300)
FIELDS = ("n_inliers", "iterations_run", "best_iteration")


@pytest.fixture(scope="module")
def ctx():
    return Context(0)


@pytest.fixture(scope="module")
def reference(ctx):
    """Per size: the problem and what the existing call returns with the refit bit on and off (computed once, never modified)."""
    rng = np.random.default_rng(21)
    ref = {}
    for n in SIZES:
        Xw, uv, _, _, _ = _scene(rng, n, 0.25 if n >= 64 else 0.0, pix_sigma=0.1)
        on = pnp_ransac_batch(ctx, [(Xw, uv)], KITTI_K, refit=True)[0]
        off = pnp_ransac_batch(ctx, [(Xw, uv)], KITTI_K, refit=False)[0]
        ref[n] = ((Xw, uv), on, off)
    # a problem none of whose hypotheses is valid: every point the same
    Xd = np.tile([[1.0, 0.5, 9.0]], (64, 1)); ud = np.tile([[600.0, 180.0]], (64, 1))
    ref["degenerate"] = ((Xd, ud), pnp_ransac_batch(ctx, [(Xd, ud)], KITTI_K, refit=True)[0], pnp_ransac_batch(ctx, [(Xd, ud)], KITTI_K, refit=False)[0])
    return ref


def _same(a, b):
    return all(a[q] == b[q] for q in FIELDS) and np.array_equal(a["T"], b["T"]) and np.array_equal(a["inliers"], b["inliers"])


def test_the_reference_is_worth_comparing_against(reference):
    for n in (64, 65, 300):
        _, on, off = reference[n]
        assert on["n_inliers"] >= 0.5 * n and not np.array_equal(on["T"], off["T"])      # the refit moves the pose: on and off can be told apart
    assert reference[3][1]["best_iteration"] == -1 and reference["degenerate"][1]["best_iteration"] == -1
    assert reference[4][1]["n_inliers"] == 4


@pytest.mark.parametrize("gate", ["always", "below", "at", "above", "none"])
@pytest.mark.parametrize("n", SIZES)
def test_one_problem_against_the_existing_call(ctx, reference, n, gate):
    prob, on, off = reference[n]
    v = on["n_inliers"]
    g = {"always": -1, "below": v - 1, "at": v, "above": v + 1, "none": None}[gate]
    got = pnp_ransac_batch_gated(ctx, [prob], KITTI_K, refit_above=None if g is None else np.array([g], np.int32))[0]
    exp = on if g is None or v > g else off
    assert _same(got, exp), (n, gate, got, exp)


def test_a_batch_of_three_mixes_gates(ctx, reference):
    (p300, on300, off300), (pd, ond, offd), (p65, on65, off65) = reference[300], reference["degenerate"], reference[65]
    gates = np.array([on300["n_inliers"], -1, on65["n_inliers"] - 1], np.int32)          # not refitted | nothing to refit | refitted
    got = pnp_ransac_batch_gated(ctx, [p300, pd, p65], KITTI_K, refit_above=gates)
    assert _same(got[0], off300) and _same(got[1], ond) and _same(got[1], offd) and _same(got[2], on65)
    assert np.array_equal(got[1]["T"], np.eye(4)) and got[1]["n_inliers"] == 0
    # the refit bit off: the gate has nothing to let through
    got = pnp_ransac_batch_gated(ctx, [p300, pd, p65], KITTI_K, refit_above=np.full(3, -1, np.int32), refit=False)
    assert _same(got[0], off300) and _same(got[1], offd) and _same(got[2], off65)


def test_hooks_run_once_in_order_on_the_calling_thread(ctx, reference):
    (p300, on300, off300), (p64, on64, off64) = reference[300], reference[64]
    log = []
    gate = np.full(2, 10 ** 6, np.int32)                      # as it stands nothing would be refitted: host_work lowers it

    def host_work(g):
        assert g is gate
        log.append(("host_work", threading.get_ident()))
        g[0] = -1; g[1] = on64["n_inliers"]

    def after_replay(view):
        log.append(("after_replay", threading.get_ident()))
        seen.extend(view)
    seen = []
    got = pnp_ransac_batch_gated(ctx, [p300, p64], KITTI_K, refit_above=gate, host_work=host_work, after_replay=after_replay)
    assert [q for q, _ in log] == ["host_work", "after_replay"] and all(t == threading.get_ident() for _, t in log)
    assert _same(got[0], on300) and _same(got[1], off64)      # the gate was read after host_work had written it
    for s, g in zip(seen, got):                               # what after_replay saw is what the call returned
        assert all(s[q] == g[q] for q in FIELDS) and np.array_equal(s["inliers"], g["inliers"])
    # no valid hypothesis at all: both hooks still run, once
    log.clear(); seen.clear()
    gate[:] = 7
    got = pnp_ransac_batch_gated(ctx, [reference[3][0]], KITTI_K, refit_above=gate[:1].copy(), host_work=lambda g: log.append(("host_work", threading.get_ident())), after_replay=after_replay)
    assert [q for q, _ in log] == ["host_work", "after_replay"] and _same(got[0], reference[3][1]) and seen[0]["best_iteration"] == -1


def test_the_switch_restores_the_ungated_call(ctx, reference, monkeypatch):
    prob, on, off = reference[300]
    monkeypatch.setenv("VDO_PNP_NO_GATE", "1")                # read on every call
    order = []
    got = pnp_ransac_batch_gated(ctx, [prob], KITTI_K, refit_above=np.array([10 ** 6], np.int32), after_replay=lambda v: order.append(v[0]["n_inliers"]))[0]
    assert _same(got, on) and order == [on["n_inliers"]]
    monkeypatch.delenv("VDO_PNP_NO_GATE")
    assert _same(pnp_ransac_batch_gated(ctx, [prob], KITTI_K, refit_above=np.array([10 ** 6], np.int32))[0], off)


def test_set_T0_equals_a_slot_set_with_that_pose(ctx):
    probs = [synth.make_flow2_problem(300, seed=4), synth.make_flow2_problem(130, seed=5, is_object=True)]
    other = []
    for p in probs:                                           # the same problems with another initial pose
        q = copy.copy(p)
        q.T0 = p.T0.copy(); q.T0[:3, 3] += [0.05, -0.02, 0.1]
        other.append(q)
    a = Flow2Batch.reserve(ctx, [512, 512, 64])
    b = Flow2Batch.reserve(ctx, [512, 512, 64])
    for k in range(2):
        a.set(k, probs[k]); b.set(k, other[k])
    a.set_T0(0, probs[0].T0); b.set_T0(0, probs[0].T0)        # (rewritten with its own pose: nothing changes; with the first batch's: now equal)
    a.set_T0(1, other[1].T0)                                  # slot 1 the other way round
    a.run(); b.run()
    ra, rb = a.fetch(), b.fetch()
    for k in range(2):
        assert ra[k]["iterations"] >= 1 and ra[k]["n_inliers"] > 50
        for q in ra[k]:
            assert np.array_equal(np.asarray(ra[k][q]), np.asarray(rb[k][q])), (k, q)
    # ... and the pose matters: slot 1 started elsewhere than its own T0 would have taken it
    c = Flow2Batch.reserve(ctx, [512, 512, 64])
    c.set(1, probs[1]); c.run()
    assert not np.array_equal(c.fetch()[1]["T"], ra[1]["T"])
    with pytest.raises(Exception):
        a.set_T0(3, probs[0].T0)
