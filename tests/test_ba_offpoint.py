"""The graphs of tests/ba_offpoint.py hit what they claim - shown with NumPy and the CPU oracle alone (no GPU): which branch of toCompactQuaternion every
residual rotation takes and by what margin, which side of its Huber width every edge lies on, and that the first Levenberg step of the unit-ball graph asks
for an increment with |q| > 1 and is accepted.  Inside the margins a last-bit difference between two implementations could choose the other branch or the
other sign of q: a discontinuity of g2o's, not an error of either."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import ba_offpoint as O
from vdo_slam_amd import _capi as K
from vdo_slam_amd import synth


def _linearize(oracle, g):
    gc, keep = K.graph_to_c(g)
    R = K.BASystem(g)
    assert oracle.vdo_oracle_ba_linearize(C.byref(gc), C.byref(R.c)) == 0
    return R


def _optimize(oracle, g, iters):
    gc, keep = K.graph_to_c(g)
    opt = K.LMOptionsC(iters, 1e-4, 0, 0, 0.0, 0)
    st = K.LMStatsC()
    pose = np.zeros_like(g.pose); point = np.zeros_like(g.point)
    assert oracle.vdo_oracle_ba_optimize(C.byref(gc), C.byref(opt), K._dp(pose), K._dp(point), C.byref(st)) == 0
    return st, pose, point


def test_numpy_chi2_is_the_oracles(oracle):
    """the NumPy restatement of the four edge classes (what the width sets and the branch shares are computed from) sums to the oracle's chi2"""
    g = O.posepose_graph()
    graphs = [dataclasses.replace(g, pose=pose) for _, pose in O.posepose_cases(g)[::5]] + list(O.huber_graphs().values())
    for gg in graphs:
        total = sum(v.sum() for v in O.edge_chi2(gg).values())
        assert abs(total - _linearize(oracle, gg).chi2) <= 1e-12 * total


def test_posepose_cases_reach_every_branch_inside_the_margins(oracle):
    g = O.posepose_graph()
    for info in list(g.ep_info) + list(g.pr_info):
        M = info.reshape(6, 6)
        assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() > 0 and np.linalg.cond(M) <= 1e3
        assert np.unique(M[np.triu_indices(6)]).size == 21 and np.abs(M[~np.eye(6, dtype=bool)]).min() > 0
    pairs = list(zip(g.ep_i.tolist(), g.ep_j.tolist()))
    assert all(p in pairs for p in [(f, f + 1) for f in range(6)] + [(4, 2)]) and pairs.count((1, 2)) == 2 and (g.ep_i >= g.n_cam).sum() >= 2
    assert g.pr_pose.tolist() == [0, 5]
    cases = O.posepose_cases(g)
    assert len(cases) == len(O.rotation_table()) == 28 and all(name in dict(cases) for name in O.LM_CASES)
    seen = {"edge": set(), "prior": set()}
    d2 = O.dsqr(g.huber_ep)
    for name, pose in cases:
        Ee, Ep = O.posepose_E(g, pose)
        for kind, Es in (("edge", Ee), ("prior", Ep)):
            for E in Es:
                cls, tr, qw, gap = O.classify_rotation(synth.iso_R(E))
                assert abs(tr) >= 1e-3 and abs(qw) >= 1e-4, (name, kind, cls, tr, qw)
                if tr < 0:                                        # (the diagonal entries are compared on this branch alone)
                    assert gap >= 1e-7, (name, kind, cls, gap)
                    if gap < O.NEAR_TIE:
                        seen[kind].add("near_tie")
                seen[kind].add(cls)
        chi = O.edge_chi2(g, pose)["ep"]
        assert (chi <= d2).any() and (chi > d2).any(), name      # both branches of the pose-pose Huber kernel in every case
        assert np.abs(chi / d2 - 1).min() > 1e-9
        R = _linearize(oracle, dataclasses.replace(g, pose=pose))
        assert np.isfinite(R.chi2) and all(np.isfinite(getattr(R, b)).all() for b in ("Hpp", "bp", "Hpp_ep"))
    for kind in ("edge", "prior"):
        assert seen[kind] >= set(O.ROTATION_CLASSES) | {"near_tie"}, (kind, seen[kind])


def test_asymmetric_information_is_not_symmetric_and_the_oracle_takes_it(oracle):
    g0 = O.posepose_graph()
    g = O.with_asymmetric_information(g0)
    for a, s in zip(list(g.ep_info) + list(g.pr_info), list(g0.ep_info) + list(g0.pr_info)):
        M = a.reshape(6, 6)
        assert np.abs(M - M.T)[~np.eye(6, dtype=bool)].min() > 1e-2 * np.abs(M).max()           # every off-diagonal pair differs
        assert np.allclose(0.5 * (M + M.T), s.reshape(6, 6), rtol=1e-13, atol=0)                  # its symmetric part is the positive definite matrix it came from
    cases = dict(O.posepose_cases(g))
    for name in O.LM_CASES:
        R = _linearize(oracle, dataclasses.replace(g, pose=cases[name]))
        S = _linearize(oracle, dataclasses.replace(g0, pose=cases[name]))
        assert abs(R.chi2 - S.chi2) <= 1e-12 * S.chi2                                            # (the skew part drops out of e^T Omega e ...)
        assert np.abs(R.bp - S.bp).max() > 1e-3 * np.abs(S.bp).max()                             # (... and not out of J^T Omega e)
        assert np.abs(R.Hpp_ep - S.Hpp_ep).max() > 1e-3 * np.abs(S.Hpp_ep).max()


def test_half_turn_graph_is_exact():
    """the exempt cases: qw == 0 exactly, and on the permutation-like half-turns the two largest diagonal entries are exactly tied"""
    g, poses = O.half_turn_graph()
    tied = 0
    for pose in poses:
        Ee, Ep = O.posepose_E(g, pose)
        for E in (Ee[0], Ep[0]):
            assert np.array_equal(E[:9], pose[1, :9])
            cls, tr, qw, gap = O.classify_rotation(synth.iso_R(E))
            assert tr == -1.0 and qw == 0.0 and gap in (0.0, 2.0)
            tied += gap == 0.0
    assert tied == 6


@pytest.mark.parametrize("which", ["compact", "general", "hub"])
def test_median_widths_split_every_class(which):
    g = O.huber_graphs()[which]
    m = O.median_widths(g)
    chi = O.edge_chi2(g)
    assert chi["ep"].size and chi["eb"].size and (chi["et"].size or which == "hub")
    for k in O.HUBER_CLASSES:
        if not chi[k].size:
            continue
        d2 = O.dsqr(m[k])
        assert d2 >= 1.1754943508222875e-38
        share = float((chi[k] <= d2).mean())
        assert 0.3 <= share <= 0.7, (k, share)
        assert np.abs(chi[k] / d2 - 1).min() >= 1e-9, k
    sets = O.huber_sets(g)
    assert len(sets) == 6 and len({w for w in sets.values()}) == 6
    for a in range(3):                                              # every class is once at its median, once without kernel, once at 1e-4
        assert sorted(w[a] for n, w in sets.items() if n.startswith("median_")) == sorted([0.0, 1e-4, list(m.values())[a]])
    if which == "hub":
        from tests import ba_envelope_graphs as E
        per_point = np.bincount(g.eb_point, minlength=g.n_point)
        assert per_point.max() > E.STATIC_SLOTS                      # a hub landmark: k_hub_sweep is on the path


@pytest.mark.parametrize("with_edges", [False, True])
def test_unit_ball_graph_leaves_the_ball_and_is_accepted(oracle, with_edges):
    g = O.unit_ball_graph(with_edges)
    R = _linearize(oracle, g)
    lam = 1e-5 * R.Hpp.reshape(-1, 6, 6)[:, np.arange(6), np.arange(6)].max()
    gc, keep = K.graph_to_c(g)
    x = np.zeros(18)
    assert oracle.vdo_oracle_ba_solve(C.byref(gc), C.c_double(lam), K._dp(x)) == 0
    q = np.linalg.norm(x.reshape(3, 6)[:, 3:], axis=1)
    assert q[1] > 1.1 and q[0] < 0.9 and q[2] < 0.9, q
    st, pose, _ = _optimize(oracle, g, 1)
    assert (st.iterations, st.total_trials) == (1, 1) and st.final_chi2 < st.initial_chi2      # the first trial is accepted
    assert np.array_equal(pose[1, :9], g.pose[1, :9]) and np.abs(pose[1, 9:] - g.pose[1, 9:]).min() > 0.1
    assert not np.array_equal(pose[2, :9], g.pose[2, :9])


def test_one_iteration_lm_runs_on_the_large_rotation_cases(oracle):
    g = O.posepose_graph()
    cases = dict(O.posepose_cases(g))
    for name in O.LM_CASES:
        st, pose, point = _optimize(oracle, dataclasses.replace(g, pose=cases[name]), 1)
        assert st.iterations == 1 and st.total_trials >= 1 and np.isfinite(st.final_chi2) and np.isfinite(pose).all() and np.isfinite(point).all()
