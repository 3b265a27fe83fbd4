"""csrc/ransac.hip (k_ap3p_hyp, k_p3p_hyp, k_ransac_vote, the host replay) on the catalogue of tests/pnp_envelope.py against the
oracle's sequential run: hypothesis counts around the 64-thread block, point counts around the ballot, the mask words and the
256-thread stride, per-problem cameras and thresholds, the clamps of the budget, non-finite and degenerate scenes - and one call
of 40 unlike problems, plain and gated, against each member run alone (pt_off, hyp_off, mask_off, the max_hyp-sized grid)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import pnp_envelope as PE
from tests.test_pnp_envelope import oracle_result
from vdo_slam_amd import _capi as K
from vdo_slam_amd.ransac import PnpProblemC, PnpResultC

pytestmark = pytest.mark.gpu

FIELDS = ("n_inliers", "iterations_run", "best_iteration")


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _same(a, b):
    return all(a[q] == b[q] for q in FIELDS) and a["T"].tobytes() == b["T"].tobytes() and np.array_equal(a["inliers"], b["inliers"])


def _check(case, g, e, refit=None):
    """The comparison of tests/test_ransac_gpu.py, plus - without the refit - the NumPy restatement of the vote on the product's result."""
    refit = case.refit if refit is None else refit
    assert tuple(g[q] for q in FIELDS) == tuple(e[q] for q in FIELDS), (case.name, [g[q] for q in FIELDS], [e[q] for q in FIELDS])
    assert np.array_equal(g["inliers"], e["inliers"]), case.name
    if not refit:
        assert np.array_equal(g["T"], e["T"]), (case.name, np.abs(g["T"] - e["T"]).max())
        assert PE.check_vote(case, g) <= 1
    elif e["n_inliers"] >= 12:
        assert np.abs(g["T"] - e["T"]).max() <= 1e-9 * max(1.0, np.abs(e["T"]).max()), (case.name, e["n_inliers"], np.abs(g["T"] - e["T"]).max())
    else:
        assert np.isfinite(g["T"]).all(), case.name


GROUPS = {"grid_ap3p": [c for c in PE.cases(PE.GRID, solver="ap3p") if c.refit == 0], "grid_ap3p_refit": PE.cases(PE.GRID, solver="ap3p", refit=1),
          "grid_grunert": PE.cases(PE.GRID, solver="grunert"), "camera2": PE.cases(PE.CAMERA2), "hostile": PE.cases(PE.HOSTILE)}
assert sum(len(v) for v in GROUPS.values()) == len(PE.CASES)


@pytest.mark.parametrize("group", list(GROUPS))
def test_catalogue_in_batches_of_eight(ctx, oracle, group):
    """(1) every case, 8 consecutive ones to a call: votes, hypotheses examined, winner and flags equal; the pose the same bits
    without the refit, to 1e-9 with it."""
    n_refit = 0
    for batch in PE.batches(GROUPS[group]):
        for c, g in zip(batch, PE.run_cases(ctx, batch)):
            e = oracle_result(oracle, c)
            _check(c, g, e)
            n_refit += bool(c.refit and e["n_inliers"] >= 12)
    if group in ("grid_ap3p_refit", "grid_grunert"):
        assert n_refit >= 50


@pytest.fixture(scope="module")
def mixed(ctx):
    """The call of 40, each member alone, and the call again with every member's refit bit on (computed once, never modified)."""
    return dict(batch=PE.run_cases(ctx, PE.MIXED), alone=[PE.run_cases(ctx, [c])[0] for c in PE.MIXED], on=PE.run_cases(ctx, PE.MIXED, flags=[1] * len(PE.MIXED)))


def test_forty_unlike_problems_in_one_call(oracle, mixed):
    """(2) every member bit-equal to the same problem run alone, and equal to the oracle."""
    for c, b, a in zip(PE.MIXED, mixed["batch"], mixed["alone"]):
        assert _same(b, a), (c.name, b, a)
        _check(c, b, oracle_result(oracle, c))
        if c.n < 4 or c.max_iterations == 0:
            assert (b["n_inliers"], b["iterations_run"], b["best_iteration"]) == (0, 0, -1) and np.array_equal(b["T"], np.eye(4)) and b["inliers"].shape == (c.n,)
    for c, r in zip(PE.MIXED, mixed["on"]):
        _check(c, r, oracle_result(oracle, dataclasses.replace(c, name=c.name + "_r1", refit=1)), refit=1)
    assert sum(r["best_iteration"] >= 0 and not np.array_equal(r["T"], b["T"]) for r, b in zip(mixed["on"], mixed["batch"])) >= 15      # on and off can be told apart


def test_forty_unlike_problems_gated(ctx, mixed):
    """(3) the gated call: a member whose vote exceeds its gate equals the refit-on result, any other the refit-off one."""
    votes = [r["n_inliers"] for r in mixed["batch"]]
    gates = np.array([(v - 1, v, v + 1, -1)[k % 4] for k, v in enumerate(votes)], np.int32)
    got = PE.run_cases(ctx, PE.MIXED, refit_above=gates, flags=[1] * len(PE.MIXED))
    n_on = n_off = 0
    for c, g, v, gate, on, off in zip(PE.MIXED, got, votes, gates, mixed["on"], mixed["batch"]):
        exp = on if v > gate else off
        assert _same(g, exp), (c.name, v, gate)
        if not _same(on, off):
            n_on += v > gate; n_off += not v > gate
    assert n_on >= 6 and n_off >= 6
    # the refit bit off: the gate has nothing to let through
    got = PE.run_cases(ctx, PE.MIXED, refit_above=np.full(len(PE.MIXED), -1, np.int32))
    assert all(_same(g, off) for g, off in zip(got, mixed["batch"]))


def test_subset_tables_are_kept_per_size_and_count(ctx, oracle):
    """(4) the draws are cached by (n, hypotheses): 65 hypotheses after 777 of the same size, another size, then 777 again."""
    by = {(c.n, c.max_iterations): c for c in PE.cases(PE.GRID, refit=0, solver="ap3p") if (c.thr, c.confidence) == (0.4, 1.0)}      # (confidence 1: every hypothesis is examined)
    order = [(65, 777), (65, 65), (129, 777), (65, 777), (64, 65), (65, 65)]
    seen = {}
    for key in order:
        g = PE.run_cases(ctx, [by[key]])[0]
        _check(by[key], g, oracle_result(oracle, by[key]))
        assert g["iterations_run"] == key[1]
        if key in seen:
            assert _same(g, seen[key])
        seen[key] = g
    assert seen[(65, 777)]["best_iteration"] >= 65          # (the longer table is not the shorter one)


def _problem(n, X, uv, max_iterations=500, flags=0):
    return PnpProblemC(n, K._dp(X) if X is not None else None, K._dp(uv) if uv is not None else None, (C.c_double * 4)(*PE.CAMERAS["kitti"]), max_iterations, 0.4, 0.98, flags)


def test_refusals(ctx, oracle):
    """(5) bad fields are refused, whatever their position in the call; the context works afterwards."""
    good = PE.BY_NAME["grid_n65_m500_t0.4_c0.98_ap3p_r0"]
    X, uv = good.build()
    L = K.lib()
    L.vdo_pnp_ransac_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PnpProblemC), C.POINTER(PnpResultC), C.POINTER(K.c_uint8_p)]
    bad = {"n = -1": _problem(-1, X, uv), "max_iterations = -1": _problem(65, X, uv, max_iterations=-1), "null X": _problem(65, None, uv),
           "null uv": _problem(65, X, None), "two solvers": _problem(65, X, uv, flags=2)}
    for what, p in bad.items():
        for first in (True, False):
            arr = (PnpProblemC * 2)(*((p, _problem(65, X, uv)) if first else (_problem(65, X, uv), p)))
            res = (PnpResultC * 2)()
            inl = [np.zeros(65, np.uint8) for _ in range(2)]
            ip = (K.c_uint8_p * 2)(*[a.ctypes.data_as(K.c_uint8_p) for a in inl])
            assert L.vdo_pnp_ransac_batch(ctx._h, 2, arr, res, ip) == K.VDO_ERR_INVALID, (what, first)
    _check(good, PE.run_cases(ctx, [good])[0], oracle_result(oracle, good))
