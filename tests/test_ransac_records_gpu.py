"""The compact read-back of the PnP RANSAC (k_ransac_records, csrc/ransac.hip): the host replay reads the record-setting hypotheses the
kernel wrote to mapped memory instead of the votes, poses and masks of all of them.  Problems at the mask-word and 64-lane padding
boundaries (4 .. 129 points), with exact inliers (one record, a budget that collapses at once) and with 60 % outliers (several
records), with 1 and 500 hypotheses, collinear points (no record at all), a batch with members of 0 - 3 points in its middle, and the
gated entry point.  Every result field, the pose bit for bit and the inlier flags equal the same call under VDO_PNP_FULL_READBACK=1
and the oracle's sequential RANSAC; the same again with VDO_PNP_RECORD_CAP=2, where a problem with more than two records takes the
overflow path (the full read-back behind the records)."""
import dataclasses
import functools

import numpy as np
import pytest

from tests import pnp_envelope as PE
from vdo_slam_amd.synth import KITTI_K, rotvec_to_R

pytestmark = pytest.mark.gpu

SIZES = (4, 5, 31, 32, 33, 63, 64, 65, 129)
FIELDS = ("n_inliers", "iterations_run", "best_iteration")


@functools.lru_cache(maxsize=None)
def _scene(n, kind):
    """kind "exact": every correspondence is the exact projection; "outliers": 60 % of them are moved by up to 60 px and the others carry 0.2 px of
    noise, so that the hypotheses drawn from inliers differ in their votes and one run sets several records."""
    fx, fy, cx, cy = KITTI_K
    rng = np.random.default_rng([n, 0 if kind == "exact" else 1])
    R = rotvec_to_R(rng.normal(0, 0.2, 3)); t = rng.normal(0, 1.0, 3)
    Xc = np.c_[rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)]
    X = (Xc - t) @ R
    uv = np.c_[fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy]
    if kind == "outliers":
        uv += rng.normal(0, 0.2, (n, 2))
        out = rng.random(n) < 0.6
        uv[out] += rng.uniform(-60, 60, (int(out.sum()), 2))
    X, uv = np.ascontiguousarray(X), np.ascontiguousarray(uv)
    X.setflags(write=False); uv.setflags(write=False)
    return X, uv


@dataclasses.dataclass(frozen=True)
class Case:                     # (the fields tests/pnp_envelope.run_cases and oracle_run read)
    n: int
    kind: str
    max_iterations: int
    refit: int = 0
    thr: float = 0.4
    confidence: float = 0.98
    K = tuple(KITTI_K)

    @property
    def flags(self):
        return int(self.refit)

    def build(self):
        if self.kind == "collinear":
            s = PE.scene(self.n, "kitti", "collinear")
            return s["X"], s["uv"]
        if self.n == 0:
            return np.zeros((0, 3)), np.zeros((0, 2))
        return _scene(self.n, self.kind)


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


_oracle_cache = {}


def oracle_of(oracle, c):
    if c not in _oracle_cache:
        _oracle_cache[c] = PE.oracle_run(oracle, c)
    return _oracle_cache[c]


def record_chain(oracle, c):
    """The hypotheses that set a record in front of the winner, from the oracle: the winner of the first m hypotheses is the last record among
    them (the budget, which let the full run reach its winner, ends no shorter run sooner), so m = the winner walks the records backwards."""
    chain, m = [], c.max_iterations
    while True:
        b = oracle_of(oracle, dataclasses.replace(c, max_iterations=m, refit=0))["best_iteration"]
        if b < 0:
            return chain[::-1]
        chain.append(b); m = b


def run(monkeypatch, ctx, cs, mode, refit_above=None):
    """One call on the cases ``cs`` in one of the three read-back modes."""
    monkeypatch.delenv("VDO_PNP_FULL_READBACK", raising=False); monkeypatch.delenv("VDO_PNP_RECORD_CAP", raising=False)
    if mode == "full":
        monkeypatch.setenv("VDO_PNP_FULL_READBACK", "1")
    elif mode == "cap2":
        monkeypatch.setenv("VDO_PNP_RECORD_CAP", "2")
    else:
        assert mode == "records"
    return PE.run_cases(ctx, cs, refit_above)


def assert_equal(got, want, what, pose_bits=True):
    for f in FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert np.array_equal(got["inliers"], want["inliers"]), what
    if pose_bits:
        assert np.array_equal(got["T"].view(np.uint64), want["T"].view(np.uint64)), (what, np.abs(got["T"] - want["T"]).max())


def check_all_modes(monkeypatch, ctx, oracle, cs, what, refit_above=None):
    """records == full == cap2, field by field and bit by bit; the oracle's consensus, and its pose bits where no EPnP refit ran."""
    full = run(monkeypatch, ctx, cs, "full", refit_above)
    for mode in ("records", "cap2"):
        got = run(monkeypatch, ctx, cs, mode, refit_above)
        for c, g, f in zip(cs, got, full):
            assert_equal(g, f, (what, mode, c))
    for k, (c, f) in enumerate(zip(cs, full)):
        refitted = c.refit and (refit_above is None or f["n_inliers"] > refit_above[k])
        want = oracle_of(oracle, c if refitted or not c.refit else dataclasses.replace(c, refit=0))      # (gated out: the winning hypothesis itself)
        assert_equal(f, want, (what, "oracle", c), pose_bits=not refitted)
    return full


@pytest.mark.parametrize("max_iterations", [1, 500])
@pytest.mark.parametrize("kind", ["exact", "outliers"])
def test_single_problems_at_the_mask_boundaries(monkeypatch, ctx, oracle, kind, max_iterations):
    for n in SIZES:
        for refit in (0, 1):
            c = Case(n, kind, max_iterations, refit)
            r = check_all_modes(monkeypatch, ctx, oracle, [c], "single")[0]
            if kind == "exact" and r["best_iteration"] >= 0:
                # every point is an inlier of the first valid hypothesis: the budget falls to 0 there and the loop ends behind it
                assert r["n_inliers"] == n and r["iterations_run"] == r["best_iteration"] + 1
            if max_iterations == 1:
                assert r["iterations_run"] == 1 and r["best_iteration"] in (-1, 0)
    if kind == "outliers" and max_iterations == 500:
        # the data has problems with several records, and some with more than two: VDO_PNP_RECORD_CAP=2 did take the overflow path
        chains = [record_chain(oracle, Case(n, kind, 500)) for n in SIZES]
        assert max(len(ch) for ch in chains) >= 3 and sum(len(ch) >= 2 for ch in chains) >= 3, chains
    if kind == "exact":
        assert all(len(record_chain(oracle, Case(n, kind, max_iterations))) <= 1 for n in SIZES)


def test_collinear_points_set_no_record(monkeypatch, ctx, oracle):
    for n in (65, 257):
        c = Case(n, "collinear", 500)
        r = check_all_modes(monkeypatch, ctx, oracle, [c], "collinear")[0]
        assert (r["n_inliers"], r["best_iteration"], r["iterations_run"]) == (0, -1, 500)
        assert np.array_equal(r["T"], np.eye(4)) and not r["inliers"].any()


def _batch():
    cs = [Case(n, ("exact", "outliers")[k & 1], (500, 500, 1)[k % 3], refit=1) for k, n in enumerate(SIZES)]
    cs[4:4] = [Case(0, "exact", 500, 1), Case(3, "exact", 500, 1), Case(1, "outliers", 500, 1), Case(2, "outliers", 1, 1)]      # members without hypotheses, in the middle
    cs.append(Case(65, "collinear", 500, 1))
    return cs


def test_a_batch_with_empty_members_in_the_middle(monkeypatch, ctx, oracle):
    cs = _batch()
    full = check_all_modes(monkeypatch, ctx, oracle, cs, "batch")
    for c, r in zip(cs, full):
        if c.n < 4:
            assert (r["n_inliers"], r["best_iteration"], r["iterations_run"]) == (0, -1, 0) and np.array_equal(r["T"], np.eye(4))


def test_the_gated_entry_point_with_one_refit_suppressed(monkeypatch, ctx, oracle):
    cs = _batch()
    votes = [r["n_inliers"] for r in run(monkeypatch, ctx, cs, "full")]
    k = max(range(len(cs)), key=lambda i: votes[i])
    assert votes[k] >= 4
    gate = np.zeros(len(cs), np.int32)
    gate[k] = votes[k]                       # "re-estimate only above this vote": the best member keeps its winning hypothesis
    full = check_all_modes(monkeypatch, ctx, oracle, cs, "gated", gate)
    assert np.array_equal(full[k]["T"], oracle_of(oracle, dataclasses.replace(cs[k], refit=0))["T"])
