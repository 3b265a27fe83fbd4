"""The register-resident path of k_flow2_lm (one correspondence per thread: every problem of at most 2048 matches on a full
cluster) against the general path over the scratch arrays (VDO_LM_GENERAL=1), bit for bit, and both against the CPU oracle."""
import numpy as np
import pytest

from vdo_slam_amd import synth
from tests.test_flow2_gpu import _check
from tests.test_oracle_flow2 import run_oracle

pytestmark = pytest.mark.gpu

# 64/65 and 255/256/257: wave and workgroup edges of the neighbour's Hll diagonal (F3 aliasing); 257..513: ragged last chunk and
# idle threads on a cluster; 2048: the last size on the register path
SIZES = [3, 4, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 1200, 2047, 2048]
BIT_KEYS = ("T", "flow", "inliers", "n_inliers", "iterations", "trials", "final_chi2", "stop_reason", "final_lambda", "initial_chi2")


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _edge_problems(quirks):
    probs = []
    for k, n in enumerate(SIZES):
        if n == 3 and quirks == 0:
            continue      # rank-deficient with the intended step: rounding-sensitive trajectory (as in test_flow2_gpu.py)
        p = synth.make_flow2_problem(n, seed=100 + k, is_object=bool(k & 1))      # camera and object problems alternate
        p.ref_quirks = quirks
        probs.append(p)
    return probs


_oracle_cache = {}


def _edge_oracle(oracle, quirks):
    """Problems of the size sweep and what the oracle makes of them: computed once per mode, shared, never modified."""
    if quirks not in _oracle_cache:
        probs = _edge_problems(quirks)
        _oracle_cache[quirks] = (probs, [run_oracle(oracle, p) for p in probs])
    return _oracle_cache[quirks]


def _run(ctx, probs, runs=1):
    from vdo_slam_amd.flow2 import Flow2Batch
    b = Flow2Batch(ctx, probs)
    out = []
    for _ in range(runs):
        b.run()
        out.append(b.fetch())
    b.close()
    return out


def _same_bits(a, c):
    """Bit for bit: -0.0 is not 0.0.  A NaN equals a NaN at the same place - sign and payload of a NaN are no computed value (IEEE 754
    leaves them open, and they follow the operand order the compiler chose for each instantiation of the loop body)."""
    for key in BIT_KEYS:
        x, y = np.asarray(a[key]), np.asarray(c[key])
        assert x.dtype == y.dtype and x.shape == y.shape, key
        if x.dtype.kind == "f":
            nan = np.isnan(x)
            assert np.array_equal(nan, np.isnan(y)), key
            x, y = np.where(nan, 0.0, x), np.where(nan, 0.0, y)
        assert x.tobytes() == y.tobytes(), key


@pytest.mark.parametrize("quirks", [1, 0])
def test_register_path_has_the_bits_of_the_general_path(ctx, oracle, monkeypatch, quirks):
    probs, ref = _edge_oracle(oracle, quirks)
    monkeypatch.delenv("VDO_LM_GENERAL", raising=False)
    monkeypatch.delenv("VDO_LM_CLUSTER_BUDGET", raising=False)
    (reg,) = _run(ctx, probs)
    monkeypatch.setenv("VDO_LM_GENERAL", "1")
    (gen,) = _run(ctx, probs)
    for p, r, g, (T, flow, inl, ninl, st) in zip(probs, reg, gen, ref):
        _same_bits(r, g)
        _check(r, T, flow, inl, ninl, st)
        _check(g, T, flow, inl, ninl, st)


def test_size_sweep_exercises_rejected_trials(oracle):
    """A rejected trial keeps the current registers and re-uses them: the sweep above must contain such trials."""
    _, ref = _edge_oracle(oracle, 1)
    assert any(st.total_trials > st.iterations for (_, _, _, _, st) in ref)


def test_mixed_launch_selects_the_path_per_problem(ctx, oracle, monkeypatch):
    """2049 and 3001 matches take the general path, the others the register path, in one launch; a second run reproduces the first."""
    monkeypatch.delenv("VDO_LM_GENERAL", raising=False)
    monkeypatch.delenv("VDO_LM_CLUSTER_BUDGET", raising=False)
    probs = [synth.make_flow2_problem(n, seed=20 + k, is_object=True) for k, n in enumerate([800, 450, 150, 2, 60, 2049, 3001])]
    r1, r2 = _run(ctx, probs, runs=2)
    for p, a, c in zip(probs, r1, r2):
        T, flow, inl, ninl, st = run_oracle(oracle, p)
        if p.n < 3:
            assert a["n_inliers"] == 0 and np.array_equal(a["T"], np.eye(4))
            assert not a["inliers"].any()
        else:
            _check(a, T, flow, inl, ninl, st)
        _same_bits(a, c)


def test_lowered_cluster_falls_back_to_the_general_path(ctx, oracle, monkeypatch):
    """A budget of one cluster workgroup puts every problem on a single workgroup: 300 and 600 matches are then more than one per
    thread (general path), 200 stay on the register path.  (No bit comparison across cluster sizes: the summation order differs.)"""
    monkeypatch.delenv("VDO_LM_GENERAL", raising=False)
    monkeypatch.setenv("VDO_LM_CLUSTER_BUDGET", "1")
    probs = [synth.make_flow2_problem(n, seed=40 + k, is_object=bool(k & 1)) for k, n in enumerate([200, 300, 600])]
    (res,) = _run(ctx, probs)
    for p, r in zip(probs, res):
        T, flow, inl, ninl, st = run_oracle(oracle, p)
        _check(r, T, flow, inl, ninl, st)
