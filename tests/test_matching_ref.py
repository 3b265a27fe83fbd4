"""CPU side of the descriptor matcher: the vectorised NumPy restatement of its contract (tests/matching_ref.py) against a literal
sequential scan, the host popcount of ORBmatcher::DescriptorDistance, and the new symbols of both libraries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import matching_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    dict(),
    dict(max_distance=3),
    dict(ratio=0.5),
    dict(ratio=0.9, max_distance=100),
    dict(window=16.0),
    dict(max_octave_diff=1),
    dict(window=24.0, max_octave_diff=0, cross_check=True),
    dict(cross_check=True),
    dict(window=8.0, max_octave_diff=1, ratio=0.8, max_distance=120, cross_check=True),
]


@pytest.mark.parametrize("prm", CASES, ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()) or "plain")
def test_restatement_equals_the_sequential_scan(prm):
    rng = np.random.default_rng(11)
    for nq, nt, make in [(0, 5, M.random_set), (5, 0, M.random_set), (1, 1, M.random_set), (7, 9, M.random_set), (9, 7, M.tied_set), (13, 12, M.tied_set)]:
        q, t = make(rng, nq), make(rng, nt)
        if nq and nt:
            q["x"][0] = np.nan                             # a NaN position is never a candidate
            t["desc"][-1] = q["desc"][0]
        got = M.match_ref(q, t, block=4, **prm)            # block 4: the query chunking is exercised
        want = M.match_loops(q, t, **prm)
        for g, w, name in zip(got, want, ("train_idx", "best_dist", "second_dist", "n_matches")):
            assert np.array_equal(g, w), (name, nq, nt)


def test_restatement_ties_second_and_cross_check():
    z = np.zeros(32, np.uint8)
    one = z.copy(); one[0] = 1
    # three equal train rows: lowest index, second == best
    q = {"desc": np.stack([z])}
    t = {"desc": np.stack([one, z, z, z])}
    idx, best, second, n = M.match_ref(q, t)
    assert (idx[0], best[0], second[0], n) == (1, 0, 0, 1)
    # a complement row: 256
    idx, best, second, n = M.match_ref(q, {"desc": np.stack([~z])})
    assert (idx[0], best[0], second[0], n) == (0, 256, -1, 1)
    # two queries share a best train row: the closer keeps it, at equal distance the lower query index
    q2 = {"desc": np.stack([one, z])}
    idx, best, _, n = M.match_ref(q2, {"desc": np.stack([z])}, cross_check=True)
    assert idx.tolist() == [-1, 0] and best.tolist() == [1, 0] and n == 1
    idx, best, _, n = M.match_ref({"desc": np.stack([z, z])}, {"desc": np.stack([z])}, cross_check=True)
    assert idx.tolist() == [0, -1] and best.tolist() == [0, 0] and n == 1


def test_host_descriptor_distance_equals_the_table_popcount():
    from vdo_slam_amd import _capi as K
    try:
        host = K.load_host_lib()
    except (OSError, RuntimeError) as e:
        pytest.skip(f"libvdo_host.so does not load here: {e}")
    host.host_descriptor_distance.argtypes = [K.c_uint8_p, K.c_uint8_p]
    host.host_descriptor_distance.restype = C.c_int
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    rows[0] = 0; rows[1] = 255
    for i in range(0, 40, 2):
        a, b = rows[i], rows[i + 1]
        want = int(M.POPCOUNT[a ^ b].sum())
        assert host.host_descriptor_distance(a.ctypes.data_as(K.c_uint8_p), b.ctypes.data_as(K.c_uint8_p)) == want
    assert host.host_descriptor_distance(rows[0].ctypes.data_as(K.c_uint8_p), rows[1].ctypes.data_as(K.c_uint8_p)) == 256


def test_matcher_symbols_are_declared_and_exported():
    from vdo_slam_amd import _capi as K
    hdr = open(os.path.join(ROOT, "include", "vdo_slam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = K.lib()
    for s in ("vdo_orb_match", "vdo_orb_match_extractors", "vdo_orb_last_keypoints"):
        assert re.search(r"\b%s\s*\(" % s, hdr), f"{s} is not declared in include/vdo_slam_hip.h"
        assert hasattr(L, s), f"{s} is not exported by libvdo_hip.so"
    for s in ("vdo_match_set", "vdo_match_params"):
        assert re.search(r"\}\s*%s\s*;" % s, hdr), f"struct {s} is not declared"
    from vdo_slam_amd import matching
    assert C.sizeof(matching.MatchParamsC) == 24 and matching.MatchSetC.is_device.offset == 40
    try:
        host = K.load_host_lib()
    except (OSError, RuntimeError) as e:
        pytest.skip(f"libvdo_host.so does not load here: {e}")
    for s in ("host_orb_match", "host_orb_match_extractors", "host_descriptor_distance"):
        assert hasattr(host, s), f"{s} is not exported by libvdo_host.so"


def test_matcher_refuses_bad_arguments_without_a_device():
    """Argument checks come before any device call: they are the same on a machine without a GPU."""
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd import matching
    L = matching._lib()
    L.vdo_last_error.restype = C.c_char_p
    p = matching.params()
    out = np.zeros(4, np.int32)
    op = out.ctypes.data_as(K.c_int32_p)
    m = C.c_int32()
    assert L.vdo_orb_match(None, None, None, C.byref(p), op, op, op, C.byref(m)) == K.VDO_ERR_INVALID
    assert b"ctx is null" in L.vdo_last_error()
    assert L.vdo_orb_match_extractors(None, None, C.byref(p), op, op, op, C.byref(m), 4) == K.VDO_ERR_INVALID
    assert b"query is null" in L.vdo_last_error()
