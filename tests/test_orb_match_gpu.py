"""GPU: the device descriptor matcher (vdo_orb_match / vdo_orb_match_extractors, csrc/orb_match.hip) against the NumPy restatement of
its contract (tests/matching_ref.py).  Integer results throughout: every comparison is array_equal."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import matching_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("train_idx", "best_dist", "second_dist", "n_matches")


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), f"{what}: {name}"


def _match(ctx, q, t, **prm):
    from vdo_slam_amd import matching
    return matching.match(ctx, q, t, **prm)


# ---- sizes x chunking ----------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)
PAIRS = [(0, 0), (0, 513), (513, 0), (1, 513), (513, 1), (2, 257), (257, 2)] + [(n, n) for n in SIZES[1:]] + [(65, 255), (256, 63)]
GATED = dict(window=16.0, max_octave_diff=1, max_distance=100, cross_check=True)
PLAIN = dict()


@functools.lru_cache(maxsize=None)
def _sets_and_refs(nq, nt):
    """Seeded sets of one size pair and the restatement's answers for both configurations: computed once, shared by every chunking."""
    rng = np.random.default_rng(1000 * nq + nt)
    # half the rows come from a small pool with a few flipped bits: equal rows and equal distances across tile and chunk edges
    def make(n):
        s = M.random_set(rng, n)
        if n >= 2:
            s["desc"][::2] = M.tied_set(rng, n, pool=max(2, n // 16), flips=3)["desc"][::2]
        return s
    q, t = make(nq), make(nt)
    return q, t, M.match_ref(q, t, **GATED), M.match_ref(q, t, **PLAIN), M.match_ref(q, t, ratio=0.8, max_distance=90)


@pytest.mark.parametrize("chunk_rows", [0, 1, 64, 256, 257])
@pytest.mark.parametrize("nq,nt", PAIRS)
def test_sizes_and_chunking(ctx, nq, nt, chunk_rows):
    q, t, want_gated, want_plain, want_ratio = _sets_and_refs(nq, nt)
    _same(_match(ctx, q, t, chunk_rows=chunk_rows, **GATED), want_gated, "gates + cross-check")
    _same(_match(ctx, q, t, chunk_rows=chunk_rows, **PLAIN), want_plain, "no gate")
    _same(_match(ctx, q, t, chunk_rows=chunk_rows, ratio=0.8, max_distance=90), want_ratio, "ratio + distance")
    # sets without positions / octaves are all the ungated form needs
    _same(_match(ctx, {"desc": q["desc"]}, {"desc": t["desc"]}, chunk_rows=chunk_rows), want_plain, "descriptors only")


# ---- ties ------------------------------------------------------------------------------------------------------------------------
def _bits(k):
    """A 32-byte row with exactly the k lowest bits set."""
    r = np.zeros(32, np.uint8)
    r[:k // 8] = 255
    if k % 8:
        r[k // 8] = (1 << (k % 8)) - 1
    return r


@pytest.mark.parametrize("chunk_rows", [0, 256, 300, 7])
@pytest.mark.parametrize("at", [(255, 256), (299, 300), (100, 255, 256), (3, 511)])
def test_ties_keep_the_lowest_index(ctx, at, chunk_rows):
    rng = np.random.default_rng(3)
    t = {"desc": rng.integers(0, 256, (513, 32), dtype=np.uint8)}
    q = {"desc": rng.integers(0, 256, (3, 32), dtype=np.uint8)}
    near = q["desc"][1].copy(); near[5] ^= 0x11                          # distance 2 from query 1: closer than any random row
    for j in at:
        t["desc"][j] = near
    got = _match(ctx, q, t, chunk_rows=chunk_rows)
    _same(got, M.match_ref(q, t), "ties")
    assert got[0][1] == at[0] and got[1][1] == 2 and got[2][1] == 2      # lowest index; second == best


def test_complement_row_is_256(ctx):
    q = {"desc": np.stack([_bits(0), _bits(77)])}
    t = {"desc": np.stack([~_bits(0), ~_bits(77)])}
    idx, best, second, n = _match(ctx, q, t)
    assert idx.tolist() == [1, 0] and best.tolist() == [256 - 77, 256 - 77] and second.tolist() == [256, 256] and n == 2
    idx, best, second, n = _match(ctx, {"desc": q["desc"][:1]}, {"desc": t["desc"][:1]})
    assert (idx[0], best[0], second[0], n) == (0, 256, -1, 1)
    idx, best, second, n = _match(ctx, {"desc": q["desc"][:1]}, {"desc": t["desc"][:1]}, max_distance=255)
    assert (idx[0], best[0], second[0], n) == (-1, 256, -1, 0)


# ---- controlled popcounts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 50, 255, 256])
def test_max_distance_accepts_at_k_and_rejects_below(ctx, k):
    q = {"desc": np.stack([_bits(0)])}
    t = {"desc": np.stack([_bits(min(k + 9, 256)), _bits(k)])}
    idx, best, _, n = _match(ctx, q, t, max_distance=k)
    assert (idx[0], best[0], n) == (1 if k < 256 else 0, k, 1)
    if k:
        idx, best, _, n = _match(ctx, q, t, max_distance=k - 1)
        assert (idx[0], best[0], n) == (-1, k, 0)


def test_ratio_is_strict_and_needs_a_second(ctx):
    q = {"desc": np.stack([_bits(0)])}
    for second_bits, accepted in ((40, False), (41, True)):              # 20 < 0.5 * 40 is false (strict), 20 < 0.5 * 41 holds
        t = {"desc": np.stack([_bits(second_bits), _bits(20), _bits(200)])}
        idx, best, second, n = _match(ctx, q, t, ratio=0.5)
        assert (best[0], second[0]) == (20, second_bits)
        assert (idx[0], n) == ((1, 1) if accepted else (-1, 0))
        _same((idx, best, second, n), M.match_ref(q, t, ratio=0.5), "ratio")
    # a single candidate: no ratio test, second_dist == -1
    idx, best, second, n = _match(ctx, q, {"desc": np.stack([_bits(20)])}, ratio=0.5)
    assert (idx[0], best[0], second[0], n) == (0, 20, -1, 1)
    # ratio outside (0, 1): off
    for r in (0.0, 1.0, 1.5, -0.5):
        idx, _, _, n = _match(ctx, q, {"desc": np.stack([_bits(40), _bits(20)])}, ratio=r)
        assert (idx[0], n) == (1, 1)


# ---- gates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0.0, 0.0), (100.25, 50.5)])
def test_window_gate_at_the_limit_and_one_ulp_beyond(ctx, origin):
    w = np.float32(16.0)
    beyond = np.nextafter(w, np.float32(np.inf))
    ox, oy = np.float32(origin[0]), np.float32(origin[1])
    # offsets from the query; only the origin (0, 0) keeps `beyond` exact after the addition, so one ulp beyond is tested there
    offs = [(w, 0), (0, w), (-w, 0), (0, -w), (w, w)]
    if origin == (0.0, 0.0):
        offs += [(beyond, 0), (0, beyond), (-beyond, 0), (0, -beyond), (w, beyond)]
    n_in = 5
    tx = np.array([ox + np.float32(a) for a, _ in offs], np.float32); ty = np.array([oy + np.float32(b) for _, b in offs], np.float32)
    # rows beyond the window equal the query (distance 0); rows inside have 10 + index bits set: the gate decides, not the distance
    desc = np.stack([_bits(10 + i) if i < n_in else _bits(0) for i in range(len(offs))])
    q = {"desc": np.stack([_bits(0)]), "x": np.array([ox]), "y": np.array([oy]), "octave": np.zeros(1, np.int32)}
    t = {"desc": desc, "x": tx, "y": ty, "octave": np.zeros(len(offs), np.int32)}
    got = _match(ctx, q, t, window=float(w))
    _same(got, M.match_ref(q, t, window=float(w)), "window")
    assert (got[0][0], got[1][0], got[2][0]) == (0, 10, 11)
    if origin == (0.0, 0.0):
        # with only the rows beyond the window: no candidate at all
        t2 = {k: v[n_in:] for k, v in t.items()}
        got = _match(ctx, q, t2, window=float(w))
        assert (got[0][0], got[1][0], got[2][0], got[3]) == (-1, -1, -1, 0)
        got = _match(ctx, q, t2)                                          # gate off: they are the best
        assert (got[0][0], got[1][0], got[2][0], got[3]) == (0, 0, 0, 1)


def test_octave_gate_nan_positions_and_gated_out_queries(ctx):
    z = _bits(0)
    q = {"desc": np.stack([z, z, z]), "x": np.array([0, 0, np.nan], np.float32), "y": np.zeros(3, np.float32), "octave": np.array([2, 7, 2], np.int32)}
    t = {"desc": np.stack([_bits(3), _bits(2), _bits(1), _bits(0), _bits(5)]), "x": np.array([0, 0, 0, np.nan, 0], np.float32),
         "y": np.zeros(5, np.float32), "octave": np.array([3, 4, 0, 2, 1], np.int32)}
    # octave difference at the limit (1) and one past it (2); query 1 (octave 7) has every row gated out
    got = _match(ctx, q, t, max_octave_diff=1)
    _same(got, M.match_ref(q, t, max_octave_diff=1), "octave")
    assert got[0].tolist() == [3, -1, 3] and got[1].tolist() == [0, -1, 0] and got[2].tolist() == [3, -1, 3] and got[3] == 2
    got = _match(ctx, q, t, max_octave_diff=2)
    assert got[0].tolist() == [3, -1, 3] and got[2].tolist() == [1, -1, 1]
    # window on: the NaN train row and the NaN query are never candidates
    got = _match(ctx, q, t, window=1.0, max_octave_diff=1)
    _same(got, M.match_ref(q, t, window=1.0, max_octave_diff=1), "NaN")
    assert got[0].tolist() == [0, -1, -1] and got[1].tolist() == [3, -1, -1] and got[2].tolist() == [5, -1, -1]
    got = _match(ctx, q, t, window=1.0, max_octave_diff=1, cross_check=True)
    _same(got, M.match_ref(q, t, window=1.0, max_octave_diff=1, cross_check=True), "NaN + cross-check")
    # extreme octaves do not wrap
    q2 = dict(q, octave=np.array([2**31 - 1, -2**31, 0], np.int32)); t2 = dict(t, octave=np.array([-2**31, 2**31 - 1, 0, 1, -1], np.int32))
    _same(_match(ctx, q2, t2, max_octave_diff=1), M.match_ref(q2, t2, max_octave_diff=1), "octave extremes")


# ---- cross-check -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [0, 1])
def test_cross_check_keeps_the_closer_then_the_lower_query(ctx, chunk_rows):
    t = {"desc": np.stack([_bits(0), ~_bits(0)])}
    # queries 0 and 1 both have train 0 as their best; 1 is closer
    got = _match(ctx, {"desc": np.stack([_bits(4), _bits(1)])}, t, cross_check=True, chunk_rows=chunk_rows)
    assert got[0].tolist() == [-1, 0] and got[1].tolist() == [4, 1] and got[2].tolist() == [252, 255] and got[3] == 1
    # at equal distance the lower query index keeps it; the other reports its best_dist all the same
    got = _match(ctx, {"desc": np.stack([_bits(4), _bits(4), _bits(9)])}, t, cross_check=True, chunk_rows=chunk_rows)
    assert got[0].tolist() == [0, -1, -1] and got[1].tolist() == [4, 4, 9] and got[3] == 1
    # the cross-check ignores the distance filter: query 0 owns train 0 although max_distance rejects it, query 1 does not inherit it
    got = _match(ctx, {"desc": np.stack([_bits(4), _bits(4)])}, t, cross_check=True, max_distance=3, chunk_rows=chunk_rows)
    assert got[0].tolist() == [-1, -1] and got[3] == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _raw_call(ctx, q, t, prm, null=None):
    """vdo_orb_match through ctypes with sentinel-filled outputs: (rc, message, outputs untouched?)."""
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd import matching
    L = matching._lib()
    L.vdo_last_error.restype = C.c_char_p
    out = [np.full(8, -7, np.int32) for _ in range(3)]
    m = C.c_int32(-7)
    ptr = [o.ctypes.data_as(K.c_int32_p) for o in out] + [C.byref(m)]
    if null is not None:
        ptr[null] = None
    rc = L.vdo_orb_match(ctx._h, C.byref(q) if q is not None else None, C.byref(t) if t is not None else None,
                         C.byref(prm) if prm is not None else None, *ptr)
    return rc, (L.vdo_last_error() or b"").decode(), all((o == -7).all() for o in out) and m.value == -7


def test_refusals_name_the_argument_and_leave_the_context_usable(ctx):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd import matching
    rng = np.random.default_rng(9)
    full = M.random_set(rng, 5)
    bare = {"desc": full["desc"]}
    P = matching.params

    def sets(a, b):
        (sa, ka), (sb, kb) = matching._set(a), matching._set(b)
        return sa, sb, (ka, kb)

    def edit(s, **kw):
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    cases = []
    q, t, keep = sets(full, full)
    cases += [((None, t, P()), "query is null"), ((q, None, P()), "train is null"), ((q, t, None), "params is null")]
    cases += [((q, t, P(), i), name + " is null") for i, name in enumerate(NAMES)]
    qn, tn, keep2 = sets(full, full)
    cases += [((edit(qn, desc=None), t, P()), "query->desc is null"), ((q, edit(tn, desc=None), P()), "train->desc is null")]
    qb, tb, keep3 = sets(bare, bare)
    cases += [((qb, t, P(window=4.0)), "query->x is null"), ((q, tb, P(window=4.0)), "train->x is null"),
              ((qb, t, P(max_octave_diff=0)), "query->octave is null"), ((q, tb, P(max_octave_diff=0)), "train->octave is null")]
    qy, _, keep4 = sets(full, full)
    cases += [((edit(qy, y=None), t, P(window=0.0)), "query->y is null")]
    cases += [((q, t, P(max_distance=-1)), "max_distance -1 outside 0..256"), ((q, t, P(max_distance=257)), "max_distance 257 outside 0..256"),
              ((q, t, P(ratio=float("nan"))), "ratio is NaN"), ((q, t, P(window=float("nan"))), "window is NaN"),
              ((q, t, P(chunk_rows=-1)), "chunk_rows -1 is negative")]
    qm, tm, keep5 = sets(full, full)
    cases += [((edit(qm, n=-1), t, P()), "query->n -1 outside"), ((q, edit(tm, n=(1 << 24) + 1), P()), "train->n 16777217 outside")]
    for args, msg in cases:
        rc, text, untouched = _raw_call(ctx, *args)
        assert rc == K.VDO_ERR_INVALID and msg in text and "vdo_orb_match" in text, (msg, rc, text)
        assert untouched, f"{msg}: outputs were written"
    # the context still runs a good call
    _same(_match(ctx, full, full, window=16.0, max_octave_diff=1, cross_check=True), M.match_ref(full, full, window=16.0, max_octave_diff=1, cross_check=True), "after refusals")


# ---- extractors --------------------------------------------------------------------------------------------------------------------
EXT = dict(window=16.0, max_octave_diff=1, max_distance=100, cross_check=True)


@pytest.fixture(scope="module")
def two_views():
    gray = np.fromfile(os.path.join(ROOT, "tests", "golden", "inputs", "orb_gray_640x200.u8"), np.uint8).reshape(200, 640)
    return gray, np.ascontiguousarray(np.roll(gray, (3, 7), axis=(0, 1)))


def test_match_extractors_equals_match_on_the_downloaded_keypoints(ctx, two_views):
    from vdo_slam_amd import matching
    from vdo_slam_amd.frontend import ORBextractor
    assert matching.TH_HIGH == 100 and matching.TH_LOW == 50
    ga, gb = two_views
    oa, ob, fresh = ORBextractor(ctx, 640, 200), ORBextractor(ctx, 640, 200), ORBextractor(ctx, 640, 200)
    ka = oa(ga)                               # no descriptors asked for: the matcher queues K8 itself
    kb = ob(gb, descriptors=True)             # descriptors already resident
    assert ka["x"].size > 500 and kb["x"].size > 500
    got = matching.match_extractors(oa, ob, **EXT)
    ka["desc"] = oa.descriptors(ka["x"].size)                           # a later vdo_orb_descriptors: the same bytes as a fresh extraction
    assert np.array_equal(ka["desc"], fresh(ga, descriptors=True)["desc"])
    assert np.array_equal(ob.descriptors(kb["x"].size), kb["desc"])
    want = M.match_ref(ka, kb, **EXT)
    assert want[3] > 50                                                  # the shifted view does match
    _same(got, want, "match_extractors vs restatement")
    _same(matching.match(ctx, ka, kb, **EXT), want, "match vs restatement")
    # a second call (everything resident), the other direction, ungated, and one extractor against itself
    _same(matching.match_extractors(oa, ob, **EXT), want, "second call")
    _same(matching.match_extractors(ob, oa, chunk_rows=100, **EXT), M.match_ref(kb, ka, **EXT), "swapped")
    _same(matching.match_extractors(oa, ob, ratio=0.8), M.match_ref(ka, kb, ratio=0.8), "ungated")
    _same(matching.match_extractors(oa, oa, **EXT), M.match_ref(ka, ka, **EXT), "self")
    # extractors on contexts (streams) of their own
    from vdo_slam_amd.ba import Context
    c2 = Context(0)
    oc = ORBextractor(c2, 640, 200)
    kc = oc(gb)
    _same(matching.match_extractors(oa, oc, **EXT), want, "two streams")
    # a new extraction replaces what is matched
    oa(gb)
    _same(matching.match_extractors(oa, ob, **EXT), M.match_ref(kb, kb, **EXT), "after a new extraction")
    # capacity smaller than the query's keypoints
    L = matching._lib()
    L.vdo_last_error.restype = C.c_char_p
    out = np.full(kb["x"].size, -7, np.int32); m = C.c_int32(-7)
    p = matching.params(**EXT)
    ip = out.ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.vdo_orb_match_extractors(oa._h, ob._h, C.byref(p), ip, ip, ip, C.byref(m), kb["x"].size - 1)
    assert rc == -1 and b"capacity" in L.vdo_last_error() and (out == -7).all()
    for o in (oa, ob, oc, fresh):
        o.close()
    c2.close()


def test_host_class_gives_the_same_arrays(ctx, two_views):
    from vdo_slam_amd import _capi as K
    from vdo_slam_amd.frontend import ORBextractor
    ga, gb = two_views
    host = K.load_host_lib()
    fp, ip, up = K.c_float_p, K.c_int32_p, K.c_uint8_p
    host.host_orb_match.argtypes = [C.c_int, fp, fp, ip, up, C.c_int, fp, fp, ip, up, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, ip, ip]
    host.host_orb_match.restype = C.c_int
    host.host_orb_match_extractors.argtypes = [up, up, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, ip, ip, C.c_int, ip]
    host.host_orb_match_extractors.restype = C.c_int
    orb = ORBextractor(ctx, 640, 200)
    ka = orb(ga, descriptors=True); kb = orb(gb, descriptors=True)
    orb.close()
    for nnratio in (0.0, 0.8):
        prm = dict(EXT, ratio=nnratio)
        want = M.match_ref(ka, kb, **prm)
        nq = ka["x"].size
        m = np.zeros(nq, np.int32); d = np.zeros(nq, np.int32)
        args = []
        for k in (ka, kb):
            args += [k["x"].size, k["x"].ctypes.data_as(fp), k["y"].ctypes.data_as(fp), k["octave"].ctypes.data_as(ip), k["desc"].ctypes.data_as(up)]
        n = host.host_orb_match(*args, nnratio, 1, EXT["window"], EXT["max_octave_diff"], EXT["max_distance"], m.ctypes.data_as(ip), d.ctypes.data_as(ip))
        assert n == want[3] and np.array_equal(m, want[0]) and np.array_equal(d, want[1])
        m2 = np.zeros(nq, np.int32); d2 = np.zeros(nq, np.int32); nq_out = C.c_int32()
        n = host.host_orb_match_extractors(ga.ctypes.data_as(up), gb.ctypes.data_as(up), 640, 200, nnratio, 1, EXT["window"], EXT["max_octave_diff"],
                                           EXT["max_distance"], m2.ctypes.data_as(ip), d2.ctypes.data_as(ip), nq, C.byref(nq_out))
        assert nq_out.value == nq and n == want[3] and np.array_equal(m2, want[0]) and np.array_equal(d2, want[1])
