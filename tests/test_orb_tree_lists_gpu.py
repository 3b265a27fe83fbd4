"""The device quadtree (k_quadtree, orb.hip) on candidate LISTS instead of images: vdo_orb_tree_run places a list where the compaction
puts an image's candidates and runs the extraction's own tree launch and per-level resolution, so the test, not FAST, decides which
branch of the kernel a case reaches.  Every case compares three selections with array_equal, in order: the device tree, the host
tree (a second handle created under VDO_ORB_HOST_TREE=1) and the oracle's DistributeOctTree (vdo_oracle_orb_distribute, pinned to
the verbatim reference build by tests/test_ref_orb.py); it asserts where each level ran (vdo_orb_tree_info) and repeats the device
run once, so that the scratch of the first run is reused.

Which lists pin which phase (test_the_lists_reach_what_they_claim asserts the branches from the oracle's trace, without a GPU):
  initial strips   g5 / g9 / g258 (2, 3 and 65 bucket passes of four strips), `strip` (keys on either side of every strip bound at a
                   non-integer hX, and at the region's last column), `one_strip` (every strip but the last empty);
  A, E (keys)      `line` (keys at split - 1 and split of every split line of three rounds: the ceil rounding on odd extents, g1 / g2),
                   `full` (nodes down to one pixel), the key-count edges on `big` (1 -> 2 keys per thread, LDS -> global scratch, more than
                   8 keys per thread, 32768 = the 16-bit counts' last value, 32769 = kQtCandOverflow), `ml` (adjacent levels in scratch);
  B, C (ranks)     `lat` (sibling nodes tie in size at every round: the final phase's order is the creation id alone) and `pair`
                   (adjacent pixels a split does not separate: nodes divide without the count growing - second final passes, ends on
                   "count unchanged"), with N from the trace: the last final pass stops after its first node, in the middle, after its last;
  D (nodes)        the N sweep around every round's node count; corner blocks (one child in round 1: the tree ends at once, on one node);
  best response    ties inside nodes of 2 to 50 keys, the maximum at the first, a middle and the last list position, responses 0 and 255.

Sizes.  Every geometry is accepted by vdo_orb_create as the issue names it.  `big` is 385x363, the smallest area (w, h in 64..1300 x 64..500)
whose dense capacity (32912) exceeds 32768.  A list cannot be longer than the extractor's dense capacity (vdo_orb_tree_run refuses it: the
device rows are that long), which is about a quarter of the region: 182, 476, 1105 and 1872 keys on g1, g2, g5 and g9.  So `full` is every
pixel of as many whole rows of the region as fit, not every pixel of the region, and the fuzz draws n from [1, dense capacity].

Statuses.  kQtHostLevel, kQtCandOverflow and kQtNodeOverflow are asserted where they occur.  kQtNodeOverflow is reached by the sweep's smallest N
only: the FIRST round divides every initial node before the count is tested, up to 4 nIni nodes, so N + 3 < 4 nIni can overflow there (the level
then takes the host tree, and the selection is compared like any other); a later full round runs only if count + 3 nToExpand <= N held, and a
final pass stops at N + 2 at most, so from N + 3 >= 4 nIni on the node bound excludes it.  Not reachable through the validated entry, and not
provoked: kQtBadStrip (the value checks keep every key inside the region, whose last strip ends behind the last column, and every response in
[0, 255]) and kQtRoundCap (a region fits 16-bit coordinates, so about 17 halvings reach one pixel, far below the cap of 48 rounds)."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

from tests import frontend_ref as R
from vdo_slam_amd import _capi as K
from vdo_slam_amd.frontend import ORBextractor, OrbParamsC, _lib

gpu = pytest.mark.gpu

OK, HOST_LEVEL, CAND_OVERFLOW, NODE_OVERFLOW = 0, 1, 2, 3      # the kQt* status words of orb.hip
MAX_N = 1021                                                    # kQtMaxNodes - 3: the largest N the device tree takes
MAX_CAND = 32768                                                # kQtMaxCand
F = np.float32


class Geo:
    """One-level extractor geometry: region (w - 32) x (h - 32), nIni strips of width hX (the float arithmetic of DistributeOctTree)."""

    def __init__(self, name, w, h, cap):
        self.name, self.w, self.h, self.cap = name, w, h, cap           # cap: dense capacity (asserted against the product's message in test 8)
        self.W, self.H = w - 32, h - 32
        self.nIni = int(math.floor(float(F(self.W) / F(self.H)) + 0.5))
        self.hX = F(self.W) / F(self.nIni)
        self.bounds = [int(self.hX * F(i)) for i in range(self.nIni + 1)]

    def strip(self, x):
        return (np.asarray(x, F) / self.hX).astype(np.int64)


G1, G2, G5, G9 = Geo("g1", 65, 64, 182), Geo("g2", 97, 65, 476), Geo("g5", 200, 64, 1105), Geo("g9", 320, 64, 1872)
G258 = Geo("g258", 8300, 64, 55536)
BIG = Geo("big", 385, 363, 32912)
GEOS = {g.name: g for g in (G1, G2, G5, G9, G258, BIG)}
assert [g.nIni for g in (G1, G2, G5, G9, G258, BIG)] == [1, 2, 5, 9, 258, 1]


# ------------------------------------------------------------------------------------------------------------------ a NumPy model of the full rounds
def _descend(geo, x, y, depth):
    """Node of every key after `depth` full rounds in which every node divides: [n, 5] = strip, x0, x1, y0, y1 (ceil split, a key goes
    left / up when it is below the split line)."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    s = geo.strip(x)
    b = np.asarray(geo.bounds, np.int64)
    x0, x1, y0, y1 = b[s], b[s + 1], np.zeros_like(y), np.full_like(y, geo.H)
    for _ in range(depth):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        lx, ly = x < mx, y < my
        x0, x1 = np.where(lx, x0, mx), np.where(lx, mx, x1)
        y0, y1 = np.where(ly, y0, my), np.where(ly, my, y1)
    return np.stack([s, x0, x1, y0, y1], 1)


def round_counts(geo, x, y):
    """Node counts [non-empty strips, after round 1, after round 2, ...] of full rounds that nothing stops but "count unchanged" (the last
    two entries are equal): a node with one key no longer divides, but it stays one node, so the count after r rounds is the number of
    occupied cells of depth r."""
    if len(x) == 0:
        return [0]
    out = []
    for d in range(40):
        out.append(len(np.unique(_descend(geo, x, y, d), axis=0)))
        if d and out[-1] == out[-2]:
            return out
    raise AssertionError("no end")


def boxes(geo, depth):
    """The nodes of depth `depth` of every strip, as (x0, x1, y0, y1)."""
    out = [(geo.bounds[i], geo.bounds[i + 1], 0, geo.H) for i in range(geo.nIni)]
    for _ in range(depth):
        nxt = []
        for x0, x1, y0, y1 in out:
            mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
            nxt += [(x0, mx, y0, my), (mx, x1, y0, my), (x0, mx, my, y1), (mx, x1, my, y1)]
        out = nxt
    return out


def expected_status(geo, N, x, y, node_cap_max=1024):
    n = len(x)
    if N + 3 > node_cap_max or geo.nIni > N + 3:
        return (0, HOST_LEVEL)
    if n > min(geo.cap, MAX_CAND):
        return (0, CAND_OVERFLOW)
    if n and len(np.unique(_descend(geo, x, y, 1), axis=0)) > N + 3:            # the first round's node count
        return (0, NODE_OVERFLOW)
    return (1, OK)


# ------------------------------------------------------------------------------------------------------------------------------------ the lists
def _finish(geo, rng, pts, resp=None, shuffle=True):
    """Distinct pixels inside the region, at most the dense capacity, in an order that is not the spatial one; integer responses."""
    p = np.asarray(pts, np.int64).reshape(-1, 2)
    p = p[(p[:, 0] >= 0) & (p[:, 0] < geo.W) & (p[:, 1] >= 0) & (p[:, 1] < geo.H)]
    _, first = np.unique(p[:, 0] + p[:, 1] * geo.W, return_index=True)
    p = p[np.sort(first)]
    if shuffle:
        p = p[rng.permutation(len(p))]
    p = p[:geo.cap]
    r = rng.integers(0, 256, len(p)) if resp is None else np.asarray(resp)[:len(p)]
    return p[:, 0].astype(F), p[:, 1].astype(F), r.astype(F)


def gen_u(geo, rng, n=None):
    n = min(n if n is not None else 300, geo.cap, geo.W * geo.H)
    k = rng.choice(geo.W * geo.H, n, replace=False)
    return _finish(geo, rng, np.stack([k % geo.W, k // geo.W], 1))


def gen_lat(geo, rng, n=None):
    """Two keys in opposite corners of every depth-3 node: 2, 8, 32 and 128 keys in every node of depth 3, 2, 1 and 0 - siblings, and all
    nodes of a round, tie in size at every round."""
    pts = []
    for x0, x1, y0, y1 in boxes(geo, 3):
        pts += [(x0 + 1, y0), (x1 - 1, y1 - 1)]      # (x0 + 1: the key at a strip's first column can belong to the strip before it, x / hX)
    return _finish(geo, rng, pts)


def gen_pair(geo, rng, n=None):
    """A pair of horizontally adjacent pixels in every depth-2 node, at an offset that keeps the pair together for one to three further
    divisions (the node divides into ONE child: the count does not grow), and in every second node a third key in the far corner."""
    pts = []
    for j, (x0, x1, y0, y1) in enumerate(boxes(geo, 2)):
        o = (0, 2, 1, 3)[j % 4]
        pts += [(x0 + 1 + o, y0 + j % 3), (x0 + 2 + o, y0 + j % 3)]
        if j % 2 == 0:
            pts.append((x1 - 1, y1 - 1))
    return _finish(geo, rng, pts)


def gen_pair_only(geo, rng, n=None):
    """The pairs alone, all at the node's last two columns: after two rounds every node divides into one child."""
    pts = []
    for x0, x1, y0, y1 in boxes(geo, 2):
        pts += [(x1 - 2, y0), (x1 - 1, y0)]
    return _finish(geo, rng, pts)


def gen_line(geo, rng, n=None):
    """Keys at split - 1 and split of every split line of the first three rounds, in x and in y."""
    pts = []
    for d in range(3):
        for x0, x1, y0, y1 in boxes(geo, d):
            mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
            for yy in {y0, my - 1, my, y1 - 1}:
                pts += [(mx - 1, yy), (mx, yy)]
            for xx in {x0, mx - 1, mx, x1 - 1}:
                pts += [(xx, my - 1), (xx, my)]
    return _finish(geo, rng, pts)


def gen_strip(geo, rng, n=None):
    """Keys at (int)(hX i) - 1, + 0, + 1 for every strip i and at the last column, on a few rows."""
    rows = sorted({0, 1, geo.H // 2 - 1, geo.H // 2, geo.H - 1} | set(rng.integers(0, geo.H, 3).tolist()))
    if n is not None:
        rows = rows[:max(1, n // (3 * geo.nIni + 4))]
    xs = [b + d for b in geo.bounds for d in (-1, 0, 1)] + [geo.W - 1]
    return _finish(geo, rng, [(xx, yy) for yy in rows for xx in xs])


def _corner(block, right, bottom):
    def gen(geo, rng, n=None):
        x0, y0 = (geo.W - block if right else 0), (geo.H - block if bottom else 0)
        return _finish(geo, rng, [(x0 + i, y0 + j) for j in range(block) for i in range(block)])
    return gen


def gen_full(geo, rng, n=None):
    """Every pixel of as many whole rows of the region as the dense capacity holds (see the module docstring)."""
    rows = min(geo.H, geo.cap // geo.W)
    return _finish(geo, rng, [(i, j) for j in range(rows) for i in range(geo.W)])


def gen_one_strip(geo, rng, n=None):
    x0 = geo.bounds[geo.nIni - 1]
    w = geo.W - x0
    n = min(n if n is not None else 200, geo.cap, w * geo.H)
    k = rng.choice(w * geo.H, n, replace=False)
    return _finish(geo, rng, np.stack([x0 + k % w, k // w], 1))


GENS = {"u": gen_u, "lat": gen_lat, "pair": gen_pair, "line": gen_line, "strip": gen_strip, "corner2": _corner(2, True, True),
        "corner3": _corner(3, True, False), "corner8": _corner(8, False, True), "full": gen_full, "one_strip": gen_one_strip}


def the_list(geo, gen, seed=1, n=None):
    fn = GENS.get(gen) or {"pair_only": gen_pair_only}[gen]
    return fn(geo, np.random.default_rng([seed, geo.w, sum(map(ord, gen))]), n)


def sweep(geo, lst):
    """The N of test 1: around nIni, around the node count after every full round, around n."""
    x, y, _ = lst
    n = len(x)
    s = {0, 1, 2, geo.nIni - 1, geo.nIni, geo.nIni + 1, n - 1, n, n + 1}
    for c in round_counts(geo, x, y)[1:]:
        s |= {c - 1, c, c + 1}
    return sorted(v for v in s if 0 <= v <= MAX_N)


def ref(oracle, geo, lst, N):
    return R.distribute(oracle, lst[0], lst[1], lst[2], geo.W, geo.H, N)


# Where the last final pass of the oracle stops, as a predicate on (trace, nodes returned, N)
STOPS = {
    "first": lambda t, m, N: t[1] >= 1 and t[2] == 1 and t[3] > 2 and m >= N,
    "middle": lambda t, m, N: t[1] >= 1 and 1 < t[2] < t[3] and m >= N,
    "last": lambda t, m, N: t[1] >= 1 and t[2] == t[3] > 2 and m >= N,
    "second_pass": lambda t, m, N: t[1] >= 2,
    "unchanged": lambda t, m, N: t[1] >= 1 and m < N,
}


def stop_cases(oracle, geo, lst):
    """{stop position: the smallest N that reaches it} on this list, read from the oracle's trace."""
    found = {}
    for N in range(1, min(len(lst[0]) + 2, MAX_N) + 1):
        sel, t = ref(oracle, geo, lst, N)
        for name, pred in STOPS.items():
            if name not in found and pred(t, sel.size, N):
                found[name] = N
    return found


# ------------------------------------------------------------------------------------------------------ multi-level scenarios (1242x375, 8 levels)
ML = OrbParamsC(2500, 1.2, 8, 20, 7)
ML_W, ML_H = 1242, 375
BENCH_COUNTS = (3339, 2700, 2150, 1700, 1350, 1050, 800, 605)      # about the bench frame's candidates per level


def ml_geos(oracle):
    ws, hs, nf = R.level_sizes(oracle, ML_W, ML_H, ML)
    return [Geo(f"ml{l}", int(ws[l]), int(hs[l]), 1 << 30) for l in range(ML.n_levels)], [int(v) for v in nf]


def ml_lists(oracle, scenario):
    geos, nf = ml_geos(oracle)
    counts = {"i": BENCH_COUNTS, "ii": (6000, 5000, 4500, 0, 40, 17, 5, 1), "iii": (5000, MAX_CAND + 1, 5000, 0, 0, 0, 0, 0),
              "iv": (6000, 5000, 4500, 0, 40, 17, 5, 1)}[scenario]
    return geos, nf, [gen_u(g, np.random.default_rng([7, l, c]), c) for l, (g, c) in enumerate(zip(geos, counts))]


# ------------------------------------------------------------------------------------------------------------------------------------ CPU tests
def test_the_round_model_is_the_oracle(oracle):
    """round_counts (which the N sweeps and the expected kQtNodeOverflow come from) against the oracle with N out of reach: the same
    number of full rounds, the same final node count, on every list of test 1."""
    for geo in (G1, G2, G5, G9):
        for gen in GENS:
            lst = the_list(geo, gen)
            c = round_counts(geo, lst[0], lst[1])
            sel, t = ref(oracle, geo, lst, 10 ** 6)
            assert (int(t[0]), sel.size, int(t[1])) == (len(c) - 1, c[-1], 0), (geo.name, gen, c, t, sel.size)


def test_the_lists_reach_what_they_claim(oracle):
    """Which branch of DistributeOctTree each named case reaches, from the oracle's trace alone."""
    def run(geo, gen, N):
        lst = the_list(geo, gen)
        sel, t = ref(oracle, geo, lst, N)
        return [int(v) for v in t], sel.size

    # test 1: a full round ends the tree on count >= N, and on "count unchanged"
    c = round_counts(G5, *the_list(G5, "lat")[:2])
    t, m = run(G5, "lat", c[2])                                  # every node divides into four: no final phase on the way to c[2]
    assert t[1] == 0 and t[0] == 2 and m == c[2] >= 2, (t, m, c)
    t, m = run(G2, "pair_only", MAX_N)
    assert t[1] == 0 and m == 32 and t[0] == 3, (t, m)           # the last round divides every node that still has two keys into ONE child
    t, m = run(G9, "corner8", MAX_N)
    assert t == [1, 0, 0, 0] and m == 1, (t, m)                  # a corner block: one child in round 1, "unchanged" at once, one node of 64 keys
    # the final phase entered after round 1, 2 and >= 3 (test 1's sweep holds these N: one above a round's count)
    for geo, gen, r in ((G5, "lat", 1), (G5, "lat", 2), (G9, "lat", 3), (G2, "lat", 3)):
        lst = the_list(geo, gen)
        N = round_counts(geo, lst[0], lst[1])[r] + 1
        assert N in sweep(geo, lst)
        t, m = run(geo, gen, N)
        assert t[1] >= 1 and t[0] == r and N <= m <= N + 2, (geo.name, gen, r, N, t, m)
    # test 2: the four stop positions, a second final pass, the end on "count unchanged" inside the final phase
    for geo in (G2, G5):
        lat, pair, only = (stop_cases(oracle, geo, the_list(geo, g)) for g in ("lat", "pair", "pair_only"))
        assert {"first", "middle", "last"} <= set(lat), (geo.name, lat)
        assert {"first", "middle", "second_pass", "unchanged"} <= set(pair), (geo.name, pair)
        assert "unchanged" in only, (geo.name, only)
    # ... with ties in size: every node of the lattice's sorted list has the same size
    lst = the_list(G5, "lat")
    N = stop_cases(oracle, G5, lst)["middle"]
    t = ref(oracle, G5, lst, N)[1]
    d = _descend(G5, lst[0], lst[1], int(t[0]))
    sizes = np.unique(d, axis=0, return_counts=True)[1]
    assert t[1] == 1 and len(sizes) == t[3] and sizes.min() == sizes.max() > 1, (t, sizes)
    # test 5: every level of the multi-level scenarios ends inside a final pass, as the bench frame does
    geos, nf, lists = ml_lists(oracle, "i")
    for g, N, lst in zip(geos, nf, lists):
        sel, t = ref(oracle, g, lst, N)
        assert t[0] >= 2 and t[1] >= 1 and 1 <= t[2] < t[3] and N <= sel.size <= N + 2, (g.name, N, t)


# ------------------------------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def make(ctx, w, h, prm, env=None):
    env = env or {}
    os.environ.update(env)
    try:
        return ORBextractor(ctx, w, h, prm.n_features, prm.scale_factor, prm.n_levels, prm.ini_th, prm.min_th)
    finally:
        for k in env:
            del os.environ[k]


class Pair:
    """A device-tree and a host-tree extractor of one geometry and N."""

    def __init__(self, ctx, w, h, prm, env=None):
        self.dev = make(ctx, w, h, prm, env)
        self.host = make(ctx, w, h, prm, {"VDO_ORB_HOST_TREE": "1"})
        self.n_levels = prm.n_levels

    def close(self):
        self.dev.close(); self.host.close()

    def check(self, lists, want, expect, what):
        """lists / want / expect per level: (x, y, resp); the oracle's selection; (on_device, status)."""
        a = self.dev.tree_run(lists)
        where = self.dev.tree_info()
        a2 = self.dev.tree_run(lists)
        where2 = self.dev.tree_info()
        b = self.host.tree_run(lists)
        assert where == list(expect) and where2 == list(expect), f"{what}: ran at {where}, {where2}, want {list(expect)}"
        assert self.host.tree_info() == [(0, HOST_LEVEL)] * self.n_levels, what
        for l in range(self.n_levels):
            assert np.array_equal(b[l], want[l]), f"{what}: level {l}: host tree against the oracle ({b[l].size} / {want[l].size} keypoints)"
            assert np.array_equal(a[l], want[l]), f"{what}: level {l}: device tree against the oracle ({a[l].size} / {want[l].size} keypoints)"
            assert np.array_equal(a2[l], want[l]), f"{what}: level {l}: device tree, second run"


def one_level(N):
    return OrbParamsC(N, 1.2, 1, 20, 7)


def run_by_N(ctx, oracle, geo, jobs):
    """jobs: (what, list, N) - one extractor pair per distinct N, every list that wants that N run on it."""
    by_N = {}
    for what, lst, N in jobs:
        by_N.setdefault(N, []).append((what, lst))
    for N, todo in sorted(by_N.items()):
        p = Pair(ctx, geo.w, geo.h, one_level(N))
        try:
            for what, lst in todo:
                sel, _ = ref(oracle, geo, lst, N)
                p.check([lst], [sel], [expected_status(geo, N, lst[0], lst[1])], f"{geo.name} {what} n={len(lst[0])} N={N}")
        finally:
            p.close()
    return len(by_N)


@gpu
@pytest.mark.parametrize("geo", ["g1", "g2", "g5", "g9"])
def test_geometries_by_generators(ctx, oracle, geo):
    geo = GEOS[geo]
    jobs = []
    for gen in GENS:
        lst = the_list(geo, gen)
        jobs += [(gen, lst, N) for N in sweep(geo, lst)]
    assert run_by_N(ctx, oracle, geo, jobs) > 20
    statuses = {expected_status(geo, N, lst[0], lst[1]) for _, lst, N in jobs}
    assert (1, OK) in statuses and ((0, HOST_LEVEL) in statuses) == (geo.nIni > 3)


@gpu
@pytest.mark.parametrize("geo", ["g2", "g5"])
def test_final_phase_stop_positions(ctx, oracle, geo):
    geo = GEOS[geo]
    jobs = []
    for gen in ("lat", "pair", "pair_only"):
        lst = the_list(geo, gen)
        found = stop_cases(oracle, geo, lst)
        for stop, N in found.items():
            # the N found, and its neighbours: the same pass one node earlier / later
            jobs += [(f"{gen} stop={stop}", lst, v) for v in (N - 1, N, N + 1) if 1 <= v <= MAX_N]
    assert len(jobs) >= 30
    run_by_N(ctx, oracle, geo, jobs)


def _tie_lists(geo):
    """Response ties inside the nodes N = 1 leaves (the four children of every strip: about 40 keys each): all responses equal (0, 7, 255);
    few distinct values; the node's maximum repeated at its first, a middle and its last key in list order (maximum 255, 1 over 0, 0)."""
    x, y, _ = the_list(geo, "u", seed=5)
    n = len(x)
    rng = np.random.default_rng(11)
    node = np.unique(_descend(geo, x, y, 1), axis=0, return_inverse=True)[1].ravel()
    out = [(f"all {v}", np.full(n, v)) for v in (0, 7, 255)]
    out += [("values 0..2", rng.integers(0, 3, n)), ("values 253..255", rng.integers(253, 256, n))]
    for top, lo, hi in ((255, 0, 255), (1, 0, 1), (200, 100, 200)):
        r = rng.integers(lo, hi, n)
        for k in np.unique(node):
            idx = np.flatnonzero(node == k)
            r[idx[[0, len(idx) // 2, -1]]] = top
        out.append((f"max {top} at first, middle, last", r))
    return x, y, node, out


@gpu
@pytest.mark.parametrize("geo", ["g2", "g9"])
def test_response_ties_take_the_first_in_list_order(ctx, oracle, geo):
    geo = GEOS[geo]
    x, y, node, variants = _tie_lists(geo)
    sizes = np.bincount(node)
    assert sizes.min() >= 2 and sizes.max() <= 50, sizes
    jobs = []
    for what, r in variants:
        lst = (x, y, r.astype(F))
        sel, _ = ref(oracle, geo, lst, 1)
        if what.startswith(("all", "max")):      # the first key of every node in list order, whatever the oracle says
            assert sorted(sel.tolist()) == sorted(int(np.flatnonzero(node == k)[0]) for k in np.unique(node)), what
        jobs += [(what, lst, N) for N in (1, 4 * geo.nIni + 1, 60)]
    run_by_N(ctx, oracle, geo, jobs)


@pytest.fixture(scope="module")
def big(ctx):
    p = Pair(ctx, BIG.w, BIG.h, one_level(MAX_N))
    yield p
    p.close()


def big_list(n):
    return gen_u(BIG, np.random.default_rng([3, n]), n)


@gpu
@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 16385, 32767, 32768, 32769])
def test_key_count_edges(big, oracle, n):
    lst = big_list(n)
    assert len(lst[0]) == n
    sel, _ = ref(oracle, BIG, lst, MAX_N)
    big.check([lst], [sel], [(0, CAND_OVERFLOW) if n > MAX_CAND else (1, OK)], f"big n={n}")
    assert sel.size == min(n, sel.size) and (n < MAX_N or MAX_N <= sel.size <= MAX_N + 2)


@gpu
def test_a_short_list_between_two_long_ones(big, oracle):
    """8193 keys (global scratch, 9 keys per thread), 5 keys (LDS), the 8193 again on one handle: nothing of a run survives into the next."""
    for n in (8193, 5, 8193):
        lst = big_list(n)
        big.check([lst], [ref(oracle, BIG, lst, MAX_N)[0]], [(1, OK)], f"big n={n} in sequence")


@gpu
@pytest.mark.parametrize("scenario", ["i", "ii", "iii", "iv"])
def test_multi_level(ctx, oracle, scenario):
    geos, nf, lists = ml_lists(oracle, scenario)
    env = {"VDO_ORB_QT_NODE_CAP": "500"} if scenario == "iv" else None
    expect = [(1, OK)] * ML.n_levels
    if scenario == "iii":
        expect[1] = (0, CAND_OVERFLOW)
    if scenario == "iv":
        assert nf[0] + 3 > 500 >= nf[1] + 3
        expect[0] = (0, HOST_LEVEL)
    if scenario in ("ii", "iv"):
        assert sum(len(q[0]) > 4096 for q in lists[:3]) == 3          # three adjacent levels in global scratch
    want = [ref(oracle, g, lst, N)[0] for g, N, lst in zip(geos, nf, lists)]
    p = Pair(ctx, ML_W, ML_H, ML, env)
    try:
        p.check(lists, want, expect, f"ml ({scenario})")
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("N", [255, 1021])
def test_wide_strip_on_the_device(ctx, oracle, N):
    """8300x64: 258 initial strips, 65 bucket passes.  N = 255: node_cap 258 = nIni, the create-time edge."""
    jobs = [(gen, the_list(G258, gen, n=3000), N) for gen in ("u", "strip", "one_strip")]
    assert all(len(j[1][0]) > 1000 for j in jobs)
    jobs.append(("u, 250 keys", the_list(G258, "u", n=250), N))
    # (N = 255: the first round of 3000 keys over 258 strips makes more than 258 nodes, kQtNodeOverflow; the two other lists stay on the device)
    assert [expected_status(G258, N, j[1][0], j[1][1]) for j in jobs] == ([(0, NODE_OVERFLOW)] * 2 + [(1, OK)] * 2 if N == 255 else [(1, OK)] * 4)
    run_by_N(ctx, oracle, G258, jobs)


@gpu
def test_wide_strip_one_below_the_create_time_edge(ctx, oracle):
    lst = the_list(G258, "u", n=3000)
    assert expected_status(G258, 254, lst[0], lst[1]) == (0, HOST_LEVEL)
    run_by_N(ctx, oracle, G258, [("u", lst, 254)])


FUZZ_N = (1, 3, 8, 21, 55, 144, 377, 1021)
FUZZ_LISTS = 200


def fuzz_list(geo, rng):
    n = int(round(math.exp(rng.uniform(0, math.log(geo.cap)))))
    parts = []
    for g in rng.choice(list(GENS), rng.integers(1, 4)):
        x, y, _ = GENS[g](geo, rng, n)
        parts.append(np.stack([x, y], 1))
    x, y, r = _finish(geo, rng, np.concatenate(parts))
    x, y = x[:n], y[:n]
    top = int(rng.choice([1, 2, 4, 256]))                          # few distinct responses: ties inside nodes
    return x, y, rng.integers(0, top, len(x)).astype(F)


@gpu
@pytest.mark.parametrize("geo", ["g2", "g5", "g9"])
def test_seeded_fuzz(ctx, oracle, geo):
    geo = GEOS[geo]
    t0 = time.perf_counter()
    pairs = {N: Pair(ctx, geo.w, geo.h, one_level(N)) for N in FUZZ_N}
    try:
        for k in range(FUZZ_LISTS):
            seed = [2024, geo.w, k]
            rng = np.random.default_rng(seed)
            N = int(FUZZ_N[min(len(FUZZ_N) - 1, int(rng.uniform(0, 1) * len(FUZZ_N)))])      # (8 buckets of a log-uniform N in [1, 1021])
            lst = fuzz_list(geo, rng)
            sel, _ = ref(oracle, geo, lst, N)
            pairs[N].check([lst], [sel], [expected_status(geo, N, lst[0], lst[1])], f"fuzz seed={seed} {geo.name} n={len(lst[0])} N={N}")
    finally:
        for p in pairs.values():
            p.close()
    print(f"fuzz {geo.name}: {FUZZ_LISTS} lists in {time.perf_counter() - t0:.2f} s")


def _raw_tree_run(orb, cnt, x, y, r, cap, null=None):
    L = _lib()
    L.vdo_orb_tree_run.argtypes = [C.c_void_p, K.c_int32_p, K.c_float_p, K.c_float_p, K.c_float_p, K.c_int32_p, C.c_int, K.c_int32_p]
    cnt = np.asarray(cnt, np.int32)
    x, y, r = (np.ascontiguousarray(np.concatenate([np.asarray(a, F), np.zeros(1, F)])) for a in (x, y, r))
    sel, sel_cnt = np.full(64, -77, np.int32), np.full(orb.nlevels, -77, np.int32)
    args = dict(cnt=cnt.ctypes.data_as(K.c_int32_p), x=x.ctypes.data_as(K.c_float_p), y=y.ctypes.data_as(K.c_float_p), r=r.ctypes.data_as(K.c_float_p),
                sel=sel.ctypes.data_as(K.c_int32_p), sel_cnt=sel_cnt.ctypes.data_as(K.c_int32_p))
    if null:
        args[null] = None
    rc = L.vdo_orb_tree_run(orb._h, args["cnt"], args["x"], args["y"], args["r"], args["sel"], cap, args["sel_cnt"])
    msg = (L.vdo_last_error() or b"").decode()
    return rc, msg, bool((sel == -77).all() and (sel_cnt == -77).all())


@gpu
def test_refusals_name_the_argument_and_write_nothing(ctx):
    geo = G2
    orb = make(ctx, geo.w, geo.h, one_level(20))
    try:
        ok = ([3], [0, 5, 64], [0, 7, 32], [9, 0, 255])
        rc, _, untouched = _raw_tree_run(orb, *ok, 64)
        assert rc == 0 and not untouched
        for null, name in (("cnt", "level_count"), ("x", "x"), ("y", "y"), ("r", "resp"), ("sel", "sel"), ("sel_cnt", "sel_count")):
            rc, msg, untouched = _raw_tree_run(orb, *ok, 64, null=null)
            assert rc == K.VDO_ERR_INVALID and f"null argument {name}" in msg and untouched, (null, rc, msg)
        z = np.zeros(geo.cap + 1, F)
        for what, (cnt, x, y, r, cap), word in (
                ("negative count", ([-1], [], [], [], 64), "level_count[0] = -1"),
                ("over the dense capacity", ([geo.cap + 1], z, z, z, 64), f"dense capacity is {geo.cap}"),
                ("sel too small", ([3], *ok[1:], 2), "sel_capacity 2"),
                ("non-integer x", ([3], [0, 5.5, 64], *ok[2:], 64), "x[1] = 5.5"),
                ("x at the region's width", ([3], [0, 5, geo.W], *ok[2:], 64), f"x[2] = {geo.W}"),
                ("negative x", ([3], [0, -1, 64], *ok[2:], 64), "x[1] = -1"),
                ("y at the region's height", ([3], ok[1], [0, geo.H, 32], ok[3], 64), f"y[1] = {geo.H}"),
                ("non-integer y", ([3], ok[1], [0.25, 7, 32], ok[3], 64), "y[0] = 0.25"),
                ("nan x", ([3], [0, np.nan, 64], *ok[2:], 64), "x[1]"),
                ("resp 256", ([3], *ok[1:3], [9, 0, 256], 64), "resp[2] = 256"),
                ("negative resp", ([3], *ok[1:3], [-1, 0, 255], 64), "resp[0] = -1"),
                ("non-integer resp", ([3], *ok[1:3], [9, 0.5, 255], 64), "resp[1] = 0.5")):
            rc, msg, untouched = _raw_tree_run(orb, cnt, x, y, r, cap)
            assert rc == K.VDO_ERR_INVALID and "vdo_orb_tree_run" in msg and word in msg and untouched, (what, rc, msg, untouched)
        # the capacity itself is accepted
        rc, msg, _ = _raw_tree_run(orb, [3], *ok[1:], 3)
        assert rc == 0, msg
    finally:
        orb.close()


@gpu
def test_the_dense_capacities_are_the_products(ctx):
    """The capacities this module's lists are cut to are what vdo_orb_tree_run states when it refuses one key more."""
    for geo in (G1, G2, G5, G9, G258, BIG):
        orb = make(ctx, geo.w, geo.h, one_level(20))
        try:
            z = np.zeros(geo.cap + 1, F)
            rc, msg, _ = _raw_tree_run(orb, [geo.cap + 1], z, z, z, 64)
            assert rc == K.VDO_ERR_INVALID and f"dense capacity is {geo.cap}" in msg, (geo.name, msg)
        finally:
            orb.close()


@gpu
def test_an_extraction_after_a_tree_run_is_a_fresh_handles(ctx, oracle):
    from vdo_slam_amd import synth_seq as SQ
    gray = np.ascontiguousarray(SQ.render_bench_frame(SQ.bench_spec(5, 20), 7)["gray"])
    _, _, lists = ml_lists(oracle, "ii")
    used, fresh = make(ctx, ML_W, ML_H, ML), make(ctx, ML_W, ML_H, ML)
    try:
        before = used(gray, descriptors=True)
        used.tree_run(lists)
        n = C.c_int(-1)
        K.check(_lib().vdo_orb_last_keypoints(used._h, C.byref(n)))
        assert n.value == 0                                          # no keypoints of an image on the handle now
        a, b = used(gray, descriptors=True), fresh(gray, descriptors=True)
        assert used.tree_info() == fresh.tree_info() == [(1, OK)] * ML.n_levels
    finally:
        used.close(); fresh.close()
    assert a["x"].size == b["x"].size > 1500
    for k in ("x", "y", "octave", "response", "size", "angle", "desc"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        assert np.array_equal(a[k].view(np.uint8), before[k].view(np.uint8)), k
