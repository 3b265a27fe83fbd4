"""The batch solver's tile planner (csrc/ba_plan.hip) on the host alone: the invariants of the layout that the tile kernels assume without checking, the
planner's refusals, its switches, and the identity of its layout with the one vdo_ba_create decided before the planner existed (tests/ba_plan_fixtures.py).
Everything here goes through vdo_ba_plan_create: no device, no context."""
import dataclasses
import json

import numpy as np
import pytest

from vdo_slam_amd import _capi as K
from vdo_slam_amd.ba import PLAN_DIMS, TILE_FIELDS, plan_graph

from tests import ba_envelope_graphs as E
from tests import ba_plan_fixtures as F
from tests.test_ba_envelope_gpu import _refused

_PLANS = {}


def _plan(name):
    """the plan of fixture `name` under the default switches (planned once; do not modify)"""
    if name not in _PLANS:
        _PLANS[name] = plan_graph(F.graph(name))
    return _PLANS[name]


def _is_permutation(a, n):
    return a.size == n and np.array_equal(np.sort(a), np.arange(n))


def check_invariants(g, p):
    """every layout invariant of the issue's list, from the plan `p` and the graph `g` alone"""
    d = p["dims"]
    T = {f: p["tiles"][:, k].astype(np.int64) for k, f in enumerate(TILE_FIELDS)}
    n_tiles, NPS, Ebp = d["tiles"], d["slots"], d["eb_entries"]
    NPS_tiles = NPS - d["hub_edges"]
    L, Eb, Et, P = g.n_point, g.n_eb, g.n_et, g.n_pose
    assert p["tiles"].shape[0] == n_tiles
    # ---- permutations
    assert _is_permutation(p["pt_old_of_new"], L)
    assert np.array_equal(p["pt_new_of_old"][p["pt_old_of_new"]], np.arange(L))
    assert _is_permutation(p["et_old_of_new"], Et)
    eb_old = p["eb_old_of_new"]
    assert eb_old.size == Ebp
    assert _is_permutation(np.concatenate([eb_old[eb_old >= 0], p["hub_eb_old"]]), Eb)
    # ---- per tile: sizes, and the build order covers points, edges, slots, chains and incidences without gaps
    assert ((T["pt_end"] - T["pt_begin"]) <= E.TILE_PTS).all() and ((T["pt_end"] - T["pt_begin"]) >= 1).all()
    assert ((T["ept"] >= 0) & (T["ept"] <= E.TILE_EPT)).all()
    nb = T["eb_end"] - T["eb_begin"]
    nt = T["et_end"] - T["et_begin"]
    assert np.array_equal(nb, E.TILE_THREADS * T["ept"])
    for lo, hi, total in (("pt_begin", "pt_end", L - d["hubs"]), ("eb_begin", "eb_end", Ebp), ("et_begin", "et_end", Et), ("slot_begin", "slot_end", NPS_tiles)):
        assert np.array_equal(T[lo][1:], T[hi][:-1]) and T[lo][0] == 0 and T[hi][-1] == total, lo
    assert np.array_equal(T["inc_begin"], np.concatenate([[0], np.cumsum(nb + 2 * nt)[:-1]]))
    assert p["inc_key"].size == int((nb + 2 * nt).sum())
    assert p["eb_key"].size == max(Ebp, E.TILE_THREADS) and (p["eb_key"][Ebp:] == -1).all()
    assert p["tile_pose"].size == NPS + 1 and p["slot_dst"].size == NPS + 1
    # ---- the edge blocks: in every thread column the edges are rows 0 .. count - 1 and share one pose slot
    key = p["eb_key"][:Ebp].astype(np.int64)
    assert np.array_equal(key >= 0, eb_old >= 0)
    tile_of_entry = np.repeat(np.arange(n_tiles), nb)
    for t in range(n_tiles):
        if not T["ept"][t]:
            continue
        k = key[T["eb_begin"][t]:T["eb_end"][t]].reshape(T["ept"][t], E.TILE_THREADS)
        valid = k >= 0
        assert (valid[1:] <= valid[:-1]).all(), t                       # a prefix of the rows
        assert ((k >> 16 == k[0:1] >> 16) | ~valid).all(), t            # one slot per thread
    v = key >= 0
    slot = T["slot_begin"][tile_of_entry[v]] + (key[v] >> 16)
    assert ((key[v] >> 16) < (T["slot_end"] - T["slot_begin"])[tile_of_entry[v]]).all()
    assert np.array_equal(p["tile_pose"][slot], g.eb_pose[eb_old[v]])
    assert np.array_equal(T["pt_begin"][tile_of_entry[v]] + (key[v] & 0xffff), p["pt_new_of_old"][g.eb_point[eb_old[v]]])
    assert ((key[v] & 0xffff) < (T["pt_end"] - T["pt_begin"])[tile_of_entry[v]]).all()
    # ---- the slots of a tile are sorted and distinct
    tp = p["tile_pose"][:NPS_tiles].astype(np.int64)
    inner = np.ones(max(NPS_tiles - 1, 0), bool)
    inner[T["slot_begin"][1:][T["slot_begin"][1:] < NPS_tiles] - 1] = False
    assert (np.diff(tp)[inner] > 0).all()
    # ---- chains: whole chains (= whole tracks) inside one tile
    co = p["chain_off"].astype(np.int64)
    assert co[0] == 0 and co[-1] == L and (np.diff(co) >= 1).all()
    assert np.array_equal(T["chain_begin"][1:], T["chain_end"][:-1]) and T["chain_begin"][0] == 0 and T["chain_end"][-1] == co.size - 1 - d["hubs"]
    assert np.array_equal(co[T["chain_begin"]], T["pt_begin"]) and np.array_equal(co[T["chain_end"]], T["pt_end"])
    single = np.zeros(max(L, 1), np.uint8)
    single[co[:-1][np.diff(co) == 1]] = 1
    assert np.array_equal(p["pt_single"], single)
    # ---- ternary edges: consecutive points of one chain, keys and incidences
    et_old = p["et_old_of_new"]
    n1, n2 = p["pt_new_of_old"][g.et_p1[et_old]].astype(np.int64), p["pt_new_of_old"][g.et_p2[et_old]].astype(np.int64)
    assert np.array_equal(n2, n1 + 1)
    assert np.array_equal(np.searchsorted(co, n1, side="right"), np.searchsorted(co, n2, side="right"))
    prev = np.full(L, -1, np.int64)
    prev[n2] = np.arange(Et)
    assert np.array_equal(p["pt_prev_edge"], prev)
    tile_of_et = np.repeat(np.arange(n_tiles), nt)
    l1, l2 = n1 - T["pt_begin"][tile_of_et], n2 - T["pt_begin"][tile_of_et]
    assert (l1 >= 0).all() and (n2 < T["pt_end"][tile_of_et]).all()
    assert np.array_equal(p["et_key"], l1 | (l2 << 16))
    sl = p["et_slot"].astype(np.int64)
    assert ((sl >= 0) & (sl < (T["slot_end"] - T["slot_begin"])[tile_of_et])).all()
    assert np.array_equal(p["tile_pose"][T["slot_begin"][tile_of_et] + sl], g.et_pose[et_old])
    j_eb = np.arange(Ebp) - T["eb_begin"][tile_of_entry]
    assert np.array_equal(p["inc_of_eb"], T["inc_begin"][tile_of_entry] + j_eb)
    j_et = np.arange(Et) - T["et_begin"][tile_of_et]
    assert np.array_equal(p["inc1_of_et"], (T["inc_begin"] + nb)[tile_of_et] + j_et)
    assert np.array_equal(p["inc2_of_et"], (T["inc_begin"] + nb + nt)[tile_of_et] + j_et)
    assert np.array_equal(p["inc_key"][p["inc_of_eb"]], p["eb_key"][:Ebp])
    assert np.array_equal(p["inc_key"][p["inc1_of_et"]], (sl << 16) | l1)
    assert np.array_equal(p["inc_key"][p["inc2_of_et"]], (sl << 16) | l2)
    # ---- slot_dst: a pose-major permutation
    sd = p["slot_dst"][:NPS].astype(np.int64)
    assert _is_permutation(sd, NPS)
    pose_of_slot = p["tile_pose"][:NPS]
    assert p["ps_off"][0] == 0 and p["ps_off"][-1] == NPS and p["ps_off"].size == P + 1
    assert ((p["ps_off"][pose_of_slot] <= sd) & (sd < p["ps_off"][pose_of_slot + 1])).all()
    assert np.array_equal(p["ps_idx"][sd], np.arange(NPS))
    if d["hubs"]:
        assert np.array_equal(p["hub_row"], sd[NPS_tiles:])
        assert np.array_equal(p["hub_pose"], g.eb_pose[p["hub_eb_old"]]) and np.array_equal(p["hub_pose"], pose_of_slot[NPS_tiles:])
    assert d["ps_stride"] in (16, 32) and (d["ps_stride"] == 32 or len(np.intersect1d(g.eb_pose, g.et_pose)) == 0)
    assert d["max_slots"] == max(1, int((T["slot_end"] - T["slot_begin"]).max()))
    # ---- launch order: the dynamic tiles first, the longest chain per tile non-increasing
    order = p["tile_order"]
    assert _is_permutation(order, n_tiles) and np.array_equal(p["tiles_launch"], p["tiles"][order])
    longest = np.maximum.reduceat(np.diff(co)[:co.size - 1 - d["hubs"]], T["chain_begin"])
    dyn = (longest > 1) | (nt > 0)
    assert d["n_dyn_tiles"] == int(dyn.sum())
    assert dyn[order][:d["n_dyn_tiles"]].all() and not dyn[order][d["n_dyn_tiles"]:].any()
    assert (np.diff(longest[order]) <= 0).all()
    # ---- pose chains
    pc_pose, pc_edge, pc_off = p["pc_pose"].astype(np.int64), p["pc_edge"].astype(np.int64), p["pc_off"].astype(np.int64)
    assert _is_permutation(pc_pose, P)
    assert pc_off[0] == 0 and pc_off[-1] == P and pc_off.size == d["n_pchains"] + 1 and d["pc_maxlen"] == int(np.diff(pc_off).max())
    assert (pc_edge[pc_off[:-1]] == -1).all()
    k = np.nonzero(pc_edge >= 0)[0]
    e, side = pc_edge[k] >> 1, pc_edge[k] & 1
    assert np.array_equal(np.where(side == 0, g.ep_i[e], g.ep_j[e]), pc_pose[k - 1])
    assert np.array_equal(np.where(side == 0, g.ep_j[e], g.ep_i[e]), pc_pose[k])
    far_pos, far_edge = p["pc_far_pos"].astype(np.int64), p["pc_far_edge"].astype(np.int64)
    c = np.nonzero(far_pos >= 0)[0]
    assert np.array_equal(far_pos < 0, far_edge < 0)
    fe, fside = far_edge[c] >> 1, far_edge[c] & 1
    assert ((pc_off[c] <= far_pos[c]) & (far_pos[c] < pc_off[c + 1] - 1)).all()
    assert np.array_equal(np.where(fside == 0, g.ep_i[fe], g.ep_j[fe]), pc_pose[far_pos[c]])
    assert np.array_equal(np.where(fside == 0, g.ep_j[fe], g.ep_i[fe]), pc_pose[pc_off[c + 1] - 1])
    used = np.concatenate([e, fe])
    assert np.unique(used).size == used.size
    if d["pose_graph_is_paths"]:
        assert used.size == g.n_ep                 # every EdgeSE3 is a link of a chain


# ------------------------------------------------------------------ a. invariants
@pytest.mark.parametrize("name", F.IDS)
def test_layout_invariants(name):
    check_invariants(F.graph(name), _plan(name))


def test_fixtures_reach_what_they_are_for():
    g = F.graph("placed")
    assert g.n_eb + 2 * g.n_et >= F.PLACE_MIN_INC > F.graph("smoke").n_eb + 2 * F.graph("smoke").n_et
    assert (_plan("twisted")["pc_far_pos"] >= 0).any()
    assert (_plan("chain_256")["dims"]["max_slots"], _plan("pieces_256")["dims"]["max_slots"]) == (511, 255)
    assert (_plan("packed_128")["dims"]["tiles"], _plan("packed_129")["dims"]["tiles"]) == (2, 3)
    assert _plan("hub_257")["dims"]["hubs"] == 1 and _plan("static_1537")["dims"]["hub_edges"] == 1537
    assert _plan("mixed_vertex")["dims"]["ps_stride"] == 32
    assert _plan("loop")["dims"]["pose_graph_is_paths"] == 0 and _plan("window")["dims"]["pose_graph_is_paths"] == 1
    assert not _plan("hub_257")["dims"]["dense_tiles_ok"] and _plan("window")["dims"]["dense_tiles_ok"]


def test_unknown_array_name_is_invalid():
    import ctypes as C
    L = K.lib()
    _plan("window")                                 # (declares the argument types)
    gc, _keep = K.graph_to_c(F.graph("window"))
    h = C.c_void_p()
    K.check(L.vdo_ba_plan_create(C.byref(gc), C.byref(h)))
    ptr, n, eb = C.c_void_p(), C.c_int64(), C.c_int32()
    assert L.vdo_ba_plan_array(h, b"no_such_array", C.byref(ptr), C.byref(n), C.byref(eb)) == -1      # VDO_ERR_INVALID
    L.vdo_ba_plan_destroy(h)


# ------------------------------------------------------------------ b. refusals without a device
@pytest.mark.parametrize("name", ["a_257_points", "b_512_poses", "b_513_poses", "c_257_pieces"])
def test_envelope_refusals_come_from_the_planner(name):
    g, env, msg = _refused(name)
    assert not env
    with pytest.raises(K.VdoError, match=msg):
        plan_graph(g)


def _i32(*v):
    return np.array(v, np.int32)


def test_structural_refusals():
    g = F.graph("window")
    statics = np.setdiff1d(np.arange(g.n_point), np.concatenate([g.et_p1, g.et_p2]))[:2]
    a, b = int(statics[0]), int(statics[1])
    m = int(g.et_pose[0])

    def with_ternary(p1, p2):
        n = len(p1)
        return dataclasses.replace(g, et_p1=np.concatenate([g.et_p1, _i32(*p1)]), et_p2=np.concatenate([g.et_p2, _i32(*p2)]),
                                   et_pose=np.concatenate([g.et_pose, _i32(*[m] * n)]), et_z=np.ascontiguousarray(np.concatenate([g.et_z, np.zeros((3, n))], 1)),
                                   et_w=np.concatenate([g.et_w, np.full(n, g.et_w[0])]))
    with pytest.raises(K.VdoError, match="ternary edges form a cycle"):
        plan_graph(with_ternary([a, b], [b, a]))
    with pytest.raises(K.VdoError, match=rf"ternary edge {g.n_et + 1}: landmark tracks must be simple chains"):
        plan_graph(with_ternary([a, a], [b, int(g.et_p1[0])]))
    bad = g.eb_pose.copy(); bad[3] = g.n_pose
    with pytest.raises(K.VdoError, match="binary edge 3: index out of range"):
        plan_graph(dataclasses.replace(g, eb_pose=bad))
    bad = g.et_p2.copy(); bad[1] = g.et_p1[1]
    with pytest.raises(K.VdoError, match="ternary edge 1: index out of range"):
        plan_graph(dataclasses.replace(g, et_p2=bad))
    bad = g.ep_j.copy(); bad[0] = -1
    with pytest.raises(K.VdoError, match="pose-pose edge 0: index out of range"):
        plan_graph(dataclasses.replace(g, ep_j=bad))
    with pytest.raises(K.VdoError, match=r"Huber width 1e-30: its square is not a normal float"):
        plan_graph(dataclasses.replace(g, huber_et=1e-30))
    # the order of refusals: the index check comes before the Huber width, the Huber width before the tracks
    with pytest.raises(K.VdoError, match="Huber width"):
        plan_graph(dataclasses.replace(with_ternary([a, b], [b, a]), huber_eb=1e-30))


# ------------------------------------------------------------------ c. switches
def test_wide_partials_switch(monkeypatch):
    assert _plan("window")["dims"]["ps_stride"] == 16
    monkeypatch.setenv("VDO_BA_WIDE_PARTIALS", "1")
    p = plan_graph(F.graph("window"))
    assert p["dims"]["ps_stride"] == 32
    check_invariants(F.graph("window"), p)


def test_no_hubs_switch_turns_the_hub_into_the_refusal(monkeypatch):
    monkeypatch.setenv("VDO_BA_NO_HUBS", "1")
    with pytest.raises(K.VdoError, match=r"touches 257 distinct pose vertices \(limit 256 per track\)"):
        plan_graph(F.graph("hub_257"))
    p = plan_graph(F.graph("smoke"))
    assert p["dims"] == _plan("smoke")["dims"]
    check_invariants(F.graph("smoke"), p)


def test_no_twist_switch(monkeypatch):
    monkeypatch.setenv("VDO_BA_NO_TWIST", "1")
    p = plan_graph(F.graph("twisted"))
    assert (p["pc_far_pos"] == -1).all() and (p["pc_far_edge"] == -1).all()
    assert np.array_equal(np.diff(p["pc_off"]), np.diff(_plan("twisted")["pc_off"]))
    check_invariants(F.graph("twisted"), p)


def test_tile_ept_switch_lowers_the_tile_size(monkeypatch):
    monkeypatch.setenv("VDO_BA_TILE_EPT", "1")
    p = plan_graph(F.graph("smoke"))
    nb_real = np.add.reduceat((p["eb_old_of_new"] >= 0).astype(np.int64), p["tiles"][:, TILE_FIELDS.index("eb_begin")])
    nt = p["tiles"][:, TILE_FIELDS.index("et_end")] - p["tiles"][:, TILE_FIELDS.index("et_begin")]
    multi = np.diff(p["tiles"][:, [TILE_FIELDS.index("chain_begin"), TILE_FIELDS.index("chain_end")]], axis=1)[:, 0] > 1
    assert (nb_real + 2 * nt)[multi].max() <= E.TILE_THREADS             # a tile of several tracks closes at 256 incidences
    assert p["dims"]["tiles"] > _plan("smoke")["dims"]["tiles"]
    check_invariants(F.graph("smoke"), p)


# ------------------------------------------------------------------ d. identity with the layout before the planner existed
@pytest.fixture(scope="module")
def golden():
    with open(F.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", F.IDS)
def test_layout_is_the_recorded_one(name, golden):
    assert sorted(golden) == sorted(F.IDS)
    want = golden[name]
    assert F.input_digest(F.graph(name)) == want["input"], f"{name}: the fixture generator changed, not the planner"
    p = _plan(name)
    assert p["dims"] == want["dims"] and tuple(sorted(want["dims"])) == tuple(sorted(PLAN_DIMS))
    assert F.plan_digest(p) == want["plan"]
