"""Graphs that sit exactly on (or one past) a capacity edge of the batch solver's tile planner (csrc/ba_plan.hip, ba_dev.hpp; the LDS edges: csrc/capi_ba.hip), and the host-side
facts that say where a graph sits.  Built on synth.make_ba_graph / synth.with_hub_points and dataclasses.replace; every added measurement is
fp32-representable, like the graphs the reference builds."""
import dataclasses

import numpy as np

from vdo_slam_amd import synth

TILE_PTS = 256          # VDO_TILE_PTS
TILE_THREADS = 256      # VDO_TILE_THREADS
TILE_EPT = 6            # VDO_TILE_EPT
TILE_INC = TILE_THREADS * TILE_EPT
HARD_SLOTS = 512        # kHardSlots
STATIC_SLOTS = 256      # kStaticSlots
LDS_MAX = 160 * 1024    # VDO_LDS_MAX_BYTES


# ---- the tile kernels' LDS (bytes per workgroup), as the size helpers of csrc/ba_sweep.hip and csrc/ba_solve.hip compute it (no tile kernel has static LDS)
def sweep_lds(max_slots, ps_stride, build=True):
    S = max_slots
    return 8 * (3 * (TILE_PTS + 2) + (4 * TILE_PTS if build else 0) + 12 * S + ((ps_stride + 2) * S + (S + 1) // 2 if build else 0) + 40)


def precond_lds(max_slots):
    return 8 * (33 * max_slots + 3 * (TILE_PTS + 2) + (max_slots + 1) // 2)


def dense_tile_lds(max_slots):
    return 8 * (39 * TILE_PTS + 48 * max_slots) + 4 * (3 * TILE_PTS + TILE_PTS // 2 + 4 + max_slots)


def largest_fitting(size_of):
    """the largest slot count whose workgroup fits the LDS"""
    s = 1
    while size_of(s + 1) <= LDS_MAX:
        s += 1
    return s


def wide_slot_limit():
    """largest tile (pose slots) the tile kernels can launch with 32 sums per partial row"""
    return largest_fitting(lambda s: max(sweep_lds(s, 32), precond_lds(s)))


def dense_slot_limit():
    return largest_fitting(dense_tile_lds)


# ---- host-side facts
def chains(g):
    """landmark tracks as lists of point ids in chain order (a static point is a chain of one)"""
    nxt = dict(zip(g.et_p1.tolist(), g.et_p2.tolist()))
    has_prev = set(g.et_p2.tolist())
    out = []
    for l in range(g.n_point):
        if l in has_prev:
            continue
        c = [l]
        while c[-1] in nxt:
            c.append(nxt[c[-1]])
        out.append(c)
    return out


def track_facts(g, pts):
    """(points, incidences, distinct pose vertices, per-pose pieces) of the track through `pts`: what the planner (csrc/ba_plan.hip build_tiles) checks a track against"""
    ps = set(pts)
    eb = np.isin(g.eb_point, list(ps))
    et = np.isin(g.et_p2, list(ps)) & np.isin(g.et_p1, list(ps))
    cams, cnt = np.unique(g.eb_pose[eb], return_counts=True)
    distinct = len(set(cams.tolist()) | set(g.et_pose[et].tolist()))
    pieces = int(((cnt + TILE_EPT - 1) // TILE_EPT).sum())
    return len(pts), int(eb.sum() + 2 * et.sum()), distinct, pieces


def longest_chain(g):
    return max(chains(g), key=len)


# ---- construction
def _observe(g, cam, X, rng, sigma=0.05):
    R = g.pose_gt[cam, :9].reshape(3, 3)
    t = g.pose_gt[cam, 9:]
    return np.float32(R.T @ (X - t) + rng.normal(0, sigma, 3)).astype(np.float64)


def add_observations(g, obs, seed=0):
    """g with one more EdgeSE3PointXYZ per (pose, point) in `obs` (the point's ground truth seen from the pose's, plus noise); weight of the point's
    existing edges"""
    rng = np.random.default_rng(seed)
    if not obs:
        return g
    ep = np.array([o[0] for o in obs], np.int32)
    el = np.array([o[1] for o in obs], np.int32)
    ez = np.array([_observe(g, c, g.point_gt[l], rng) for c, l in obs]).T
    w_of = {}
    for p, w in zip(g.eb_point.tolist(), g.eb_w.tolist()):
        w_of.setdefault(p, w)
    ew = np.array([w_of.get(l, g.eb_w[0]) for l in el.tolist()])
    return dataclasses.replace(g, eb_pose=np.concatenate([g.eb_pose, ep]), eb_point=np.concatenate([g.eb_point, el]),
                               eb_z=np.ascontiguousarray(np.concatenate([g.eb_z, ez], 1)), eb_w=np.concatenate([g.eb_w, ew]))


def chain_graph(n_points, extra_cams=0, frames=None, n_static=None, seed=1):
    """One object, one dynamic track: a chain of `n_points` points over frames 0 .. n_points - 1 (n_points cameras + n_points - 1 motion vertices), its last
    point also seen from `extra_cams` cameras that follow - 2 n_points - 1 + extra_cams distinct pose vertices.  Built from make_ba_graph's track over every
    frame (long_dyn_tracks=1), cut behind point n_points - 1: the rest of it is a track of its own."""
    F = frames or n_points + extra_cams
    assert F >= n_points + extra_cams
    g = synth.make_ba_graph(F, n_static if n_static is not None else 6 * F, 1, 1, seed=seed, long_dyn_tracks=1, outlier_frac=0.0)
    c = longest_chain(g)
    assert len(c) == F
    if n_points < F:
        keep = ~((g.et_p1 == c[n_points - 1]) & (g.et_p2 == c[n_points]))
        assert (~keep).sum() == 1
        g = dataclasses.replace(g, et_p1=g.et_p1[keep], et_p2=g.et_p2[keep], et_pose=g.et_pose[keep],
                                et_z=np.ascontiguousarray(g.et_z[:, keep]), et_w=g.et_w[keep])
    g = add_observations(g, [(n_points + k, c[n_points - 1]) for k in range(extra_cams)], seed=seed + 100)
    return g, c[:n_points]


def with_motion_observation(g, pts):
    """g with ONE EdgeSE3PointXYZ whose pose vertex is a motion vertex of the track through `pts` (a .g2o file may hold one): that vertex then carries both
    edge kinds and the sweep's partial rows are 32 wide.  The vertex is one the track touches already: its slot count does not change."""
    sel = np.isin(g.et_p2, pts)
    m = int(g.et_pose[sel][0])
    l = int(g.et_p2[sel][0])
    assert m >= g.n_cam
    return add_observations(g, [(m, l)], seed=7)


def repeated_chain_graph(n_points, reps, seed=1):
    """A chain of `n_points` points whose point k is observed reps[k] times by its own camera (several observations of a point from the same camera):
    sum over the cameras of ceil(reps / VDO_TILE_EPT) per-pose pieces."""
    g, c = chain_graph(n_points, seed=seed)
    obs = [(k, c[k]) for k in range(n_points) for _ in range(int(reps[k]) - 1)]
    return add_observations(g, obs, seed=seed + 200), c


def static_point_graph(counts, seed=5):
    """make_ba_graph without objects, over len(counts) frames, whose point 0 (static: a hub candidate, like synth.with_hub_points') is seen counts[c] times
    from camera c and from no other camera"""
    g = synth.make_ba_graph(len(counts), 400, 0, 0, seed=seed, outlier_frac=0.0)
    l = 0                                                    # (no objects: every point is static)
    keep = g.eb_point != l
    g = dataclasses.replace(g, eb_pose=g.eb_pose[keep], eb_point=g.eb_point[keep], eb_z=np.ascontiguousarray(g.eb_z[:, keep]), eb_w=g.eb_w[keep])
    return add_observations(g, [(c, l) for c, n in enumerate(counts) for _ in range(int(n))], seed=seed + 300), l


def hub_graph(cams, seed=5):
    """with_hub_points on a graph of `cams` frames: one static point seen from every camera"""
    g = synth.with_hub_points(synth.make_ba_graph(cams, 400, 0, 0, seed=seed), 1, seed=2)
    per_point = np.bincount(g.eb_point, minlength=g.n_point)
    return g, int(np.argmax(per_point))


def packed_chains_graph(n_short, seed=3):
    """A 256-frame chain (its own tile: 256 points) and `n_short` two-point tracks of the same object, track j in frames 2j, 2j + 1 (mod 256), each point seen
    once: the long track raises the slot cap of the dynamic tiles to its 511 slots, so the two-point tracks pack into one tile until its points (2 each) and its
    per-pose pieces (one camera each) reach 256 - exactly at 128 tracks.  No static points: the graph's tiles are the dynamic ones alone (a static point may join
    the last dynamic tile)."""
    g, _ = chain_graph(256, n_static=0, seed=seed)
    rng = np.random.default_rng(seed + 400)
    F = g.n_cam
    P0 = g.n_pose
    pts, pts_gt, et_p1, et_p2, et_pose, obs = [], [], [], [], [], []
    for j in range(n_short):
        f = (2 * j) % (F - 1)
        body = np.array([rng.uniform(-1, 1), rng.uniform(-0.8, 0.8), rng.uniform(-2, 2)])
        m = F + f                                           # motion vertex of frame f + 1 (synth.make_ba_graph: P_cam + (f - 1) * K + k, K = 1)
        H = g.pose_gt[m]
        cam = g.pose_gt[f]
        X1 = cam[:9].reshape(3, 3) @ (body + np.array([0.0, 0.0, 12.0])) + cam[9:]
        X2 = H[:9].reshape(3, 3) @ X1 + H[9:]
        a = g.n_point + len(pts)
        for X in (X1, X2):
            pts_gt.append(X)
            pts.append(np.float32(X + rng.normal(0, 0.05, 3)).astype(np.float64))
        et_p1.append(a); et_p2.append(a + 1); et_pose.append(m)
        obs += [(f, a), (f + 1, a + 1)]
    n = len(et_p1)
    g = dataclasses.replace(g, point=np.concatenate([g.point, np.array(pts).reshape(-1, 3)]), point_gt=np.concatenate([g.point_gt, np.array(pts_gt).reshape(-1, 3)]),
                            et_p1=np.concatenate([g.et_p1, np.array(et_p1, np.int32)]), et_p2=np.concatenate([g.et_p2, np.array(et_p2, np.int32)]),
                            et_pose=np.concatenate([g.et_pose, np.array(et_pose, np.int32)]), et_z=np.ascontiguousarray(np.concatenate([g.et_z, np.zeros((3, n))], 1)),
                            et_w=np.concatenate([g.et_w, np.full(n, g.et_w[0])]))
    assert P0 == g.n_pose
    w_dyn = g.eb_w[np.isin(g.eb_point, longest_chain(g))][0]
    g = add_observations(g, obs, seed=seed + 500)
    g.eb_w[-len(obs):] = w_dyn
    return g
