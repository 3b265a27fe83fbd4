"""Batch-BA graphs away from the operating point of synth.make_ba_graph (pose-pose residuals near the identity, scalar information matrices, one Huber
width under which every edge is an outlier, increments inside the unit ball), and the NumPy facts that say where a graph sits: which branch of
toCompactQuaternion / _q2m a residual rotation takes and by what margin, the chi2 of every edge.  No GPU and no oracle in here: tests/test_ba_offpoint.py
proves on the CPU that the builders hit what they claim, tests/test_ba_offpoint_gpu.py runs them on the device."""
import dataclasses

import numpy as np

from vdo_slam_amd import synth

# ---------------------------------------------------------------- classifiers (restated from Eigen's Quaternion(Matrix3) and g2o's toCompactQuaternion)
ROTATION_CLASSES = ("tr_pos", "x", "x_flip", "y", "y_flip", "z", "z_flip")
NEAR_TIE = 1e-5          # a residual rotation with trace < 0 whose two largest diagonal entries are closer than this counts as a near-tie


def classify_rotation(R):
    """(class, trace, raw qw, gap between the two largest diagonal entries) of a 3x3 rotation: the branch Eigen's Quaternion(Matrix3) takes - trace > 0, or the
    largest diagonal entry - and, on the other branches, whether the raw qw is negative (toCompactQuaternion then flips the sign of q)."""
    d = np.diag(R)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    s = np.sort(d)
    gap = float(s[2] - s[1])
    if tr > 0.0:
        return "tr_pos", float(tr), float(0.5 * np.sqrt(tr + 1.0)), gap
    i = 0
    if d[1] > d[0]:
        i = 1
    if d[2] > d[i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(d[i] - d[j] - d[k] + 1.0)
    qw = (R[k, j] - R[j, k]) * (0.5 / t)
    return "xyz"[i] + ("_flip" if qw < 0 else ""), float(tr), float(qw), gap


def to_vector_mqt(T):
    """toVectorMQT of a [12] isometry: (t, xyz of the normalised quaternion with w >= 0)"""
    R = synth.iso_R(T)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)                               # x y z w
    if tr > 0.0:
        t = np.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t; q[1] = (R[0, 2] - R[2, 0]) * t; q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    q /= np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    return np.concatenate([synth.iso_t(T), q[:3]])


def posepose_E(g, pose=None):
    """the residual isometries E = Z^-1 Xi^-1 Xj of every EdgeSE3 and E = Z^-1 X of every prior at `pose` (default: the graph's estimate): ([Ep,12], [Npr,12])"""
    pose = g.pose if pose is None else pose
    Ee = synth.iso_mul(synth.iso_inv(g.ep_z), synth.iso_mul(synth.iso_inv(pose[g.ep_i]), pose[g.ep_j])) if g.n_ep else np.zeros((0, 12))
    Ep = synth.iso_mul(synth.iso_inv(g.pr_z), pose[g.pr_pose]) if g.n_prior else np.zeros((0, 12))
    return Ee, Ep


def edge_chi2(g, pose=None, point=None):
    """chi2 = e^T Omega e of every edge at (pose, point), per class: dict eb, et, ep, pr"""
    pose = g.pose if pose is None else pose
    point = g.point if point is None else point
    out = {}
    e = synth.iso_apply(synth.iso_inv(pose[g.eb_pose]), point[g.eb_point]) - g.eb_z.T
    out["eb"] = g.eb_w * (e * e).sum(1)
    e = point[g.et_p1] - synth.iso_apply(synth.iso_inv(pose[g.et_pose]), point[g.et_p2]) - g.et_z.T
    out["et"] = g.et_w * (e * e).sum(1)
    Ee, Ep = posepose_E(g, pose)
    for name, E, info in (("ep", Ee, g.ep_info), ("pr", Ep, g.pr_info)):
        c = np.zeros(E.shape[0])
        for k in range(E.shape[0]):
            v = to_vector_mqt(E[k])
            c[k] = v @ info[k].reshape(6, 6) @ v
        out[name] = c
    return out


def dsqr(delta):
    """RobustKernelHuber keeps delta^2 in a float member"""
    return float(np.float32(delta * delta))


# ---------------------------------------------------------------- 2a: large residual rotations, dense information
def dense_info(rng):
    """a dense symmetric positive definite 6x6 with distinct entries: A A^T + 6 I (condition far below 1e3), at a random scale"""
    A = rng.normal(0, 1, (6, 6))
    M = A @ A.T + 6 * np.eye(6)
    M = 0.5 * (M + M.T) * 10.0 ** rng.uniform(0, 2)
    assert np.linalg.cond(M) <= 1e3 and np.unique(np.triu(M)).size == 22       # (21 distinct entries of the triangle + the zeros below it)
    return M.ravel()


def _small(rng, rot, trans):
    return synth.iso(synth.rotvec_to_R(rng.normal(0, rot, 3)), rng.normal(0, trans, 3))


HUBER_EP_POSEPOSE = 0.3


def posepose_graph(seed=5):
    """make_ba_graph(7, 30, 1, 6) - points and an object are there, so k_finalize_pose adds the pose-pose blocks onto blocks of the sweep - with its EdgeSE3 set
    replaced by: the camera chain (0,1) .. (5,6), consistent with the estimate; a reversed edge (4,2); a second edge (1,2) whose measurement is 0.5 rad off (an
    outlier under HUBER_EP_POSEPOSE at every estimate, while the chain's edge (0,1) is always an inlier); the object's smoothness edges as generated; priors on
    poses 0 and 5 (the latter at the base estimate: its residual rotation is what pose 5 is multiplied by).  Every information matrix is dense."""
    g = synth.make_ba_graph(7, 30, 1, 6, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    cam = g.pose

    def rel(i, j):
        return synth.iso_mul(synth.iso_inv(cam[i]), cam[j])
    smooth = g.ep_i >= g.n_cam
    assert smooth.sum() >= 2
    ei = [f for f in range(6)] + [4, 1]
    ej = [f + 1 for f in range(6)] + [2, 2]
    ez = [rel(f, f + 1) for f in range(6)] + [synth.iso_mul(rel(4, 2), _small(rng, 0.02, 0.05)),
                                             synth.iso_mul(rel(1, 2), synth.iso(synth.rotvec_to_R(np.array([0.3, -0.3, 0.27])), np.array([0.05, -0.02, 0.04])))]
    ep_i = np.concatenate([np.array(ei, np.int32), g.ep_i[smooth]])
    ep_j = np.concatenate([np.array(ej, np.int32), g.ep_j[smooth]])
    ep_z = np.concatenate([np.array(ez), g.ep_z[smooth]])
    ep_info = np.array([dense_info(rng) for _ in range(ep_i.size)])
    pr_pose = np.array([0, 5], np.int32)
    pr_z = np.array([synth.iso_mul(cam[0], _small(rng, 0.01, 0.02)), cam[5]])
    pr_info = np.array([dense_info(rng) for _ in range(2)])
    return dataclasses.replace(g, ep_i=ep_i, ep_j=ep_j, ep_z=np.ascontiguousarray(ep_z), ep_info=np.ascontiguousarray(ep_info), pr_pose=pr_pose,
                               pr_z=np.ascontiguousarray(pr_z), pr_info=np.ascontiguousarray(pr_info), huber_ep=HUBER_EP_POSEPOSE)


def with_asymmetric_information(g, seed=77):
    """g with a skew part added to every information matrix.  g2o takes the matrix as given - Omega e, e^T Omega e, A^T Omega B - and so do the oracle and
    k_posepose; such a matrix means nothing statistically, but it is the only input on which the ORDER of the two indices of a read of Omega shows: on a
    symmetric matrix a transposed read gives the same bits.  For one linearisation only (the solvers assume a symmetric system)."""
    rng = np.random.default_rng(seed)

    def skewed(info):
        out = info.copy()
        for k in range(out.shape[0]):
            B = np.triu(rng.uniform(0.5, 1.0, (6, 6)) * rng.choice([-1.0, 1.0], (6, 6)), 1)
            out[k] += (0.05 * np.abs(out[k]).max() * (B - B.T)).ravel()
        return out
    return dataclasses.replace(g, ep_info=skewed(g.ep_info), pr_info=skewed(g.pr_info))


def rotation_table():
    """[(name, R)]: trace > 0 at angles 0, 1e-9, 0.3, 2 pi / 3 - 0.01; each dominant diagonal entry with either sign of the dominant axis component at
    2 pi / 3 + 0.01, 2.5 and pi - 1e-3; near-ties (1e-6) of the two largest diagonal entries, every pair in either order."""
    out = []
    ax = np.array([0.5, -0.6, 0.62]); ax /= np.linalg.norm(ax)
    for th in (0.0, 1e-9, 0.3, 2 * np.pi / 3 - 0.01):
        out.append((f"pos_{th:.3g}", synth.rotvec_to_R(ax * th)))
    for d in range(3):
        for sg in (1.0, -1.0):
            for th in (2 * np.pi / 3 + 0.01, 2.5, np.pi - 1e-3):
                n = np.array([0.31, -0.23, 0.17]); n[d] = sg
                n /= np.linalg.norm(n)
                out.append((f"{'xyz'[d]}{'+' if sg > 0 else '-'}_{th:.4g}", synth.rotvec_to_R(n * th)))
    th = 2.5
    for i, j in ((0, 1), (1, 2), (2, 0)):
        for order in (1.0, -1.0):
            l = 3 - i - j
            d2 = order * 1e-6 / (1 - np.cos(th))
            n = np.zeros(3)
            n[i] = np.sqrt((0.9 + d2) / 2); n[j] = -order * np.sqrt((0.9 - d2) / 2); n[l] = np.sqrt(0.1)
            out.append((f"tie_{'xyz'[i]}{'xyz'[j]}{'>' if order > 0 else '<'}", synth.rotvec_to_R(n * th)))
    return out


def posepose_cases(g):
    """[(name, pose)]: the base poses with pose 3 and pose 5 right-multiplied by rotations of the table - every rotation once on each of the two"""
    T = rotation_table()
    out = []
    for k in range(len(T)):
        n3, R3 = T[k]
        n5, R5 = T[(k + 9) % len(T)]
        pose = g.pose.copy()
        pose[3] = synth.iso_mul(pose[3], synth.iso(R3, np.zeros(3)))
        pose[5] = synth.iso_mul(pose[5], synth.iso(R5, np.zeros(3)))
        out.append((f"{n3}|{n5}", pose))
    return out


# the three cases of the errors-only kernel (a one-iteration LM): names of posepose_cases
LM_CASES = ("x-_3.141|z+_3.141", "y+_2.5|z-_2.5", "tie_zx<|x-_2.5")

HALF_TURNS = np.array([[1, 0, 0, 0, -1, 0, 0, 0, -1], [-1, 0, 0, 0, 1, 0, 0, 0, -1], [-1, 0, 0, 0, -1, 0, 0, 0, 1],
                       [0, 1, 0, 1, 0, 0, 0, 0, -1], [0, 0, 1, 0, -1, 0, 1, 0, 0], [-1, 0, 0, 0, 0, 1, 0, 1, 0]], np.float64)


def half_turn_graph(seed=9):
    """Two poses, Xi = (I, t), Xj = (half-turn, t'), one EdgeSE3 (0, 1) with Z = I and one prior on pose 1 with Z = (I, t''): the residual rotation is the
    half-turn exactly, on the device and in the oracle (products with 0 and 1 only) - qw == 0, and for the permutation-like ones a tie on which Eigen's
    and g2o's rules differ.  Plus a prior on pose 0 (gauge).  Returns (graph, [pose sets], one per exactly representable half-turn)."""
    rng = np.random.default_rng(seed)
    z3 = np.zeros((0, 3)); zi = np.zeros(0, np.int32)
    t0, t1 = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
    poses = [np.array([synth.iso(np.eye(3), t0), np.concatenate([H, t1])]) for H in HALF_TURNS]
    I12 = synth.IDENT12.copy()
    g = synth.BAGraph(pose=poses[0].copy(), point=z3.copy(), eb_pose=zi.copy(), eb_point=zi.copy(), eb_z=np.zeros((3, 0)), eb_w=np.zeros(0),
                      et_p1=zi.copy(), et_p2=zi.copy(), et_pose=zi.copy(), et_z=np.zeros((3, 0)), et_w=np.zeros(0),
                      ep_i=np.array([0], np.int32), ep_j=np.array([1], np.int32), ep_z=I12[None].copy(), ep_info=dense_info(rng)[None].copy(),
                      pr_pose=np.array([1, 0], np.int32), pr_z=np.array([synth.iso(np.eye(3), rng.uniform(-2, 2, 3)), synth.iso(np.eye(3), t0 + 0.01)]),
                      pr_info=np.array([dense_info(rng), dense_info(rng)]), huber_ep=HUBER_EP_POSEPOSE, n_cam=2)
    return g, poses


# ---------------------------------------------------------------- 2b: Huber widths
def with_noisy_pose_edges(g, seed=31):
    """g with the measurement of every EdgeSE3 moved by N(0, (0.01 rad, 0.02 m)^2).  synth.make_ba_graph takes the odometry from the initial estimate itself and
    starts the motions at the identity: its pose-pose residuals are exactly zero or rounding noise, and no width splits them.  With this they have a distribution."""
    rng = np.random.default_rng(seed)
    z = np.array([synth.iso_mul(g.ep_z[k], _small(rng, 0.01, 0.02)) for k in range(g.n_ep)]).reshape(-1, 12)
    return dataclasses.replace(g, ep_z=np.ascontiguousarray(z))


def general_inputs(g0, seed=4):
    """per-edge weights, measurements that are not floats, non-zero ternary measurements: the general edge-input path (test_ba_gpu.test_general_edge_inputs_match_oracle)"""
    rng = np.random.default_rng(seed)
    return dataclasses.replace(g0, eb_w=g0.eb_w * rng.uniform(0.5, 2.0, g0.eb_w.shape), eb_z=g0.eb_z + rng.normal(0, 1e-7, g0.eb_z.shape),
                               et_w=g0.et_w * rng.uniform(0.5, 2.0, g0.et_w.shape), et_z=g0.et_z + rng.normal(0, 1e-3, g0.et_z.shape))


HUBER_CLASSES = ("eb", "et", "ep")


def median_widths(g):
    """per class the median of sqrt(chi2) of its edges at the graph's estimate (a class without edges keeps its width)"""
    c = edge_chi2(g)
    return {k: float(np.median(np.sqrt(c[k]))) if c[k].size else float(getattr(g, "huber_" + k)) for k in HUBER_CLASSES}


def huber_sets(g):
    """{name: (huber_eb, huber_et, huber_ep)}: each class at its median; three different widths (one class at its median, one without kernel, one at 1e-4) in
    its three rotations; all off; all inliers"""
    m = median_widths(g)
    sets = {"median": (m["eb"], m["et"], m["ep"])}
    three = (("eb", "et", "ep"), ("et", "ep", "eb"), ("ep", "eb", "et"))
    for a, b, c in three:
        w = {a: m[a], b: 0.0, c: 1e-4}
        sets[f"median_{a}_off_{b}"] = (w["eb"], w["et"], w["ep"])
    sets["all_off"] = (-1.0, -1.0, -1.0)
    sets["all_inliers"] = (1e6, 1e6, 1e6)
    return sets


def with_widths(g, w):
    return dataclasses.replace(g, huber_eb=float(w[0]), huber_et=float(w[1]), huber_ep=float(w[2]))


def huber_graphs():
    """{name: graph}: make_ba_graph(12, 300, 2, 40, seed=21) on its compact and on its general edge-input path, and a graph with a hub landmark (k_hub_sweep)"""
    from tests import ba_envelope_graphs as E
    g0 = with_noisy_pose_edges(synth.make_ba_graph(12, 300, 2, 40, seed=21))
    return {"compact": g0, "general": general_inputs(g0), "hub": with_noisy_pose_edges(E.hub_graph(E.STATIC_SLOTS + 1)[0])}


# ---------------------------------------------------------------- 2c: increments outside the unit ball
def unit_ball_graph(with_edges=False):
    """Three poses at the identity, one EdgeSE3Prior each (information I6): the prior of pose 1 is 172 degrees about (0.2, 1, 0.1) and (1, 0.5, -0.3) away, that
    of pose 2 0.3 rad about x and (0.1, 0, 0), that of pose 0 the identity.  The first Levenberg step asks pose 1 for an increment with |q| > 1 -
    fromCompactQuaternion then returns the identity rotation - and is accepted.  with_edges: two weak EdgeSE3 (0,1), (1,2) couple the poses, so that the
    reduced system is not block diagonal."""
    z3 = np.zeros((0, 3)); zi = np.zeros(0, np.int32)
    ax = np.array([0.2, 1.0, 0.1]); ax /= np.linalg.norm(ax)
    pr_z = np.array([synth.IDENT12, synth.iso(synth.rotvec_to_R(ax * np.deg2rad(172.0)), np.array([1.0, 0.5, -0.3])),
                     synth.iso(synth.rotvec_to_R(np.array([0.3, 0.0, 0.0])), np.array([0.1, 0.0, 0.0]))])
    I6 = np.eye(6).ravel()
    ne = 2 if with_edges else 0
    return synth.BAGraph(pose=np.tile(synth.IDENT12, (3, 1)), point=z3.copy(), eb_pose=zi.copy(), eb_point=zi.copy(), eb_z=np.zeros((3, 0)), eb_w=np.zeros(0),
                         et_p1=zi.copy(), et_p2=zi.copy(), et_pose=zi.copy(), et_z=np.zeros((3, 0)), et_w=np.zeros(0),
                         ep_i=np.arange(ne, dtype=np.int32), ep_j=np.arange(1, ne + 1, dtype=np.int32), ep_z=np.tile(synth.IDENT12, (ne, 1)),
                         ep_info=np.tile(UNIT_BALL_EDGE_INFO * I6, (ne, 1)), pr_pose=np.arange(3, dtype=np.int32), pr_z=np.ascontiguousarray(pr_z),
                         pr_info=np.tile(I6, (3, 1)), n_cam=3)


UNIT_BALL_EDGE_INFO = 1e-3
