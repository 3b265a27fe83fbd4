"""NumPy restatement of the distance field's contract (include/vdo_slam_hip.h, vdo_distance_*) over tests/dense_ref.py volumes: valid, site and state
from the words, the field as plain separable minima in integers, the sample in float32 with one rounded operation per step.  The device must equal
it bit for bit."""
import numpy as np

F = np.float32
FAR = 0x0FFFFFFF
OUTSIDE = 0xFFFFFFFF


def clip(V, lo, hi):
    """The box clipped to the volume, global voxels; (0, 0, 0), (0, 0, 0) when nothing is left"""
    o, n = np.asarray(V.origin, np.int64), np.array(V.n, np.int64)
    lo = np.maximum(np.array(lo, np.int64), o); hi = np.minimum(np.array(hi, np.int64), o + n)
    if np.any(hi <= lo):
        return np.zeros(3, np.int64), np.zeros(3, np.int64)
    return lo, hi


def _global_order(V):
    """t and w of the whole volume as [nz, ny, nx] arrays in GLOBAL order (index g - o)"""
    idx = [(np.arange(V.origin[a], V.origin[a] + V.n[a]) % V.n[a]) for a in range(3)]
    words = V.words[np.ix_(idx[2], idx[1], idx[0])]
    return (words & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64), (words >> 16).astype(np.int64)


def _cut(a, V, lo, hi):
    o = np.asarray(V.origin, np.int64)
    return a[lo[2] - o[2]:hi[2] - o[2], lo[1] - o[1]:hi[1] - o[1], lo[0] - o[0]:hi[0] - o[0]]


def _volume_sites(V, min_weight):
    t, w = _global_order(V)
    valid = w >= min_weight
    neg = t < 0
    site = np.zeros(t.shape, bool)
    for ax in range(3):                                     # array axis 0 is z; the rule is the same on every axis
        a = [slice(None)] * 3; b = [slice(None)] * 3
        a[ax] = slice(0, -1); b[ax] = slice(1, None)
        a, b = tuple(a), tuple(b)
        cross = valid[a] & valid[b] & (neg[a] != neg[b])    # a lattice edge of the VOLUME with a sign change between two valid ends
        site[a] |= cross; site[b] |= cross
    return site, valid, neg


def sites(V, lo, hi, min_weight):
    """bool [bz, by, bx] over the clipped box"""
    lo, hi = clip(V, lo, hi)
    return _cut(_volume_sites(V, min_weight)[0], V, lo, hi)


def state(V, lo, hi, min_weight):
    """uint8 [bz, by, bx] over the clipped box: 0 unknown, 1 free, 2 inside"""
    lo, hi = clip(V, lo, hi)
    _, valid, neg = _volume_sites(V, min_weight)
    return _cut(np.where(valid, np.where(neg, 2, 1), 0).astype(np.uint8), V, lo, hi)


def _axis_min(f, ax):
    """out(p) = min_q f(q) + (p - q)^2 along one axis, all q"""
    L = f.shape[ax]
    p = np.arange(L, dtype=np.int64).reshape([L if k == ax else 1 for k in range(3)])
    out = np.full(f.shape, np.iinfo(np.int64).max, np.int64)
    for q in range(L):
        out = np.minimum(out, np.take(f, [q], axis=ax) + (p - q) ** 2)
    return out


def field(V, lo, hi, min_weight, radius):
    """-> (words uint32 [bz, by, bx], lo, hi): the clipped box's field; sites outside the box do not count"""
    lo, hi = clip(V, lo, hi)
    s = sites(V, lo, hi, min_weight)
    f = np.where(s, 0, FAR).astype(np.int64)
    for ax in (2, 1, 0):                                    # x, y, z
        f = _axis_min(f, ax)
    d2 = np.where(f <= int(radius) ** 2, f, FAR).astype(np.uint32)
    return d2 | (state(V, lo, hi, min_weight).astype(np.uint32) << 28), lo, hi


def sample(words, lo, hi, voxel, xyz):
    """The snapshot (words over the global box [lo, hi), voxel size) at world points float32 [m, 3] -> uint32 [m]"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    inside = np.ones(len(xyz), bool)
    g = np.zeros((len(xyz), 3), np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            p = xyz[:, a]
            b = np.floor(p / F(voxel))
            assert b.dtype == F
            ok = (np.abs(p) <= np.finfo(F).max) & (b >= F(-4194304.0)) & (b <= F(4194303.0))
            g[:, a] = np.where(ok, b, 0).astype(np.int64)
            inside &= ok & (g[:, a] >= lo[a]) & (g[:, a] < hi[a])
    out = np.full(len(xyz), OUTSIDE, np.uint32)
    gi = g[inside] - np.asarray(lo, np.int64)
    out[inside] = np.asarray(words)[gi[:, 2], gi[:, 1], gi[:, 0]]
    return out


def sparse_volume(dense_ref, n, k, origin, seed=0, voxel=0.05):
    """The test volumes: t = +3000 everywhere except k random voxels at -3000, w random in 1..5, 4 % of the voxels unseen (the whole word 0).  With more
    than one voxel, the first seed from `seed` on whose volume has a site at min_weight 1 and at min_weight 2, so that no case is vacuous."""
    while True:
        V = _sparse_volume(dense_ref, n, k, origin, seed, voxel)
        hi = V.origin + np.array(V.n)
        if int(np.prod(n)) == 1 or all(sites(V, V.origin, hi, mw).any() for mw in (1, 2)):
            return V
        seed += 1


def _sparse_volume(dense_ref, n, k, origin, seed, voxel):
    rng = np.random.default_rng(seed)
    V = dense_ref.Volume(n, voxel, origin)
    shape = V.words.shape
    t = np.full(shape, 3000, np.int64)
    flat = rng.choice(t.size, size=min(k, t.size), replace=False)
    t.reshape(-1)[flat] = -3000
    w = rng.integers(1, 6, shape)
    unseen = rng.random(shape) < 0.04
    words = (w.astype(np.uint32) << 16) | t.astype(np.int16).view(np.uint16).astype(np.uint32)
    V.words = np.where(unseen, np.uint32(0), words).astype(np.uint32)
    return V


# the sizes of the parity tests, as (nx, ny, nz), k, R
CASES = [((1, 1, 1), 1, 1), ((2, 1, 1), 1, 1), ((3, 2, 2), 1, 2), ((17, 5, 9), 3, 3), ((65, 3, 3), 2, 7), ((257, 2, 2), 2, 100), ((3, 3, 130), 2, 40), ((2, 70, 2), 1, 8191),
         ((33, 33, 33), 6, 5)]
ORIGINS = [(0, 0, 0), (-37, 5, -101)]                       # the second negative and no multiple of 64


def corner_box():
    """A 5^3 box with exactly one site, at its corner (0, 0, 0): the volume is one voxel longer on x and its one negative voxel (-1, 0, 0) lies outside
    the box -> (volume, lo, hi)"""
    from tests import dense_ref as R
    V = R.Volume((6, 5, 5), 0.05, (-1, 0, 0))
    V.words[:] = (2 << 16) | 3000
    V.words[0, 0, (-1) % 6] = (2 << 16) | (-3000 & 0xFFFF)
    return V, (0, 0, 0), (5, 5, 5)
