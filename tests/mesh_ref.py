"""NumPy restatement of the mesher's contract (include/vdo_slam_hip.h, "Mesher"): surface nets over a TSDF volume of tests/dense_ref.py.  One vertex
per active cell at the mean of its edge crossings, one quad (two triangles) per sign-changing lattice edge whose four cells are valid.  The geometry is
float32 with one rounded operation per step in the header's order, everything else is integer: the device must equal it bit for bit."""
import numpy as np

F = np.float32


def global_words(V):
    """the words of a dense_ref.Volume as [nz, ny, nx] in GLOBAL order (index g - origin), whatever the slot alignment"""
    n, o = V.n, [int(v) for v in V.origin]
    s = [(o[a] + np.arange(n[a])) % n[a] for a in range(3)]
    return V.words[np.ix_(s[2], s[1], s[0])]


def _corner(A, d):
    """A[z + dz, y + dy, x + dx] over the cells' lower corners (each axis one shorter than A); d = (dx, dy, dz)"""
    nz, ny, nx = A.shape
    return A[d[2]:nz - 1 + d[2], d[1]:ny - 1 + d[1], d[0]:nx - 1 + d[0]]


def clip_box(V, lo, hi):
    """the box clipped to the volume in LOCAL voxels (g - origin); an empty box is (0, 0, 0), (0, 0, 0)"""
    o, n = np.array(V.origin, np.int64), np.array(V.n, np.int64)
    lo = np.maximum(np.array(lo, np.int64), o) - o; hi = np.minimum(np.array(hi, np.int64), o + n) - o
    if np.any(hi <= lo):
        return np.zeros(3, np.int64), np.zeros(3, np.int64)
    return lo, hi


def mesh(V, lo, hi, outside=0, min_weight=1, info=None):
    """-> (xyz float32 [nv, 3], grad int32 [nv, 3], weight int32 [nv], tri int32 [nt, 3]) in the contract's order.  info: a dict that receives
    "cell" (int64 [nv, 3], the LOCAL lower corner x, y, z of every vertex's cell) and "valid" (bool [nz - 1, ny - 1, nx - 1]) for the tests"""
    W = global_words(V)
    t = (W & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64); w = (W >> 16).astype(np.int64)
    nz, ny, nx = t.shape
    n = (nx, ny, nz)
    o = [int(v) for v in V.origin]
    lo, hi = clip_box(V, lo, hi)
    empty = (np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros(0, np.int32), np.zeros((0, 3), np.int32))
    if min(n) < 2:
        return empty
    # ---- cells, indexed [z, y, x] by their lower corner (local) ------------------------------------------------------------------------
    offs = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    neg = t < 0
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool); any_neg = ~valid; any_pos = ~valid
    wmin = np.full(valid.shape, 1 << 30, np.int64)
    for d in offs:
        wc = _corner(w, d); ng = _corner(neg, d)
        valid &= wc >= min_weight; any_neg |= ng; any_pos |= ~ng; wmin = np.minimum(wmin, wc)
    active = valid & any_neg & any_pos
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    c = [cx, cy, cz]

    def cell_in(shrink):                                                        # the 8 corners inside the box shrunk by `shrink` on every side
        r = np.ones(valid.shape, bool)
        for a in range(3):
            r &= (c[a] >= lo[a] + shrink) & (c[a] + 1 < hi[a] - shrink)
        return r
    emit = active & (~cell_in(1) if outside else cell_in(0))
    # ---- vertices ---------------------------------------------------------------------------------------------------------------------
    s = [np.zeros(valid.shape, F) for _ in range(3)]
    m = np.zeros(valid.shape, np.int64)
    grad = [np.zeros(valid.shape, np.int64) for _ in range(3)]
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        for dj in (0, 1):
            for di in (0, 1):
                da = [0, 0, 0]; da[i] = di; da[j] = dj
                db = list(da); db[k] = 1
                ta, tb = _corner(t, da), _corner(t, db)
                cross = (ta < 0) != (tb < 0)
                with np.errstate(all="ignore"):
                    frac = ta.astype(F) / (ta - tb).astype(F)
                for a in range(3):
                    p = F(da[a]) + frac if a == k else np.full(valid.shape, F(da[a]))
                    s[a] = np.where(cross, s[a] + p, s[a]).astype(F)
                m += cross
                grad[k] += tb - ta
    sel = emit
    mm = m[sel].astype(F)
    xyz = np.stack([(((c[a][sel] + o[a]).astype(F) + F(0.5)) + s[a][sel] / mm) * V.voxel for a in range(3)], -1).astype(F).reshape(-1, 3)
    g = np.stack([grad[a][sel] for a in range(3)], -1).astype(np.int32).reshape(-1, 3)
    wt = wmin[sel].astype(np.int32)
    vnum = np.full(valid.shape, -1, np.int64)
    vnum[sel] = np.arange(int(sel.sum()))
    if info is not None:
        info["cell"] = np.stack([c[a][sel] for a in range(3)], -1).reshape(-1, 3); info["valid"] = valid
    # ---- quads: lattice edge (a, k), a over the whole volume [z, y, x] --------------------------------------------------------------------
    vfull = np.zeros((nz, ny, nx), bool); vfull[:nz - 1, :ny - 1, :nx - 1] = valid
    nfull = np.full((nz, ny, nx), -1, np.int64); nfull[:nz - 1, :ny - 1, :nx - 1] = vnum
    az, ay, ax = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    al = [ax, ay, az]
    lin = (az * ny + ay) * nx + ax

    def shifted(A, d, fill):
        """A at a - d (d >= 0 per axis, (dx, dy, dz)), `fill` where that leaves the volume"""
        out = np.full(A.shape, fill, A.dtype)
        out[d[2]:, d[1]:, d[0]:] = A[:nz - d[2], :ny - d[1], :nx - d[0]]
        return out
    keys, tris = [], []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        ok = np.ones((nz, ny, nx), bool)
        ids = []
        for di, dj in ((1, 1), (0, 1), (0, 0), (1, 0)):
            d = [0, 0, 0]; d[i] = di; d[j] = dj
            ok &= shifted(vfull, d, False)
            ids.append(shifted(nfull, d, -1))
        tb = np.zeros_like(t); sl = [slice(None)] * 3; sl[2 - k] = slice(0, n[k] - 1); src = [slice(None)] * 3; src[2 - k] = slice(1, n[k])
        tb[tuple(sl)] = t[tuple(src)]                                            # where a + e_k leaves the volume no cell is valid
        ok &= (t < 0) != (tb < 0)
        inb = (al[i] - 1 >= lo[i]) & (al[i] + 1 < hi[i]) & (al[j] - 1 >= lo[j]) & (al[j] + 1 < hi[j]) & (al[k] >= lo[k]) & (al[k] + 1 < hi[k])
        ok &= ~inb if outside else inb
        if not ok.any():
            continue
        q = np.stack([v[ok] for v in ids], -1)
        q = np.where((t[ok] < 0)[:, None], q, q[:, ::-1])
        assert q.min() >= 0, "a quad uses a cell that is not emitted"
        keys.append(lin[ok] * 3 + k); tris.append(q)
    if tris:
        q = np.concatenate(tris)[np.argsort(np.concatenate(keys), kind="stable")]
        tri = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    else:
        tri = np.zeros((0, 3), np.int32)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(g), np.ascontiguousarray(wt), np.ascontiguousarray(tri)


def mesh_all(V, min_weight=1):
    o = [int(v) for v in V.origin]
    return mesh(V, o, [o[a] + V.n[a] for a in range(3)], 0, min_weight)


def quads_of(xyz, tri):
    """the quads of a mesh as rows of 12 float32 bit patterns (4 corner positions in the quad's order): what two meshes of the same surface share
    whatever their vertex numbering"""
    t = np.asarray(tri).reshape(-1, 2, 3)
    q = np.concatenate([t[:, 0, :], t[:, 1, 2:3]], 1)                            # (v0, v1, v2), (v0, v2, v3) -> v0 v1 v2 v3
    return np.ascontiguousarray(np.asarray(xyz, F)[q].reshape(len(q), 12)).view(np.uint32)


def sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def make_volume(n, origin, t, w, voxel=0.1):
    """A dense_ref.Volume whose GLOBAL content is t, w ([nz, ny, nx], global order): the slot alignment follows from the origin"""
    from tests import dense_ref as R
    V = R.Volume(n, voxel, origin)
    words = ((np.asarray(w).astype(np.uint32) << 16) | np.asarray(t).astype(np.int16).view(np.uint16).astype(np.uint32)).astype(np.uint32)
    words = np.where(np.asarray(w) == 0, np.uint32(0), words)
    o = [int(v) for v in origin]
    s = [(o[a] + np.arange(n[a])) % n[a] for a in range(3)]
    V.words[np.ix_(s[2], s[1], s[0])] = words
    return V


def sdf_words(n, fn, trunc=4.0):
    """t of a signed distance fn(points [.., 3] in voxel units, voxel centres at +0.5) -> int64 [nz, ny, nx]"""
    z, y, x = np.meshgrid(np.arange(n[2]) + 0.5, np.arange(n[1]) + 0.5, np.arange(n[0]) + 0.5, indexing="ij")
    d = fn(np.stack([x, y, z], -1))
    return np.floor(np.clip(d / trunc, -1, 1) * 32767 + 0.5).astype(np.int64)
