"""NumPy restatement of the instance labeller's contract (include/vdo_slam_hip.h, vdo_labels_*): links by slicing, roots by repeated
min-over-edges with pointer jumping until nothing changes, areas by bincount, the threshold A* and the ranks from their definitions.  The
device (csrc/labels.hip) is compared with this array_equal; tests/test_labels_ref.py checks this file against a plain flood fill."""
import numpy as np


def int_disparity(disp):
    """d = (int32)v by truncation where 0 <= v < 2^24, else 0 = unknown (NaN, negative, too large)"""
    v = np.asarray(disp, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (v >= 0) & (v < np.float32(2 ** 24))
    return np.where(ok, v, np.float32(0)).astype(np.int64)


def offsets(connectivity):
    return [(1, 0), (0, 1)] + ([(1, 1), (-1, 1)] if connectivity == 8 else [])


def edges(member, linked, connectivity):
    """(a, b): raster indices of the linked pairs.  member [H, W] bool; linked(p, q) -> bool array on two tuples of index arrays (ys, xs)."""
    H, W = member.shape
    idx = np.arange(H * W).reshape(H, W)
    A, B = [], []
    for dx, dy in offsets(connectivity):
        ys, xs = np.mgrid[0:H - dy, max(0, -dx):W - max(0, dx)]
        p, q = (ys, xs), (ys + dy, xs + dx)
        ok = member[p] & member[q] & linked(p, q)
        A.append(idx[p][ok]); B.append(idx[q][ok])
    return np.concatenate(A), np.concatenate(B)


def roots_of(member, a, b):
    """int64 [H, W]: the smallest raster index of each pixel's component, -1 off the components"""
    n = member.size
    mem = np.flatnonzero(member.ravel())
    lab = np.full(n, -1, np.int64)
    lab[mem] = mem
    while True:
        before = lab.copy()
        m = np.minimum(lab[a], lab[b])
        for t in (a, b, before[a], before[b]):                   # the pair and the pair's representatives take the smaller label
            np.minimum.at(lab, t, m)
        while True:                                              # pointer jumping
            nxt = lab[lab[mem]]
            if np.array_equal(nxt, lab[mem]):
                break
            lab[mem] = nxt
        if np.array_equal(lab, before):
            return lab.reshape(member.shape)


def areas_of(roots):
    """int64 [H, W]: the pixel count of each component at its root, 0 elsewhere"""
    r = roots.ravel()
    return np.bincount(r[r >= 0], minlength=r.size).reshape(roots.shape)


def area_threshold(component_areas, min_area, max_labels):
    """A*.  With A the smallest value >= min_area such that at most max_labels components have area >= A: min_area when nothing overflows
    (A == min_area); otherwise the area of the smallest component that A keeps (the smallest threshold that occurs as an area and keeps the same
    components), or A itself when it keeps none."""
    s = np.asarray(component_areas, np.int64)
    for A in sorted({int(min_area)} | {int(v) + 1 for v in s if v + 1 > min_area}):       # the count only changes just above an area
        if int((s >= A).sum()) <= max_labels:
            kept = s[s >= A]
            return A if A == min_area or kept.size == 0 else int(kept.min())
    raise AssertionError("unreachable: nothing has an area above the largest")


def components(cls, disp=None, connectivity=8, max_disp_diff=-1):
    """Instance mode, steps 1 and 2: (roots, areas)"""
    cls = np.asarray(cls)
    d = int_disparity(disp) if max_disp_diff >= 0 else np.zeros(cls.shape, np.int64)

    def linked(p, q):
        same = cls[p] == cls[q]
        if max_disp_diff < 0:
            return same
        return same & ((d[p] == 0) | (d[q] == 0) | (np.abs(d[p] - d[q]) <= max_disp_diff))

    member = cls != 0
    roots = roots_of(member, *edges(member, linked, connectivity))
    return roots, areas_of(roots)


def select(roots, areas, min_area, max_labels):
    """Step 3: (mask int32, n_labels, n_components, A*)"""
    comp = areas.ravel()[areas.ravel() > 0]
    A = area_threshold(comp, min_area, max_labels)
    kept = np.flatnonzero(areas.ravel() >= A)                    # ascending roots
    rank = np.zeros(areas.size, np.int32)
    rank[kept] = np.arange(1, kept.size + 1)
    mask = np.where(roots >= 0, rank[np.maximum(roots, 0)], 0).astype(np.int32)
    return mask, int(kept.size), int(comp.size), int(A)


def stages(cls, disp=None, connectivity=8, max_disp_diff=-1, min_area=1, max_labels=1023):
    roots, areas = components(cls, disp, connectivity, max_disp_diff)
    mask, n, nc, A = select(roots, areas, min_area, max_labels)
    return {"roots": roots.astype(np.int32), "areas": areas.astype(np.int32), "mask": mask, "counts": (n, nc, A)}


def speckle_components(disp, max_diff):
    d = int_disparity(disp)
    member = d != 0
    roots = roots_of(member, *edges(member, lambda p, q: np.abs(d[p] - d[q]) <= max_diff, 4))
    return roots, areas_of(roots)


def filter_speckles(disp, max_diff, max_size):
    """Step 4: {disp: the filtered copy, n_removed, roots, areas}"""
    disp = np.asarray(disp, np.float32)
    roots, areas = speckle_components(disp, max_diff)
    drop = (roots >= 0) & (areas.ravel()[np.maximum(roots, 0)] <= max_size)
    out = disp.copy()
    out[drop] = np.float32(0)
    return {"disp": out, "n_removed": int(drop.sum()), "roots": roots.astype(np.int32), "areas": areas.astype(np.int32)}


# ---- class images built for the purpose --------------------------------------------------------------------------------------------------
def spiral(H, W):
    """A one-pixel-wide rectangular spiral walked from the top left corner inwards, a free row / column between its arms: one component whose
    path is as long as the image allows"""
    a = np.zeros((H, W), np.uint8)
    y = x = k = 0
    a[0, 0] = 1
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]

    def can(dy, dx):                                             # the next cell is free and the one behind it as well (else the arms would touch)
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        return 0 <= ny < H and 0 <= nx < W and not a[ny, nx] and not (0 <= my < H and 0 <= mx < W and a[my, mx])

    while True:
        if not can(*steps[k]):
            k = (k + 1) % 4
            if not can(*steps[k]):
                return a
        y, x = y + steps[k][0], x + steps[k][1]
        a[y, x] = 1


def serpentine(H, W):
    """Every second row is full, joined to the next at alternating ends: one component that crosses every vertical tile edge on each such row"""
    a = np.zeros((H, W), np.uint8)
    a[::2] = 1
    a[1::4, W - 1] = 1
    a[3::4, 0] = 1
    return a


def comb(H, W, vertical):
    """Teeth along one axis joined by a spine at the far end, so that the teeth stay apart until the last row / column"""
    a = np.zeros((H, W), np.uint8)
    if vertical:
        a[:, ::2] = 1; a[H - 1] = 1
    else:
        a[::2] = 1; a[:, W - 1] = 1
    return a


def checkerboard(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys + xs) & 1).astype(np.uint8)


def noise(H, W, density, seed, classes=1):
    rng = np.random.default_rng(seed)
    fg = rng.random((H, W)) < density
    return np.where(fg, rng.integers(1, classes + 1, (H, W)), 0).astype(np.uint8)


def blobs(H, W, sizes, cls=1):
    """Squares / rectangles of the given areas (w, h pairs or square sides), left to right with a gap, top row first; returns the class image"""
    a = np.zeros((H, W), np.uint8)
    x = y = 0
    row_h = 0
    for s in sizes:
        w, h = (s, s) if np.isscalar(s) else s
        if x + w > W:
            x = 0; y += row_h + 1; row_h = 0
        assert y + h <= H, "blobs: the image is too small"
        a[y:y + h, x:x + w] = cls
        x += w + 1; row_h = max(row_h, h)
    return a
