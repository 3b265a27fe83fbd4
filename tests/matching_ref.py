"""NumPy restatement of the descriptor matcher's contract (include/vdo_slam_hip.h, vdo_orb_match): a plain scan over all
(query, train) pairs, vectorised over blocks of queries, plus the same thing as a literal triple loop for small sets.

A set is a dict with ``desc`` [n, 32] uint8 and optionally ``x``, ``y`` (float32) and ``octave`` (int32)."""
import numpy as np

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int32)      # 256-entry table

_BIG = np.int64(1) << 40            # larger than every distance: "not a candidate"


def _arrays(s):
    desc = np.ascontiguousarray(s["desc"], np.uint8).reshape(-1, 32)
    n = desc.shape[0]
    x = None if s.get("x") is None else np.asarray(s["x"], np.float32).reshape(n)
    y = None if s.get("y") is None else np.asarray(s["y"], np.float32).reshape(n)
    o = None if s.get("octave") is None else np.asarray(s["octave"], np.int64).reshape(n)
    return desc, x, y, o


def _masked_distances(qd, qx, qy, qo, td, tx, ty, to, window, max_octave_diff):
    """[nq, nt] int64: d(i, j) where j is a candidate of i, _BIG elsewhere."""
    d = POPCOUNT[qd[:, None, :] ^ td[None, :, :]].sum(axis=2).astype(np.int64)
    cand = np.ones(d.shape, bool)
    if window >= 0:
        w = np.float32(window)
        with np.errstate(invalid="ignore"):
            # one fp32 subtraction, abs and compare per axis; a NaN compares false
            cand &= (np.abs(tx[None, :] - qx[:, None]) <= w) & (np.abs(ty[None, :] - qy[:, None]) <= w)
    if max_octave_diff >= 0:
        cand &= np.abs(to[None, :] - qo[:, None]) <= max_octave_diff
    return np.where(cand, d, _BIG)


def _best_of_rows(D):
    """Per row of D: (lowest index of the minimum or -1, best or -1, second-smallest of the multiset or -1)."""
    n, m = D.shape
    if m == 0:
        z = np.full(n, -1, np.int64)
        return z, z.copy(), z.copy()
    j = np.argmin(D, axis=1)                         # (first occurrence: the lowest index)
    best = D[np.arange(n), j]
    if m >= 2:
        second = np.partition(D, 1, axis=1)[:, 1]
    else:
        second = np.full(n, _BIG)
    none = best >= _BIG
    return np.where(none, -1, j), np.where(none, -1, best), np.where(second >= _BIG, -1, second)


def match_ref(q, t, max_distance=256, ratio=0.0, window=-1.0, max_octave_diff=-1, cross_check=False, block=128):
    """(train_idx, best_dist, second_dist, n_matches) as the contract states them; int32 arrays."""
    qd, qx, qy, qo = _arrays(q)
    td, tx, ty, to = _arrays(t)
    nq, nt = qd.shape[0], td.shape[0]
    raw = np.full(nq, -1, np.int64); best = raw.copy(); second = raw.copy()
    sl = lambda a, b0, b1: None if a is None else a[b0:b1]
    for b0 in range(0, nq, block):                   # chunked over the queries: bounds the [block, nt, 32] intermediate
        b1 = min(b0 + block, nq)
        D = _masked_distances(qd[b0:b1], sl(qx, b0, b1), sl(qy, b0, b1), sl(qo, b0, b1), td, tx, ty, to, window, max_octave_diff)
        raw[b0:b1], best[b0:b1], second[b0:b1] = _best_of_rows(D)
    ok = (raw >= 0) & (best <= max_distance)
    if 0 < ratio < 1:
        lhs = best.astype(np.float32)
        rhs = np.float32(ratio) * second.astype(np.float32)          # one fp32 multiply
        ok &= (second < 0) | (lhs < rhs)
    if cross_check:
        rev = np.full(nt, -1, np.int64)
        for b0 in range(0, nt, block):               # the reverse best of every train row: over all queries, the same gates, lowest query index on ties
            b1 = min(b0 + block, nt)
            D = _masked_distances(td[b0:b1], sl(tx, b0, b1), sl(ty, b0, b1), sl(to, b0, b1), qd, qx, qy, qo, window, max_octave_diff)
            rev[b0:b1] = _best_of_rows(D)[0]
        if nt:
            ok &= rev[np.where(raw >= 0, raw, 0)] == np.arange(nq)
    idx = np.where(ok, raw, -1)
    return idx.astype(np.int32), best.astype(np.int32), second.astype(np.int32), int(np.count_nonzero(idx >= 0))


def match_loops(q, t, max_distance=256, ratio=0.0, window=-1.0, max_octave_diff=-1, cross_check=False):
    """The same as a literal sequential scan (small sets only): strict < keeps the first best, the second-smallest is tracked beside it."""
    qd, qx, qy, qo = _arrays(q)
    td, tx, ty, to = _arrays(t)

    def scan(ad, ax, ay, ao, bd, bx, by, bo):
        n = ad.shape[0]
        raw = [-1] * n; best = [-1] * n; second = [-1] * n
        for i in range(n):
            for j in range(bd.shape[0]):
                if window >= 0:
                    with np.errstate(invalid="ignore"):
                        if not (np.abs(np.float32(bx[j]) - np.float32(ax[i])) <= np.float32(window)
                                and np.abs(np.float32(by[j]) - np.float32(ay[i])) <= np.float32(window)):
                            continue
                if max_octave_diff >= 0 and abs(int(bo[j]) - int(ao[i])) > max_octave_diff:
                    continue
                d = 0
                for k in range(32):
                    d += int(POPCOUNT[ad[i, k] ^ bd[j, k]])
                if best[i] < 0 or d < best[i]:
                    if best[i] >= 0:
                        second[i] = best[i]              # the displaced best is the runner-up: nothing between them was seen
                    best[i] = d; raw[i] = j
                elif second[i] < 0 or d < second[i]:
                    second[i] = d
        return raw, best, second

    raw, best, second = scan(qd, qx, qy, qo, td, tx, ty, to)
    rev = scan(td, tx, ty, to, qd, qx, qy, qo)[0] if cross_check else None
    idx = []
    for i in range(len(raw)):
        ok = raw[i] >= 0 and best[i] <= max_distance
        if ok and 0 < ratio < 1 and second[i] >= 0:
            ok = bool(np.float32(best[i]) < np.float32(ratio) * np.float32(second[i]))
        if ok and cross_check:
            ok = rev[raw[i]] == i
        idx.append(raw[i] if ok else -1)
    idx = np.array(idx, np.int32).reshape(-1)
    return idx, np.array(best, np.int32).reshape(-1), np.array(second, np.int32).reshape(-1), int(np.count_nonzero(idx >= 0))


def random_set(rng, n, with_pos=True, span=64.0, n_octaves=4):
    s = {"desc": rng.integers(0, 256, (n, 32), dtype=np.uint8)}
    if with_pos:
        s["x"] = rng.uniform(0, span, n).astype(np.float32)
        s["y"] = rng.uniform(0, span, n).astype(np.float32)
        s["octave"] = rng.integers(0, n_octaves, n).astype(np.int32)
    return s


def tied_set(rng, n, pool=3, flips=2, **kw):
    """Rows drawn from ``pool`` base descriptors with up to ``flips`` bits flipped: equal rows and equal distances are common."""
    s = random_set(rng, n, **kw)
    base = rng.integers(0, 256, (pool, 32), dtype=np.uint8)
    d = base[rng.integers(0, pool, n)].copy()
    for i in range(n):
        for _ in range(int(rng.integers(0, flips + 1))):
            d[i, rng.integers(0, 32)] ^= np.uint8(1 << int(rng.integers(0, 8)))
    s["desc"] = d
    return s
