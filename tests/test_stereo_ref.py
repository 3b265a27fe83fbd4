"""CPU: the NumPy restatement of the stereo contract (tests/stereo_ref.py) against a literal per-pixel scalar transcription of
include/vdo_slam_hip.h (vdo_stereo_compute), hand-made cases, and ground-truth recovery on built scenes."""
import functools

import numpy as np
import pytest

from tests import stereo_ref as R

INF = float("inf")


# ---- the contract, pixel by pixel --------------------------------------------------------------------------------------------------
def scalar_census(img):
    H, W = img.shape
    out = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            k = 0
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dx == 0 and dy == 0:
                        continue
                    if img[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)] < img[y, x]:
                        out[y][x] |= 1 << k
                    k += 1
    return out


def scalar_volume(left, right, D, p1, p2, paths):
    H, W = left.shape
    cl, cr = scalar_census(left), scalar_census(right)
    C = [[[bin(cl[y][x] ^ cr[y][x - d]).count("1") if x - d >= 0 else 62 for d in range(D)] for x in range(W)] for y in range(H)]
    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    dirs = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)][:paths]
    for dx, dy in dirs:
        L = {}
        ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
        xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
        for y in ys:
            for x in xs:
                px, py = x - dx, y - dy
                if px < 0 or px >= W or py < 0 or py >= H:
                    L[x, y] = list(C[y][x])
                else:
                    P = L[px, py]
                    m = min(P)
                    row = []
                    for d in range(D):
                        cand = [P[d], m + p2]
                        if d - 1 >= 0: cand.append(P[d - 1] + p1)
                        if d + 1 < D: cand.append(P[d + 1] + p1)
                        row.append(C[y][x][d] + min(cand) - m)
                    L[x, y] = row
                for d in range(D):
                    S[y][x][d] += L[x, y][d]
    return cl, cr, C, S


def scalar_select(S, W, H, D, uniqueness, lr_max_diff, subpixel):
    def d_right(xp, y):
        best, arg = None, 0
        for d in range(D):
            if xp + d < W and (best is None or S[y][xp + d][d] < best):
                best, arg = S[y][xp + d][d], d
        return arg
    out = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            s = S[y][x]
            ds = min(range(D), key=lambda d: (s[d], d))
            s0 = s[ds]
            if ds < 1 or x - ds < 0:
                continue
            if uniqueness > 0:
                s2 = min([s[d] for d in range(D) if abs(d - ds) > 1], default=INF)
                if not 100 * s0 < (100 - uniqueness) * s2:
                    continue
            if lr_max_diff >= 0 and abs(d_right(x - ds, y) - ds) > lr_max_diff:
                continue
            off = 0
            if subpixel and 1 <= ds <= D - 2:
                den = s[ds - 1] + s[ds + 1] - 2 * s0
                if den > 0:
                    num = 128 * (s[ds - 1] - s[ds + 1])
                    off = (1 if num > 0 else -1 if num < 0 else 0) * ((2 * abs(num) + den) // (2 * den))
            out[y, x] = float(256 * ds + off)
    return out


@functools.lru_cache(maxsize=None)
def _pair(H, W, D):
    left, right, _, _ = R.scene(H, W, D, seed=H + W)
    return left, right


@functools.lru_cache(maxsize=None)
def _scalar(H, W, D, paths):
    left, right = _pair(H, W, D)
    return scalar_volume(left, right, D, 10, 120, paths)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("H,W,D", [(9, 13, 16), (12, 20, 32)])
def test_stages_equal_the_scalar_transcription(H, W, D, paths):
    left, right = _pair(H, W, D)
    cl, cr, C, S = _scalar(H, W, D, paths)
    got = R.stages(left, right, max_disparity=D, paths=paths)
    assert np.array_equal(got["census_l"], np.array(cl, np.uint64)) and np.array_equal(got["census_r"], np.array(cr, np.uint64))
    assert np.array_equal(got["cost"], np.array(C)) and got["cost"].dtype == np.uint8
    assert np.array_equal(got["aggregated"], np.array(S)) and got["aggregated"].dtype == np.uint16
    for uniq in (0, 5, 60):
        for lr in (-1, 0, 1):
            for sub in (0, 1):
                want = scalar_select(S, W, H, D, uniq, lr, sub)
                out = R.select(got["aggregated"], uniq, lr, sub)
                assert np.array_equal(out, want), (uniq, lr, sub)
                assert out.dtype == np.float32
    assert got["n_valid"] == np.count_nonzero(scalar_select(S, W, H, D, 5, 1, 1))


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------
def _volume(D, W=40, fill=500):
    """One row of W pixels whose S is `fill` everywhere"""
    return np.full((1, W, D), fill, np.uint16)


def test_constant_images_have_no_valid_pixel():
    img = np.full((10, 30), 77, np.uint8)
    out, n = R.compute(img, img, max_disparity=16)
    assert n == 0 and not out.any()          # every cost ties: d* = 0 fails rule (a)


def test_shift_by_five_is_found_in_the_interior():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (24, 70)).astype(np.uint8)
    left, right = base[:, :64], base[:, 5:69]              # right(x) = left(x + 5): a left pixel x matches right x - 5
    out, _ = R.compute(left, right, max_disparity=16, subpixel=0)
    assert (out[:, 5 + 16:] == 5 * 256).all()
    sub, _ = R.compute(left, right, max_disparity=16, subpixel=1)
    assert (np.abs(sub[:, 5 + 16:] - 5 * 256) <= 128).all()


def test_a_two_way_tie_takes_the_lower_d():
    S = _volume(16)
    S[0, :, 3] = 100; S[0, :, 9] = 100
    out = R.select(S, 0, -1, 0)
    assert (out[0, 3:] == 3 * 256).all() and (out[0, :3] == 0).all()       # rule (b) at x < 3


@pytest.mark.parametrize("sm,sp,want", [(102, 100, 64), (100, 102, -64), (101, 100, 43), (100, 101, -43), (100, 100, 0), (355, 100, 127)])
def test_subpixel_offsets(sm, sp, want):
    # s0 = 99 at d = 7: num = 128 (sm - sp), den = sm + sp - 198.  (102, 100): 256 / 4 = 64; (101, 100): 128 / 3 = 42.67 -> 43;
    # (355, 100): 32640 / 257 = 127.0039 -> 127
    S = _volume(16)
    S[0, :, 6] = sm; S[0, :, 7] = 99; S[0, :, 8] = sp
    assert R.select(S, 0, -1, 1)[0, 20] == 7 * 256 + want
    assert R.select(S, 0, -1, 0)[0, 20] == 7 * 256


def test_subpixel_exactly_half_rounds_away_from_zero():
    # num / den = 1/2 exactly: S(d*-1) - S(d*+1) = 1 and den = 256
    S = _volume(16, fill=1000)
    S[0, :, 7] = 99
    S[0, :, 6] = 99 + 129; S[0, :, 8] = 99 + 127
    assert R.select(S, 0, -1, 1)[0, 20] == 7 * 256 + 1
    S[0, :, 6] = 99 + 127; S[0, :, 8] = 99 + 129
    assert R.select(S, 0, -1, 1)[0, 20] == 7 * 256 - 1
    # 3/2 exactly: difference 3, den = 256
    S[0, :, 6] = 99 + 126; S[0, :, 8] = 99 + 130
    assert R.select(S, 0, -1, 1)[0, 20] == 7 * 256 - 2


def test_den_not_positive_gives_no_offset():
    # At the LOWEST argmin S(d*-1) > s0 and S(d*+1) >= s0, so den >= 1: the rule is a guard.  Its edge is the plateau to the right of d*
    # (den = S(d*-1) - s0, here 1: the full +128) ...
    S = _volume(16, fill=99)
    S[0, :, 0] = 100
    assert R.select(S, 0, -1, 1)[0, 20] == 256 + 128
    # ... and volumes full of ties agree with the scalar transcription, guard included
    for trial in range(50):
        T = np.random.default_rng(trial).integers(90, 94, (1, 40, 16)).astype(np.uint16)
        for lr in (-1, 0):
            assert np.array_equal(R.select(T, 5, lr, 1), scalar_select(T.astype(int).tolist(), 40, 1, 16, 5, lr, 1))


def test_last_disparity_takes_no_offset():
    S = _volume(16)
    S[0, :, 15] = 10; S[0, :, 14] = 300
    out = R.select(S, 5, -1, 1)
    assert (out[0, 15:] == 15 * 256).all()


def test_uniqueness_without_a_far_candidate_passes():
    S = np.full((1, 8, 3), 50, np.uint16)                  # D = 3, d* = 1: no d with |d - d*| > 1
    S[0, :, 1] = 49
    out = R.select(S, 99, -1, 0)
    assert (out[0, 1:] == 256).all()
    S = np.full((1, 8, 4), 50, np.uint16)                  # D = 4: d = 3 is far and as good as s0 / 0.01
    S[0, :, 1] = 49
    assert not R.select(S, 99, -1, 0).any()


def test_left_right_check_rejects_an_occluded_match():
    S = _volume(16, W=30)
    S[0, :, 4] = 10                                        # everybody says 4 ...
    S[0, 20, 4] = 500; S[0, 20, 8] = 10                    # ... but pixel 20 says 8; its right pixel 12 is claimed by 16 at d = 4 as well
    out = R.select(S, 0, 0, 0)
    assert out[0, 20] == 0 and out[0, 19] == 4 * 256
    assert R.select(S, 0, -1, 0)[0, 20] == 8 * 256


# ---- ground-truth recovery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("H,W,D,seed", [(40, 96, 32, 1), (48, 160, 64, 2), (37, 131, 48, 3)])
def test_recovers_the_truth_of_a_built_scene(H, W, D, seed, paths):
    left, right, gt, visible = R.scene(H, W, D, seed)
    out, n = R.compute(left, right, max_disparity=D, p1=10, p2=120, paths=paths, uniqueness=5, lr_max_diff=1, subpixel=1)
    share = R.recovery(out, gt, visible)
    print(f"{H}x{W} D {D} paths {paths}: {share:.4f} of {int(visible.sum())} visible pixels recovered, {n} valid")
    assert share >= 0.90
