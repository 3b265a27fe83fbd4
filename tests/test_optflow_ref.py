"""CPU: the NumPy restatement of the dense optical-flow contract (tests/optflow_ref.py) checked on its own - the census against the stereo
restatement's, the pyramid and the candidate ranking by hand, the degenerate sizes, and the accuracy conditions the contract was accepted on.
tests/test_optflow_gpu.py compares the device with this restatement array_equal, so the device inherits what is shown here."""
import functools

import numpy as np
import pytest

from tests import optflow_ref as R
from tests import stereo_ref as SR


def test_census_is_the_stereo_census():
    rng = np.random.default_rng(1)
    for H, W in ((1, 1), (5, 7), (7, 9), (23, 41)):
        img = rng.integers(0, 256, (H, W)).astype(np.uint8)
        img[rng.integers(0, H, 3), rng.integers(0, W, 3)] = img[0, 0]          # equal values: "<" is strict
        assert np.array_equal(R.census(img), SR.census(img)), (H, W)


def test_pyramid_by_hand():
    a = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 250]], np.uint8)
    # 3 x 3 -> 2 x 2: (1 + 2 + 4 + 5 + 2) >> 2 = 3; the right column pairs 3, 6 with themselves: (3 + 3 + 6 + 6 + 2) >> 2 = 5;
    # the bottom row 7, 8 twice: (7 + 8 + 7 + 8 + 2) >> 2 = 8; the corner 250 four times: 1002 >> 2 = 250
    assert R.downsample(a).tolist() == [[3, 5], [8, 250]]
    b = np.array([[0, 1, 2, 3, 255], [4, 5, 6, 8, 255]], np.uint8)
    # 5 x 2 (W x H) -> 3 x 1: (0 + 1 + 4 + 5 + 2) >> 2 = 3, (2 + 3 + 6 + 8 + 2) >> 2 = 5, (255 * 4 + 2) >> 2 = 255
    assert R.downsample(b).tolist() == [[3, 5, 255]]
    assert R.level_sizes(5, 2, 4) == [(5, 2), (3, 1), (2, 1), (1, 1)]
    assert R.level_sizes(3, 3, 3) == [(3, 3), (2, 2), (1, 1)]
    p = R.pyramid(a, 3)
    assert [x.shape for x in p] == [(3, 3), (2, 2), (1, 1)] and p[2].tolist() == [[(3 + 5 + 8 + 250 + 2) >> 2]]
    assert R.downsample(np.array([[1, 2]], np.uint8)).tolist() == [[(1 + 2 + 1 + 2 + 2) >> 2]]


def test_candidate_ranking():
    # r = 1, ascending (du^2 + dv^2, dv, du): the centre, then the four at distance 1 by dv then du, then the four corners
    assert R.candidates(1) == [(0, 0), (0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]
    for r in (1, 2, 3, 4):
        c = R.candidates(r)
        assert len(c) == len(set(c)) == (2 * r + 1) ** 2 and c[0] == (0, 0)
        assert c[-1] == (r, r)


def test_constant_pair_gives_zero_flow():
    img = np.full((13, 21), 99, np.uint8)
    for prm in (dict(), dict(levels=3, radius=4, window=0), dict(levels=1, fb_max_diff=0)):
        s = R.stages(img, img, **prm)
        assert not s["flow"].any() and s["valid"].all() and s["n_valid"] == 13 * 21
        assert all(not f.any() for f in s["forward"]) and all(not f.any() for f in s["backward"])


def test_one_pixel_images_at_seven_levels():
    a, b = np.array([[3]], np.uint8), np.array([[200]], np.uint8)
    s = R.stages(a, b, levels=7)
    assert [x.shape for x in s["pyramid0"]] == [(1, 1)] * 7 and all(x[0, 0] == 200 for x in s["pyramid1"])
    assert s["flow"].shape == (1, 1, 2) and not s["flow"].any() and s["n_valid"] == 1
    assert len(s["forward"]) == 7 and all(f.shape == (1, 1, 2) for f in s["forward"])


def test_median_and_ties_by_hand():
    F = np.zeros((3, 3, 2), np.int32)
    F[1, 1] = (9, -9); F[0, 0] = (5, 5)
    M = R.median3(F)
    assert not M[1, 1].any()                                 # one outlier among nine
    # the corner's clamped neighbourhood: (0, 0) four times, (0, 1) and (1, 0) twice each, (1, 1) once: u = 0 0 0 0 5 5 5 5 9, v = -9 0 0 0 0 5 5 5 5
    assert M[0, 0].tolist() == [5, 0]
    F[0, 1] = (5, 5)
    assert R.median3(F)[0, 0].tolist() == [5, 5]             # now six of nine in both components


def test_fb_off_runs_nothing_backward():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 256, (9, 12)).astype(np.uint8), rng.integers(0, 256, (9, 12)).astype(np.uint8)
    s = R.stages(a, b, levels=2, fb_max_diff=-1)
    assert s["backward"] is None and s["valid"].all() and s["n_valid"] == 9 * 12
    t = R.stages(a, b, levels=2, fb_max_diff=0)
    assert np.array_equal(s["flow"], t["flow"]) and t["n_valid"] < 9 * 12          # the flow is written for every pixel, valid or not


# ---- Condition A: integer shifts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx,dy,L", [(0, 0, 1), (3, -2, 3), (9, 5, 3), (-13, 7, 4)])
def test_condition_a_integer_shifts(dx, dy, L):
    I0, I1 = R.shifted_pair(dx, dy)
    s = R.stages(I0, I1, levels=L, radius=2, window=2, median=1, fb_max_diff=-1)
    F = s["forward"][0][16:-16, 16:-16]
    share = float(((F[..., 0] == dx) & (F[..., 1] == dy)).mean())
    print(f"shift ({dx}, {dy}) L {L}: exact share {share:.4f}")
    assert share >= 0.99


# ---- Condition B: two motions --------------------------------------------------------------------------------------------------------
CASES = {"i": ((2.5, -1.25), (2.5, -1.25)), "ii": ((-1, 0), (6, 2)), "iii": ((5.5, 3), (-4, 1))}


@functools.lru_cache(maxsize=None)
def _two_motion(case, seed, subpixel):
    I0, I1, truth = R.two_motion_pair(seed, *CASES[case])
    s = R.stages(I0, I1, levels=3, radius=2, window=2, median=1, fb_max_diff=1, subpixel=subpixel)
    err = np.abs(s["flow"].astype(np.float64) - truth).max(axis=-1)
    valid = s["valid"].astype(bool)
    return float(valid.mean()), float((err[valid] <= 1.0).mean()), float(err[valid].mean())


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("case,min_valid,min_good", [("i", 0.90, 0.99), ("ii", 0.75, 0.93), ("iii", 0.75, 0.93)])
def test_condition_b_two_motions(case, min_valid, min_good, seed):
    share, good, mean_err = _two_motion(case, seed, 1)
    print(f"case ({case}) seed {seed}: valid share {share:.4f}, within 1 px {good:.4f}, mean error {mean_err:.4f}")
    assert share >= min_valid
    assert good >= min_good


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_condition_b_subpixel_ratio(seed):
    _, _, with_sub = _two_motion("i", seed, 1)
    _, _, without = _two_motion("i", seed, 0)
    print(f"seed {seed}: mean error {with_sub:.4f} with sub-pixel, {without:.4f} without")
    assert with_sub <= 0.6 * without
