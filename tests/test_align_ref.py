"""CPU: the NumPy restatement of the aligner's contract (tests/align_ref.py) against cases worked by hand, the exact sum, numpy.linalg.solve and a
matrix exponential by series, degenerate systems, and the accuracy of a solve in the inside corner of a room; then the library's host step
(vdo_align_step needs no device) against the restatement's."""
import math

import numpy as np
import pytest

from tests import align_ref as A

F = np.float32
I4 = np.eye(4, dtype=F)


def _sums_dict(sums):
    d = {f"A{r}{c}": sums[t] for t, (r, c) in enumerate(A.UPPER)}
    d.update({f"b{r}": sums[21 + r] for r in range(6)})
    d["chi2"] = sums[27]
    return d


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------------
def test_one_pixel_by_hand():
    """K = (1, 1, 0, 0), T = Tm = I.  Pixel (0, 0) at depth 2: Pc = Pw = (0, 0, 2); it projects to model pixel (0, 0), whose depth 1.5 and gradient
    (0, 0, -2) give Vm = (0, 0, 1.5), del = (0, 0, 0.5), e = -1, gg = 4, w = 1/4, J = (0, 0, -2, -0, 0, 0): A22 = (-0.5)(-2) = 1, b2 = (-0.5)(-1) = 0.5,
    chi2 = (-0.25)(-1) = 0.25 - the squared point-to-plane distance 0.5^2."""
    K1 = (1.0, 1.0, 0.0, 0.0)
    sums, counts, rw = A.linearise(np.array([[2.0]], F), None, K1, I4, np.array([[1.5]], F), np.array([[[0.0, 0.0, -2.0]]], F), K1, I4, 0.0, 10.0, 1.0)
    assert counts.tolist() == [1, 0, 0, 0, 0]
    assert rw[0, 0].tolist() == [0.0, 0.0, -2.0, 0.0, 0.0, 0.0, -1.0, 0.25] and math.copysign(1.0, rw[0, 0, 3]) == -1.0      # J3 = 0*(-2) - 2*0 = -0.0
    want = dict.fromkeys(_sums_dict(sums), 0.0); want.update(A22=1.0, b2=0.5, chi2=0.25)
    assert _sums_dict(sums) == want
    assert not np.signbit(sums).any()                                        # a -0.0 term meets the +0.0 of an empty slot in the first level
    status, Tn, xi, rms = A.step(sums, 1, 1, I4)
    assert status == 2 and rms == 0.5 and np.array_equal(Tn, I4)             # one row: five motions unconstrained


def test_two_pixels_by_hand():
    """The same with a second pixel (1, 0) at depth 2: dx = 1, Pc = Pw = (2, 0, 2), model pixel (1, 0) with depth 1 and gradient (-1, 0, -1): r = (1, 0, 1),
    Vm = (1, 0, 1), del = (1, 0, 1), dist2 = 2, e = -2, gg = 2, w = 1/2, J = (-1, 0, -1, -0, 2*(-1) - 2*(-1) = 0, 0), h = (-1/2, 0, -1/2, ..):
    A00 = A02 = 1/2, A22 = 1 + 1/2, b0 = 1, b2 = 1/2 + 1, chi2 = 1/4 + 2.  Then the skips, each through its count."""
    K1 = (1.0, 1.0, 0.0, 0.0)
    D = np.array([[2.0, 2.0]], F); Dm = np.array([[1.5, 1.0]], F); Gm = np.array([[[0.0, 0.0, -2.0], [-1.0, 0.0, -1.0]]], F)
    sums, counts, rw = A.linearise(D, None, K1, I4, Dm, Gm, K1, I4, 0.0, 10.0, 2.0)
    assert counts.tolist() == [2, 0, 0, 0, 0]
    assert rw[0, 1].tolist() == [-1.0, 0.0, -1.0, 0.0, 0.0, 0.0, -2.0, 0.5]
    want = dict.fromkeys(_sums_dict(sums), 0.0); want.update(A00=0.5, A02=0.5, A22=1.5, b0=1.0, b2=1.5, chi2=2.25)
    assert _sums_dict(sums) == want
    # the far gate exactly at max_dist: pixel 0 has dist2 = 0.25 = 0.5 * 0.5 and is used; one float below 0.5 it is far (pixel 1, dist2 = 2, is far in both)
    assert A.linearise(D, None, K1, I4, Dm, Gm, K1, I4, 0.0, 10.0, 0.5)[1].tolist() == [1, 0, 0, 0, 1]
    below = float(np.nextafter(F(0.5), F(0)))
    assert A.linearise(D, None, K1, I4, Dm, Gm, K1, I4, 0.0, 10.0, below)[1].tolist() == [0, 0, 0, 0, 2]
    # the mask, a hole in the model, a zero gradient, a depth out of range: each through its count
    assert A.linearise(D, np.array([[0, 7]], np.int32), K1, I4, Dm, Gm, K1, I4, 0.0, 10.0, 2.0)[1].tolist() == [1, 0, 1, 0, 0]
    assert A.linearise(D, None, K1, I4, np.array([[1.5, 0.0]], F), Gm, K1, I4, 0.0, 10.0, 2.0)[1].tolist() == [1, 0, 0, 1, 0]
    assert A.linearise(D, None, K1, I4, Dm, np.zeros((1, 2, 3), F), K1, I4, 0.0, 10.0, 2.0)[1].tolist() == [0, 0, 0, 2, 0]
    assert A.linearise(np.array([[np.nan, 11.0]], F), None, K1, I4, Dm, Gm, K1, I4, 0.0, 10.0, 2.0)[1].tolist() == [0, 2, 0, 0, 0]


def test_slots_and_the_tree_written_out():
    """A 9 x 9 grid: 2 x 2 tiles, 256 slots; sample (8, 8) is alone in tile 3 at slot 192; the tree of 1 .. 81 at their slots is their exact sum"""
    t = np.arange(1.0, 82.0).reshape(9, 9, 1)
    v = A.slot_vector(t)
    assert v.shape == (256, 1) and v[192, 0] == 81.0 and v[0, 0] == 1.0 and v[9, 0] == 11.0 and v[64, 0] == 9.0 and v[128, 0] == 73.0 and v[193:].sum() == 0
    assert A.pair_tree(v)[0] == 81 * 82 / 2
    assert A.slot_vector(np.ones((8, 24, 1))).shape[0] == 256 and A.slot_vector(np.ones((1, 1, 1))).shape[0] == 64      # 3 tiles pad to 4


# ---- a random scene: the tree against the exact sum, the counts ------------------------------------------------------------------------------------
def _random_scene(seed, W=37, H=29, Wm=41, Hm=23):
    rng = np.random.default_rng(seed)
    D = rng.uniform(1.0, 6.0, (H, W)).astype(F)
    D[rng.random((H, W)) < 0.05] = 0.0
    mask = (rng.random((H, W)) < 0.1).astype(np.int32) * 3
    Dm = rng.uniform(1.0, 6.0, (Hm, Wm)).astype(F); Dm[rng.random((Hm, Wm)) < 0.1] = 0.0
    Gm = rng.normal(0, 3000, (Hm, Wm, 3)).astype(F); Gm[rng.random((Hm, Wm)) < 0.1] = 0.0
    K4 = (30.0, 28.0, 18.2, 14.1); Km = (25.0, 26.0, 20.5, 11.0)
    T = A.perturbed(I4, (0.1, -0.05, 0.02), (1.0, 2.0, -1.5)); Tm = A.perturbed(I4, (-0.2, 0.1, 0.0), (-3.0, 1.0, 0.5))
    return D, mask, K4, T, Dm, Gm, Km, Tm


@pytest.mark.parametrize("s", [1, 2, 3])
def test_every_tree_sum_is_within_its_bound_of_the_exact_sum_and_the_counts_add_up(s):
    """A pair tree over N = 2^L values has L levels; each addition's relative error is at most 2^-53, so the sum is off by at most
    L * 2^-53 * sum|term| (to first order), far inside the N * 2^-52 * sum|term| asserted here."""
    D, mask, K4, T, Dm, Gm, Km, Tm = _random_scene(5 + s)
    rw, cls = A.rows(D, mask, K4, T, Dm, Gm, Km, Tm, 0.5, 5.5, 3.0, s)
    sums, counts, _ = A.linearise(D, mask, K4, T, Dm, Gm, Km, Tm, 0.5, 5.5, 3.0, s)
    Ws, Hs = A.grid(37, 29, s)
    assert counts.sum() == Ws * Hs and (counts > 0).all(), counts
    t = A.terms(rw).reshape(-1, 28)
    N = A.slot_vector(A.terms(rw)).shape[0]
    for k in range(28):
        exact = math.fsum(t[:, k].tolist())
        assert abs(sums[k] - exact) <= N * 2.0 ** -52 * math.fsum(np.abs(t[:, k]).tolist()), k
    assert (t[cls.ravel() != A.USED] == 0).all() and not np.signbit(t[cls.ravel() != A.USED]).any()      # a skipped sample contributes +0.0


# ---- the step ----------------------------------------------------------------------------------------------------------------------------------
def _expm_series(M):
    out = np.eye(4); term = np.eye(4)
    for k in range(1, 40):
        term = term @ M / k
        out = out + term
    return out


def _twist(xi):
    v, w = xi[:3], xi[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = v
    return M


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e-6])
def test_the_step_against_linalg_solve_and_a_series_exponential(scale):
    rng = np.random.default_rng(11)
    Jm = rng.normal(0, 1, (200, 6)); e = rng.normal(0, scale, 200); w = rng.uniform(0.5, 2.0, 200)
    Amat = (Jm * w[:, None]).T @ Jm; b = (Jm * w[:, None]).T @ e
    sums = np.array([Amat[r, c] for r, c in A.UPPER] + b.tolist() + [float((w * e * e).sum())])
    T = A.perturbed(I4, (3.0, -2.0, 100.0), (20.0, -30.0, 45.0))
    status, Tn, xi, rms = A.step(sums, 200, 6, T)
    assert status == 0 and rms == pytest.approx(math.sqrt((w * e * e).sum() / 200), rel=1e-14)
    want = np.linalg.solve(Amat, -b)
    assert np.allclose(xi, want, rtol=1e-9, atol=0)
    Tw = _expm_series(_twist(-want)) @ T.astype(np.float64)
    assert np.abs(Tn.astype(np.float64) - Tw)[:3].max() <= 2.0 ** -23 * np.abs(Tw[:3]).max()
    assert Tn[3].tolist() == [0, 0, 0, 1]
    for xi_t in ([1e-7, 0, 0, 0, 0, 3e-5], [0.1, -0.2, 0.3, 0, 0, 0], [0.1, 0.2, 0.3, 1.5, -2.0, 0.7]):      # the series branch, a pure translation, a large turn
        assert np.allclose(A.exp_se3(np.array(xi_t)), _expm_series(_twist(np.array(xi_t))), rtol=0, atol=1e-14)


def _plane_model(normal, d, W, H, K4):
    """A synthetic model at Tm = I: the plane n . p = d seen exactly, with the constant gradient -n * 1000 (towards the camera)"""
    Dm = A.plane_depth([(normal, d)], I4, W, H, K4)
    Gm = np.broadcast_to((-1000.0 * np.asarray(normal)).astype(F), (H, W, 3)).copy()
    return Dm, Gm


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (0.6, 0.0, 0.8)], ids=["fronto", "tilted"])
def test_a_single_plane_is_degenerate_and_leaves_T_untouched(normal):
    """Both planes have a gradient without a y component, at Tm = I: the y column of J is exactly zero and so is its pivot.  (A plane oblique to all
    three axes is degenerate only up to the rounding of the fp32 rows, about 4e-8 of the diagonal entry with either sign: the contract's plain
    'pivot not positive' cannot promise status 2 there, and no such case is asserted.)"""
    W, H, K4 = 24, 16, (20.0, 20.0, 11.5, 7.5)
    Dm, Gm = _plane_model(normal, 3.0, W, H, K4)
    T = A.perturbed(I4, (0.0, 0.0, 0.03), (0.0, 0.0, 0.0))
    D = A.plane_depth([(normal, 3.0)], I4, W, H, K4)
    sums, counts, _ = A.linearise(D, None, K4, T, Dm, Gm, K4, I4, 0.0, 10.0, 0.5)
    assert counts[0] > W * H // 2
    status, Tn, xi, rms = A.step(sums, int(counts[0]), 6, T)
    assert status == 2 and np.array_equal(Tn.view(np.uint32), T.view(np.uint32)) and not xi.any() and rms > 0
    Tn, rep, trace = A.solve(D, None, K4, T, Dm, Gm, K4, I4, 0.0, 10.0, 0.5, 1, 6, 5, 1e-6)
    assert rep["status"] == 2 and rep["iterations"] == 1 and np.array_equal(Tn, T)


def test_fewer_samples_than_min_pixels_is_status_1_and_leaves_T_untouched():
    c = A.CORNER
    D, T_true, T_init, Dm, Gm = A.corner_case(0)
    few = np.zeros_like(D); few[10:12, 20:25] = D[10:12, 20:25]
    Tn, rep, trace = A.solve(few, None, c["K4"], T_init, Dm, Gm, c["K4"], T_init, 0.0, c["max_depth"], c["max_dist"], 1, 11, c["max_iterations"], c["eps"])
    assert rep["status"] == 1 and rep["iterations"] == 1 and rep["used"] == 10 and np.array_equal(Tn.view(np.uint32), T_init.view(np.uint32)) and not rep["xi"].any()
    Tn, rep, trace = A.solve(np.zeros_like(D), None, c["K4"], T_init, Dm, Gm, c["K4"], T_init, 0.0, c["max_depth"], c["max_dist"], 1, 6, c["max_iterations"], c["eps"])
    assert rep["status"] == 1 and rep["used"] == 0 and rep["rms_first"] == 0.0 and not trace[0][1].any() and not np.signbit(trace[0][1]).any() and np.array_equal(Tn, T_init)
    nan_T = T_init.copy(); nan_T[1, 2] = np.nan
    sums, counts, _ = A.linearise(D, None, c["K4"], nan_T, Dm, Gm, c["K4"], T_init, 0.0, c["max_depth"], c["max_dist"])
    assert counts[0] == 0 and not sums.any()


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------------------
# What the restatement reaches from each of align_ref.PERTURBATIONS (5 cm and 2 degrees): (camera-centre error in metres, rotation error in degrees)
CORNER_MEASURED = [(0.00202, 0.0461), (0.00149, 0.0306), (0.00166, 0.0368), (0.00111, 0.0134), (0.00056, 0.0447)]


def check_corner(k, T, rep, trace, T_true, T_init):
    """The accuracy condition, shared with the device test"""
    c = A.CORNER
    assert rep["status"] == 0 and rep["iterations"] < c["max_iterations"], rep
    assert rep["rms_last"] < rep["rms_first"]
    for it_T, sums, counts in trace:
        assert counts[0] * 4 >= c["W"] * c["H"], counts
    dt0, dr0 = A.pose_error(T_init, T_true)
    dt, dr = A.pose_error(T, T_true)
    print(f"corner {k}: from {dt0 * 1e3:.1f} mm, {dr0:.3f} deg to {dt * 1e3:.2f} mm, {dr:.4f} deg in {rep['iterations']} iterations, rms {rep['rms_first'] * 1e3:.1f} -> {rep['rms_last'] * 1e3:.2f} mm")
    assert dt < 0.5 * dt0 and dr < 0.5 * dr0
    assert dt <= 1.5 * CORNER_MEASURED[k][0] and dr <= 1.5 * CORNER_MEASURED[k][1], (dt, dr)


@pytest.mark.parametrize("k", range(len(A.PERTURBATIONS)))
def test_a_solve_in_a_room_corner_recovers_the_pose(k):
    """The inside corner of a room (x = 2, y = 1.5, z = 4 m) fused from four poses at 100 mm voxels (dense_ref), the model rendered at the perturbed pose
    (raycast_ref), a 64 x 48 frame measured at the true pose.  From 50 mm and 2 degrees the restatement stops by eps after 4-5 iterations with
    status 0, the RMS point-to-plane distance falling from 32-80 mm to 5.5-5.9 mm, at (mm, degrees) 2.02, 0.046 | 1.49, 0.031 | 1.66, 0.037 | 1.11, 0.013 |
    0.56, 0.045; 91-97 % of the samples are used, cond(A) is 90-99.  Asserted: those figures times 1.5 (the restatement is deterministic; the margin is
    for edits of the fixture), below half the perturbation, and at least a quarter of the samples used."""
    c = A.CORNER
    D, T_true, T_init, Dm, Gm = A.corner_case(k)
    T, rep, trace = A.solve(D, None, c["K4"], T_init, Dm, Gm, c["K4"], T_init, 0.0, c["max_depth"], c["max_dist"], 1, c["W"] * c["H"] // 16, c["max_iterations"], c["eps"])
    check_corner(k, T, rep, trace, T_true, T_init)


# ---- the library's host step ----------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a = np.asarray(a, F).ravel(); b = np.asarray(b, F).ravel()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


def test_vdo_align_step_equals_the_restatement_without_a_device():
    from vdo_slam_amd import align as AL
    c = A.CORNER
    D, T_true, T_init, Dm, Gm = A.corner_case(3)
    sums, counts, _ = A.linearise(D, None, c["K4"], T_init, Dm, Gm, c["K4"], T_init, 0.0, c["max_depth"], c["max_dist"])
    want = A.step(sums, int(counts[0]), 6, T_init)
    got = AL.step(sums, int(counts[0]), 6, T_init)
    assert got[0] == want[0] == 0 and _ulps(got[1], want[1]) <= 1 and np.allclose(got[2], want[2], rtol=1e-12, atol=1e-18) and got[3] == pytest.approx(want[3], rel=1e-15)
    for sm, used, min_px, status in [(sums, 5, 6, 1), (np.where(np.arange(28) == 3, np.nan, sums), 100, 6, 2), (np.where(np.arange(28) == 0, 0.0, sums), 100, 6, 2),
                                     (np.zeros(28), 0, 6, 1), (np.where(np.arange(28) == 20, -1.0, sums), 100, 6, 2)]:
        got = AL.step(sm, used, min_px, T_init); want = A.step(sm, used, min_px, T_init)
        assert got[0] == want[0] == status and np.array_equal(got[1].view(np.uint32), T_init.view(np.uint32)) and not got[2].any()
    L = AL._lib()
    T16 = np.ascontiguousarray(T_init.reshape(16)); out = np.full(16, -7.0, F)
    assert L.vdo_align_step(None, 10, 6, T16.ctypes.data, out.ctypes.data, None, None) == -1
    assert L.vdo_align_step(sums.ctypes.data, 10, 6, None, out.ctypes.data, None, None) == -1
    assert L.vdo_align_step(sums.ctypes.data, 10, 6, T16.ctypes.data, None, None, None) == -1 and (out == -7).all()
    assert L.vdo_align_step(sums.ctypes.data, int(counts[0]), 6, T16.ctypes.data, out.ctypes.data, None, None) == 0 and _ulps(out.reshape(4, 4), want_T(sums, counts, T_init)) <= 1


def want_T(sums, counts, T):
    return A.step(sums, int(counts[0]), 6, T)[1]
