"""The Tracking-side image kernels across sizes and edge cases: K11 / mask_at (k_gather modes 0, 1, 2), RenewFrameInfo static
(k_renew_pred, k_carry_select, k_near_flags_sel) and objects (k_renew_obj_pred / k_renew_obj_all), the single-label warp and
UpdateMask (k_warp_candidates, k_votes_par, k_apply_warps; k_label_vote + k_mask_warp_if beyond 64 labels), and the object chain.
Bit for bit against the CPU oracle's sequential walks (and the NumPy restatements of tests/image_kernels_ref.py where they exist);
the inputs are built so that the counts that matter - valid candidates, recovered labels, label slots, which path runs - are known
in advance and asserted."""
import numpy as np
import pytest

from tests import image_kernels_ref as N
from tests import tracking_ref as T
from vdo_slam_amd import _capi as K
from vdo_slam_amd.synth import KITTI_K
from vdo_slam_amd.synth_frames import TH_DEPTH_OBJ

gpu = pytest.mark.gpu
K4 = np.array(KITTI_K, np.float32)
TWC = np.eye(4, dtype=np.float32); TWC[:3, 3] = (0.3, -0.1, 2.0); TWC[0, 1], TWC[1, 0] = -0.02, 0.02
ONE_PASS_SLOTS = 64                      # label slots of k_votes_par (one bit each); more labels run label after label
GATHER_SIZES = [(1, 1), (3, 3), (17, 9), (256, 2), (1242, 375)]
GATHER_N = [1, 255, 256, 257]
RENEW_STATIC = [(1023, 255), (1024, 256), (1025, 257), (2049, 513)]
RENEW_OBJECT = [(255, 257), (256, 255), (257, 256), (256, None)]


@pytest.fixture(scope="module")
def ctx():
    from vdo_slam_amd.ba import Context
    c = Context(0)
    yield c
    c.close()


def _images(ctx, depth, flow, mask):
    from vdo_slam_amd.frontend import FrameImages
    h, w = mask.shape
    im = FrameImages(ctx, w, h)
    im.upload(depth, flow, mask)
    return im


def _same(got, exp, what=""):
    for k in exp:
        assert got[k].shape == exp[k].shape and got[k].tobytes() == exp[k].tobytes(), f"{what}: {k}"


def _max_nums(case):
    v = case["n_valid"]
    return [0, 1, v - 1, v, v + 1, v + 40, v + case["orb_x"].size]


def _keys(d, sel=None):
    kx, ky = (d["key_x"], d["key_y"]) if sel is None else (d["key_x"][sel], d["key_y"][sel])
    return set(zip(kx.tolist(), ky.tolist()))


def _scenes():
    """(name, scene, recovered slots, one-pass?) of block 8"""
    out = []
    for w, n, slots in ((255, 1, (0,)), (256, 63, (0, 31, 62)), (257, 64, (0, 32, 63)), (400, 65, (0, 32, 64))):
        for r in slots:
            sc, rec = N.scene_plain(w, n, r)
            out.append((f"{n} labels, slot {r} missing", sc, rec))
    sc, rec = N.scene_top_slot_after_recovery(400)
    out.append(("64 labels, slot 63 after slot 10", sc, rec))
    for w, n, abc in ((400, 8, (1, 3, 6)), (257, 64, (10, 40, 63)), (400, 65, (10, 40, 63))):
        sc, rec = N.scene_cascade(w, n, *abc)
        out.append((f"cascade, {n} labels", sc, rec))
    for n in (6, 64, 65):
        sc, rec = N.scene_votes(400, n)
        out.append((f"vote thresholds, {n} labels", sc, rec))
    return [(name, sc, rec, sc.n <= ONE_PASS_SLOTS) for name, sc, rec in out]


# =============================================================================================================================
# without a GPU: the NumPy restatements and the constructions against the oracle
# =============================================================================================================================
def test_numpy_gather_and_warp_equal_the_oracle(oracle):
    for w, h in GATHER_SIZES:
        mask, depth = N.gather_images(w, h)
        for n in GATHER_N + [400]:
            kx, ky = N.gather_points(w, h, n)
            assert np.array_equal(N.gather(0, kx, ky, depth, mask), T.propagate_static(oracle, kx, ky, depth)), (w, h, n)
            d, lab = N.gather(1, kx, ky, depth, mask, TH_DEPTH_OBJ)
            d_o, lab_o = T.propagate_object(oracle, kx, ky, depth, mask, TH_DEPTH_OBJ)
            assert np.array_equal(d, d_o) and np.array_equal(lab, lab_o), (w, h, n)
            assert np.array_equal(N.gather(2, kx, ky, depth, mask), T.mask_at(oracle, kx, ky, mask)), (w, h, n)
    for w in (255, 256, 257, 400):
        last, flow, cur, must, must_not = N.warp_case(w)
        out = N.mask_warp(last, flow, 4, cur)
        assert np.array_equal(out, T.mask_warp(oracle, last, flow, 4, cur))
        assert all(out[p] == 4 for p in must) and all(out[p] == 6 for p in must_not) and (out == 4).sum() > 500


def test_gather_bounds_differ_between_the_modes():
    """u == w-1 (and v == h-1) is inside for the label gather of UpdateMask (u < w) and outside for K11 (u < w-1)."""
    mask, depth = N.gather_images(17, 9)
    depth[:] = 5.0
    kx = np.array([16.999, 15.5, 8.0, 8.0, 0.999, 17.0], np.float32); ky = np.array([4.0, 4.0, 8.999, 7.5, 4.0, 4.0], np.float32)
    assert (N.gather(2, kx, ky, depth, mask) != -1).tolist() == [True, True, True, True, False, False]
    assert (N.gather(0, kx, ky, depth, mask) != -1).tolist() == [False, True, False, True, False, False]
    assert (N.gather(1, kx, ky, depth, mask)[1] != 0).tolist() == [False, True, False, True, False, False]


def test_renew_cases_do_what_they_say_in_the_oracle(oracle):
    for n1, n_orb in RENEW_STATIC:
        c = N.renew_static_case(n1, n_orb)
        assert (c["tm"] != -1).sum() == n1
        for m in _max_nums(c):
            e = T.renew_static(oracle, c["tm"], c["stat_x"], c["stat_y"], c["orb_x"], c["orb_y"], c["mask"], c["depth"], c["flow"], m)
            assert ((e["inlier_id"] >= 0).sum(), (e["inlier_id"] < 0).sum()) == N.renew_static_expected(c, m), (n1, m)
        _check_static_pairs(c, e)
    for nc0, n_tmp in RENEW_OBJECT:
        c = N.renew_object_case(nc0, n_tmp)
        for m in (c["n_valid0"] - 1, c["n_valid0"], c["n_valid0"] + 1, 100000):
            e = T.renew_object(oracle, c["inl"], c["stat"], c["sem_pos"], c["mod"], c["cur_x"], c["cur_y"], c["col"], c["tmp"], c["mask"], c["depth"], c["flow"], m)
            _check_object_counts(c, e, m)


def _check_static_pairs(c, e):
    """(after the walk with the largest limit) every keypoint exactly 1 px from a host is in the new set, none of the ones 1 - 2^-20 px
    away is, and the one beside the INVALID carried candidate is"""
    keys = _keys(e, e["inlier_id"] < 0)
    ox, oy = c["orb_x"], c["orb_y"]
    assert all((float(ox[i]), float(oy[i])) in keys for i in c["at_one"])
    assert not any((float(ox[i]), float(oy[i])) in keys for i in c["near"])
    assert (float(ox[c["beside_invalid"]]), float(oy[c["beside_invalid"]])) in keys


def _check_object_counts(c, e, m):
    carried = e["inlier_id"] >= 0
    assert carried.sum() == c["n_valid0"] + c["n_valid2"]
    top0 = (~carried & (e["obj_label"] == 11)).sum()
    assert top0 == (0 if m <= c["n_valid0"] else 1 if m == c["n_valid0"] + 1 else top0) and (m < 100000 or top0 > 100)
    assert (e["obj_label"] == -2).sum() == (c["tmp"]["label"] == 3).sum() > 0
    if m == 100000:
        keys = _keys(e, ~carried)
        assert (60.0, 12.0) not in keys and (64.0, 12.0) in keys and (24.0, 8.0) in keys      # on a carried key / exactly 1 px from one (twice)


def test_update_mask_scenes_do_what_they_say_in_the_oracle(oracle):
    for name, sc, rec, one_pass in _scenes():
        assert np.unique(sc.sl).size == sc.n and one_pass == (sc.n <= 64), name
        out, n = T.update_mask(oracle, *sc.samples(), sc.last, sc.flow, sc.cur)
        assert sc.recovered(out) == rec and n == len(rec), name
    _check_cascade_subproblems(oracle)


def _check_cascade_subproblems(oracle):
    """every step of the cascade would decide the other way alone"""
    for w, n, (a, b, c) in ((400, 8, (1, 3, 6)), (257, 64, (10, 40, 63))):
        sc, rec = N.scene_cascade(w, n, a, b, c)
        run = lambda slots: sc.recovered(T.update_mask(oracle, *sc.samples(slots), sc.last, sc.flow, sc.cur)[0])
        assert run([b]) == set() and run([a, b]) == {a, b}                    # b needs a
        assert run([c]) == {c} and run([a, c]) == {a, c} and run([b, c]) == {c}      # c alone / after a: recovered; (b alone is not, so c still is)
        assert run([a, b, c]) == {a, b} == rec                                # after b: not
    sc, rec = N.scene_top_slot_after_recovery(400)
    run = lambda slots: sc.recovered(T.update_mask(oracle, *sc.samples(slots), sc.last, sc.flow, sc.cur)[0])
    assert run([63]) == set() and run([10, 63]) == {10, 63} == rec


# =============================================================================================================================
# 5. K11 / mask_at
# =============================================================================================================================
@gpu
@pytest.mark.parametrize("w,h", GATHER_SIZES)
def test_gathers_at_every_bound(ctx, oracle, w, h):
    from vdo_slam_amd import tracking as TR
    mask, depth = N.gather_images(w, h)
    im = _images(ctx, depth, np.zeros((h, w, 2), np.float32), mask)
    for n in GATHER_N:
        kx, ky = N.gather_points(w, h, n)
        e0 = N.gather(0, kx, ky, depth, mask)
        e1 = N.gather(1, kx, ky, depth, mask, TH_DEPTH_OBJ)
        e2 = N.gather(2, kx, ky, depth, mask)
        assert np.array_equal(e0, T.propagate_static(oracle, kx, ky, depth)) and np.array_equal(e2, T.mask_at(oracle, kx, ky, mask))
        o1 = T.propagate_object(oracle, kx, ky, depth, mask, TH_DEPTH_OBJ)
        assert np.array_equal(e1[0], o1[0]) and np.array_equal(e1[1], o1[1])
        assert np.array_equal(TR.propagate_static(im, kx, ky), e0), (n, "mode 0")
        d, lab = TR.propagate_object(im, kx, ky, TH_DEPTH_OBJ)
        assert np.array_equal(d, e1[0]) and np.array_equal(lab, e1[1]), (n, "mode 1")
        assert np.array_equal(TR.mask_at(im, kx, ky), e2), (n, "mode 2")
        if n == 257 and w >= 3 and h >= 3:
            # the cases sit where they say: some positions inside for the label gather only (u == w-1 or v == h-1), depth exactly th seen
            assert ((e2 != -1) & (e1[1] == 0)).sum() > 0 and (e2 != -1).sum() > 0 and (e2 == -1).sum() > 0
        if n == 257 and w == 1242:
            assert (e0 > 0).sum() > 50 and (e0 == -1).sum() > 50 and (e1[1] != 0).sum() > 50
    im.close()


# =============================================================================================================================
# 6. RenewFrameInfo, static
# =============================================================================================================================
@gpu
@pytest.mark.parametrize("n1,n_orb", RENEW_STATIC)
def test_renew_static_limits_tiles_and_unit_distance(ctx, oracle, n1, n_orb):
    from vdo_slam_amd import tracking as TR
    c = N.renew_static_case(n1, n_orb)
    im = _images(ctx, c["depth"], c["flow"], c["mask"])
    for m in _max_nums(c):
        exp = T.renew_static(oracle, c["tm"], c["stat_x"], c["stat_y"], c["orb_x"], c["orb_y"], c["mask"], c["depth"], c["flow"], m)
        assert ((exp["inlier_id"] >= 0).sum(), (exp["inlier_id"] < 0).sum()) == N.renew_static_expected(c, m)
        got = TR.renew_static(im, c["tm"], c["stat_x"], c["stat_y"], c["orb_x"], c["orb_y"], m)
        _same(got, exp, f"max_num {m}")
        got3 = TR.renew_static(im, c["tm"], c["stat_x"], c["stat_y"], c["orb_x"], c["orb_y"], m, world=(K4, TWC))
        _same(got3, exp, f"max_num {m}, world")
        assert np.array_equal(got3["xyz"], TR.get3d_world(ctx, got3["key_x"], got3["key_y"], got3["depth"], K4, TWC))
    _check_static_pairs(c, got)
    assert (got["depth"] == 40.0).sum() > 100 and (c["depth"] == N.above(40.0)).sum() > 50
    im.close()


# =============================================================================================================================
# 7. RenewFrameInfo, objects
# =============================================================================================================================
@gpu
@pytest.mark.parametrize("nc0,n_tmp", RENEW_OBJECT)
def test_renew_object_bounds_limits_and_capacity(ctx, oracle, nc0, n_tmp):
    from vdo_slam_amd import tracking as TR
    c = N.renew_object_case(nc0, n_tmp)
    im = _images(ctx, c["depth"], c["flow"], c["mask"])
    args = (c["inl"], c["stat"], c["sem_pos"], c["mod"], c["cur_x"], c["cur_y"], c["col"], c["tmp"])
    for m in (c["n_valid0"] - 1, c["n_valid0"], c["n_valid0"] + 1, 100000):
        exp = T.renew_object(oracle, *args, c["mask"], c["depth"], c["flow"], m)
        _check_object_counts(c, exp, m)
        got = TR.renew_object(im, *args, m)
        _same(got, exp, f"max_num_obj {m}")
        got3 = TR.renew_object(im, *args, m, world=(K4, TWC))
        _same(got3, exp, f"max_num_obj {m}, world")
        assert np.array_equal(got3["xyz"], TR.get3d_world(ctx, got3["key_x"], got3["key_y"], got3["depth"], K4, TWC))
        total = exp["key_x"].size
        assert TR.renew_object(im, *args, m, cap=total)["key_x"].size == total
        for world in (None, (K4, TWC)):
            with pytest.raises(K.VdoError, match="capacity"):
                TR.renew_object(im, *args, m, cap=total - 1, world=world)
    assert (exp["depth"] == N.below(25.0)).sum() > 20 and not (exp["depth"] == 25.0).any()
    im.close()


# =============================================================================================================================
# 8. the single-label warp, UpdateMask, the object chain
# =============================================================================================================================
@gpu
@pytest.mark.parametrize("w", [255, 256, 257, 400])
def test_mask_warp_truncation_and_bounds(ctx, oracle, w):
    from vdo_slam_amd import tracking as TR
    last, flow, cur, must, must_not = N.warp_case(w)
    depth = np.ones((120, w), np.float32)
    exp = N.mask_warp(last, flow, 4, cur)
    assert np.array_equal(exp, T.mask_warp(oracle, last, flow, 4, cur))
    assert all(exp[p] == 4 for p in must) and all(exp[p] == 6 for p in must_not)
    last_im, cur_im = _images(ctx, depth, flow, last), _images(ctx, depth, flow, cur)
    TR.mask_warp(cur_im, last_im, 4)
    assert np.array_equal(TR.download_mask(cur_im), exp)
    TR.mask_warp(cur_im, last_im, 6)                                       # and a second label on top
    assert np.array_equal(TR.download_mask(cur_im), N.mask_warp(last, flow, 6, exp))
    last_im.close(); cur_im.close()


@gpu
def test_update_mask_label_counts_slots_thresholds_and_cascades(ctx, oracle):
    """1, 63, 64 and 65 labels with the missing label in the first, a middle and the last slot; slot 63 recovered through an earlier
    recovery; the 99 / 100 samples threshold, ties, the last histogram bin; the three-deep cascade on both paths.  One pair of image sets
    per size serves every scene of that size, one after the other."""
    from vdo_slam_amd import tracking as TR
    ims = {}
    paths = set()
    for name, sc, rec, one_pass in _scenes():
        if sc.w not in ims:
            ims[sc.w] = (_images(ctx, sc.depth, sc.flow, sc.last), _images(ctx, sc.depth, sc.flow, sc.cur))
        last_im, cur_im = ims[sc.w]
        last_im.upload(sc.depth, sc.flow, sc.last); cur_im.upload(sc.depth, sc.flow, sc.cur)
        exp, n = T.update_mask(oracle, *sc.samples(), sc.last, sc.flow, sc.cur)
        assert sc.recovered(exp) == rec and n == len(rec) and one_pass == (np.unique(sc.sl).size <= ONE_PASS_SLOTS), name
        got_n = TR.update_mask(cur_im, last_im, *sc.samples())
        got = TR.download_mask(cur_im)
        assert got_n == n and sc.recovered(got) == rec, name
        assert np.array_equal(got, exp), name
        paths.add(one_pass)
    assert paths == {True, False}
    for a, b in ims.values():
        a.close(); b.close()


@gpu
@pytest.mark.parametrize("n_labels", [6, 64, 65])
def test_update_mask_refuses_a_label_outside_the_bins_and_recovers(ctx, oracle, n_labels):
    """A current-mask label 1023 under the samples runs (the scenes above); 1024 raises VdoError naming the limit, on the one-pass path
    (6 and 64 labels) and on the label-after-label path (65).  The next call on the same image sets, images uploaded afresh, equals the
    oracle: the ticket and the candidate image are clean after the error."""
    from vdo_slam_amd import tracking as TR
    bad, _ = N.scene_votes(400, n_labels, bad_label=1024)
    assert (bad.cur == 1024).sum() == 10 and (n_labels <= ONE_PASS_SLOTS) == (np.unique(bad.sl).size <= ONE_PASS_SLOTS)
    last_im, cur_im = _images(ctx, bad.depth, bad.flow, bad.last), _images(ctx, bad.depth, bad.flow, bad.cur)
    good = [N.scene_votes(400, n_labels), N.scene_cascade(400, max(n_labels, 8), 1, 3, 6)]
    for sc, rec in good:
        last_im.upload(bad.depth, bad.flow, bad.last); cur_im.upload(bad.depth, bad.flow, bad.cur)
        with pytest.raises(K.VdoError, match=r"outside \[0,1024\)"):
            TR.update_mask(cur_im, last_im, *bad.samples())
        last_im.upload(sc.depth, sc.flow, sc.last); cur_im.upload(sc.depth, sc.flow, sc.cur)
        exp, n = T.update_mask(oracle, *sc.samples(), sc.last, sc.flow, sc.cur)
        assert sc.recovered(exp) == rec
        assert TR.update_mask(cur_im, last_im, *sc.samples()) == n
        assert np.array_equal(TR.download_mask(cur_im), exp)
    last_im.close(); cur_im.close()


@gpu
def test_update_mask_two_label_sets_alternate_on_the_same_images(ctx, oracle):
    """The 64-label scene (one pass, slot 63 recovered after slot 10) and the 65-label cascade (label after label), alternately, four
    times each on the same two image sets."""
    from vdo_slam_amd import tracking as TR
    a, rec_a = N.scene_top_slot_after_recovery(400)
    b, rec_b = N.scene_cascade(400, 65, 10, 40, 63)
    c, rec_c = N.scene_cascade(400, 8, 1, 3, 6)
    exp = {id(sc): T.update_mask(oracle, *sc.samples(), sc.last, sc.flow, sc.cur) for sc in (a, b, c)}
    last_im, cur_im = _images(ctx, a.depth, a.flow, a.last), _images(ctx, a.depth, a.flow, a.cur)
    for k in range(4):
        for sc, rec in ((a, rec_a), (b, rec_b), (c, rec_c)):
            last_im.upload(sc.depth, sc.flow, sc.last); cur_im.upload(sc.depth, sc.flow, sc.cur)
            assert TR.update_mask(cur_im, last_im, *sc.samples()) == exp[id(sc)][1] == len(rec), k
            assert np.array_equal(TR.download_mask(cur_im), exp[id(sc)][0]), k
    last_im.close(); cur_im.close()


@gpu
def test_object_chain_on_the_cascade_and_on_64_labels(ctx, oracle):
    """vdo_object_chain = vdo_update_mask + vdo_propagate_object + vdo_scene_flow, bit for bit, where the vote's second phase runs."""
    from vdo_slam_amd import tracking as TR
    Tl = np.eye(4, dtype=np.float32)
    Tc = np.eye(4, dtype=np.float32); Tc[:3, 3] = [0.02, -0.01, -0.8]
    for sc, rec in (N.scene_cascade(400, 8, 1, 3, 6), N.scene_top_slot_after_recovery(400), N.scene_cascade(400, 65, 10, 40, 63)):
        sl, cx, cy = sc.samples()
        ld = np.full(sl.size, 10.0, np.float32)
        last_im = _images(ctx, sc.depth, sc.flow, sc.last)
        cur_a, cur_b = _images(ctx, sc.depth, sc.flow, sc.cur), _images(ctx, sc.depth, sc.flow, sc.cur)
        rec_a = TR.update_mask(cur_a, last_im, sl, cx, cy)
        d_a, sem_a = TR.propagate_object(cur_a, cx, cy, TH_DEPTH_OBJ)
        fl_a, ol_a = TR.scene_flow(ctx, (cx, cy, d_a, sem_a), Tc, (sc.kx, sc.ky, ld, sl), Tl, K4, np.full(sl.size, -2, np.int32))
        rec_b, d_b, sem_b, fl_b, ol_b = TR.object_chain(cur_b, last_im, sl, cx, cy, TH_DEPTH_OBJ, Tc, sc.kx, sc.ky, ld, Tl, K4)
        exp, n = T.update_mask(oracle, sl, cx, cy, sc.last, sc.flow, sc.cur)
        assert rec_a == rec_b == n == len(rec)
        assert np.array_equal(TR.download_mask(cur_a), exp) and np.array_equal(TR.download_mask(cur_b), exp)
        d_o, sem_o = T.propagate_object(oracle, cx, cy, sc.depth, exp, TH_DEPTH_OBJ)
        assert np.array_equal(d_b, d_o) and np.array_equal(sem_b, sem_o)
        assert np.array_equal(d_a, d_b) and np.array_equal(sem_a, sem_b) and np.array_equal(fl_a, fl_b) and np.array_equal(ol_a, ol_b)
        for s in rec:                                  # the samples of a recovered label see their own label again
            assert (sem_b[sl == N.slot_label(s)] == N.slot_label(s)).sum() >= 80
        for x in (last_im, cur_a, cur_b):
            x.close()
