"""GPU: the seam between the dense mapper and its colourer.  Both move their words with the same code (dn_queue_move over dense_plan.hpp's dn_move), so
after a recenter of the map and the follow of the colour volume the surviving words sit in the same slots - and those are the slots the brute-force
rule keeps: a slot keeps its word iff its global voxel is the same before and after.

5 x 3 x 7 at origin (-2, 4, -6): no size is a multiple of anything and origin mod size is non-zero on every axis.  The moves: one slab, three slabs,
a negative move, a move of exactly n on one axis and one of -n on another (both clear everything)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, ORIGIN = (5, 3, 7), (-2, 4, -6)
MOVES = [(1, 0, 0), (-2, 1, 3), (0, -3, 0), (5, 0, 0), (4, 2, -6)]


def _kept(origin, new_origin):
    """[nz, ny, nx] bool: the slots whose global voxel is the same at both origins"""
    keep = []
    for a in range(3):
        s = np.arange(N[a])
        g0 = origin[a] + (s - origin[a]) % N[a]
        g1 = new_origin[a] + (s - new_origin[a]) % N[a]
        keep.append(g0 == g1)
    return keep[2][:, None, None] & keep[1][None, :, None] & keep[0][None, None, :]


def test_map_and_colour_keep_the_same_slots():
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.colour import Colourer
    from vdo_slam_amd.dense import DenseMapper
    ctx = Context(0)
    m = DenseMapper(ctx, 8, 6, N, 0.25, (10.0, 10.0, 4.0, 3.0), origin=ORIGIN, trunc=1.0, min_depth=0.3, max_depth=3.0, max_weight=64, stage_points=64)
    c = Colourer(m, 0.25, 64, 64)
    try:
        fill = np.random.default_rng(5).integers(1, 1 << 32, N[::-1], dtype=np.uint64).astype(np.uint32)
        assert fill.all()
        seen = set()
        for mv in MOVES:
            m.recenter(ORIGIN)
            c.set_volume(fill)                       # (follows the map back to ORIGIN first)
            m.set_volume(fill)
            new = tuple(ORIGIN[a] + mv[a] for a in range(3))
            m.recenter(new)
            wm, om = m.volume()
            wc, oc = c.volume()
            assert om == new and oc == new, mv
            keep = _kept(ORIGIN, new)
            assert np.array_equal(wm != 0, wc != 0), mv
            assert np.array_equal(wm, np.where(keep, fill, 0)) and np.array_equal(wc, np.where(keep, fill, 0)), mv
            seen.add(int(keep.sum()))
        assert 0 in seen and len(seen) >= 3          # everything cleared, and slabs of more than one size
    finally:
        c.close()
        m.close()
        ctx.close()
