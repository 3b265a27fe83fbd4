"""Fixture graphs of tests/test_ba_plan.py (the batch solver's host-only tile planner, csrc/ba_plan.hip) and the digests that pin its layout.

tests/golden/ba_plan_digests.json holds, per fixture:
  input  sha256 over the graph's sizes (n_pose, n_point, n_eb, n_et, n_ep, n_prior as int64) and its index arrays as int32, in the order of INPUT_ARRAYS;
  dims   the plan's scalars (vdo_slam_amd.ba.PLAN_DIMS);
  plan   sha256 over the plan's integer arrays in the order of vdo_slam_amd.ba.PLAN_INT_ARRAYS, each as its name, its length (int64) and its bytes.
It is written by `python -m tests.ba_plan_fixtures --write` and was written from the planner as it was lifted, statement for statement, out of vdo_ba_create:
the digests stand for the layout of the commit before the planner existed."""
import dataclasses
import functools
import hashlib
import json
import os

import numpy as np

from vdo_slam_amd import synth
from vdo_slam_amd.ba import PLAN_INT_ARRAYS, plan_graph

from tests import ba_envelope_graphs as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_plan_digests.json")
INPUT_ARRAYS = ("eb_pose", "eb_point", "et_p1", "et_p2", "et_pose", "ep_i", "ep_j", "pr_pose")
PLACE_MIN_INC = 32768       # kPlaceMinInc: from this many incidences on the edges of a tile are placed bank-aware


def with_loop_edge(g):
    """g with one more EdgeSE3 between cameras 0 and 2: camera 2 then has degree 3 and the odometry component is no path"""
    assert g.n_cam >= 4
    z = np.zeros((1, 12)); z[0, [0, 4, 8]] = 1.0
    return dataclasses.replace(g, ep_i=np.concatenate([g.ep_i, np.array([0], np.int32)]), ep_j=np.concatenate([g.ep_j, np.array([2], np.int32)]),
                               ep_z=np.concatenate([g.ep_z, z]), ep_info=np.concatenate([g.ep_info, np.eye(6).reshape(1, 36)]))


_BUILD = {
    "window": lambda: synth.make_ba_graph(6, 100, 1, 10, seed=11),
    "smoke": lambda: synth.make_ba_graph(10, 400, 2, 40, seed=7),
    "twisted": lambda: synth.make_ba_graph(20, 300, 2, 20, seed=3),
    "placed": lambda: synth.make_ba_graph(30, 6000, 2, 40, seed=5),
    "chain_256": lambda: E.chain_graph(256)[0],
    "pieces_256": lambda: E.repeated_chain_graph(128, [7] * 128)[0],
    "packed_128": lambda: E.packed_chains_graph(128),
    "packed_129": lambda: E.packed_chains_graph(129),
    "hub_257": lambda: E.hub_graph(257)[0],
    "static_1537": lambda: E.static_point_graph([13] + [12] * 127)[0],
    "mixed_vertex": lambda: E.with_motion_observation(*E.chain_graph(100)),
    "loop": lambda: with_loop_edge(synth.make_ba_graph(6, 100, 1, 10, seed=11)),
}
IDS = tuple(_BUILD)


@functools.lru_cache(maxsize=None)
def graph(name):
    """the fixture graph `name` (built once per process; do not modify)"""
    return _BUILD[name]()


def input_digest(g):
    h = hashlib.sha256()
    h.update(np.array([g.n_pose, g.n_point, g.n_eb, g.n_et, g.n_ep, g.n_prior], np.int64).tobytes())
    for name in INPUT_ARRAYS:
        h.update(np.ascontiguousarray(getattr(g, name), dtype=np.int32).tobytes())
    return h.hexdigest()


def plan_digest(plan):
    h = hashlib.sha256()
    for name in PLAN_INT_ARRAYS:
        a = np.ascontiguousarray(plan[name])
        h.update(name.encode()); h.update(np.int64(a.size).tobytes()); h.update(a.tobytes())
    return h.hexdigest()


def digests(name):
    g = graph(name)
    plan = plan_graph(g)
    return {"input": input_digest(g), "dims": plan["dims"], "plan": plan_digest(plan)}


if __name__ == "__main__":
    import sys
    if "--write" not in sys.argv[1:]:
        sys.exit("usage: python -m tests.ba_plan_fixtures --write")
    with open(GOLDEN, "w") as f:
        json.dump({name: digests(name) for name in IDS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
