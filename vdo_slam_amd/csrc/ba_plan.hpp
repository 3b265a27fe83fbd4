// The batch solver's device layout as a PLAN: plain host vectors and scalars, decided from the graph alone (ba_plan.hip: host code only - no device, no context,
// no LDS size).  vdo_ba_create (capi_ba.hip) checks the plan against the tile kernels' LDS, allocates and uploads it; vdo_ba_plan_create hands it to the tests.
// Every array here is what the device array of the same name (ba_dev.hpp) receives, byte for byte.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/vdo_slam_hip.h"
#include "ba_dev.hpp"

namespace vdo {

// the create-time switches, read once per call
struct BaPlanOptions {
  bool trace = false;           // VDO_BATCH_TRACE: the planner keeps its phase times, vdo_ba_create prints them
  int tile_ept = 0;             // VDO_BA_TILE_EPT: incidences a tile is closed at = 256 x this (0: by the graph's size)
  bool no_hubs = false;         // VDO_BA_NO_HUBS: a static point beyond a tile is refused (the envelope's messages)
  bool wide_partials = false;   // VDO_BA_WIDE_PARTIALS: 32 sums per partial row whatever the graph
  bool no_twist = false;        // VDO_BA_NO_TWIST: pose chains in path order
  static BaPlanOptions from_env();
};

struct BaPlan {
  int P = 0, L = 0, Eb = 0, Et = 0, Ep = 0, Npr = 0;      // the graph's sizes
  // tiles
  std::vector<Tile> tiles;                  // in build order (= order of the points)
  std::vector<int32_t> tile_order;          // launch position -> build index
  std::vector<Tile> tiles_launch;           // tiles[tile_order[b]]: what the device holds (>= 1 entry)
  std::vector<int32_t> tile_pose;           // [NPS + 1] global pose of every slot: the tiles' slots, then one per hub edge, then one entry of padding
  std::vector<int32_t> chain_off, pt_prev_edge;
  std::vector<uint8_t> pt_single;
  std::vector<int32_t> eb_key, et_key, et_slot, inc_key;      // (eb_key: >= one row of 256)
  // permutations between the caller's numbering and the tile-major one; incidence of every (new) edge
  std::vector<int32_t> pt_old_of_new, pt_new_of_old, eb_old_of_new, et_old_of_new;
  std::vector<int32_t> inc_of_eb, inc1_of_et, inc2_of_et;
  // pose -> slots, pose-major partial rows
  std::vector<int32_t> ps_off, ps_idx, slot_dst, pose_kind;
  int ps_stride = 16;
  // pose -> EdgeSE3 / priors, pose chains
  std::vector<int32_t> pe_off, pe_idx, pr_off, pr_idx;
  std::vector<int32_t> pc_off, pc_pose, pc_edge, pc_far_pos, pc_far_edge;
  int pc_maxlen = 1;
  // hub landmarks (ba_hub.hip)
  std::vector<int32_t> hub_off, hub_point, hub_pose, hub_eb_old, hub_row;
  std::vector<double> hub_z, hub_w;
  // permuted data; compact_edges says which of them the device takes (bit 0: uniform eb_w, 1: fp32 eb_z, 2: uniform et_w, 3: et_z all zero)
  std::vector<double> point, eb_z, eb_w, et_z, et_w;
  std::vector<float> eb_zf;
  int compact_edges = 0;
  int max_slots = 1, n_dyn_tiles = 0, NPS = 0, NPS_tiles = 0;
  bool pose_graph_is_paths = true;
  bool dense_tiles_ok = true;               // the incidence half: every tile fits the dense assembly's VDO_TILE_EPT + 2 incidences per thread, and there is no hub
  // VDO_BATCH_TRACE: cumulative ms at the end of validate, tracks, tiles, hubs, permuted data; ms spent closing tiles
  double t_mark[5] = {0, 0, 0, 0, 0}, t_close_ms = 0;

  int n_tiles() const { return (int)tiles.size(); }
  int n_chains() const { return (int)chain_off.size() - 1; }
  int n_pchains() const { return (int)pc_off.size() - 1; }
  int n_hubs() const { return (int)hub_point.size(); }
  int n_hub_edges() const { return (int)hub_pose.size(); }
  int Ebp() const { return (int)eb_old_of_new.size(); }       // entries of the padded edge blocks = the device's edge index space
};

// Fills `plan` from the graph.  VDO_OK, or the code of a refusal with its message in set_error.
int plan_graph(const vdo_ba_graph& g, const BaPlanOptions& opt, BaPlan& plan);

// ---- landmark tracks (shared with vdo_ba_partition): a track = one static point, or the chain of per-frame points of one dynamic feature linked by
// LandmarkMotionTernaryEdges
struct TrackLinks {
  std::vector<int32_t> next_e, prev_e;      // per point: the ternary edge that leaves it (the point is its p1) / enters it (p2), -1: none
  // f(point, ternary edge to the next point or -1) for every point of the track that starts at `head`, in chain order
  template <class F>
  void walk(const vdo_ba_graph& g, int head, F f) const {
    for (int c = head;;) {
      const int e = next_e[c];
      f(c, e);
      if (e == -1) break;
      c = g.et_p2[e];
    }
  }
};

// links the points of every track (refused: a point with two successors or two predecessors); the ternary edges' indices must be in range
int link_tracks(const vdo_ba_graph& g, TrackLinks& lk);

// The tracks of the graph in the order of their first points: a copy of `init` each, its `head` set, on_point(track, point, edge to the next point or -1)
// called along it.  Refused: tracks that are no simple chains, ternary edges that form a cycle.
template <class T, class F>
int find_tracks(const vdo_ba_graph& g, TrackLinks& lk, const T& init, F on_point, std::vector<T>& tracks) {
  const int rc = link_tracks(g, lk);
  if (rc != VDO_OK) return rc;
  int visited = 0;
  for (int l = 0; l < g.n_point; ++l) {
    if (lk.prev_e[l] != -1) continue;
    T t = init;
    t.head = l;
    lk.walk(g, l, [&](int c, int e) { ++visited; on_point(t, c, e); });
    tracks.push_back(t);
  }
  if (visited != g.n_point) return set_error(VDO_ERR_UNSUPPORTED, "ternary edges form a cycle");
  return VDO_OK;
}

}  // namespace vdo
