// Host-only: the tile planner of the batch solver (ba_plan.hpp).  plan_graph decides the whole device layout of a graph - which points share a tile, where every
// edge sits in its tile's block, the pose-side tables, the pose chains, the launch order - as plain host vectors; vdo_ba_create (capi_ba.hip) uploads them.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ba_plan.hpp"

namespace vdo {

BaPlanOptions BaPlanOptions::from_env() {
  BaPlanOptions o;
  o.trace = std::getenv("VDO_BATCH_TRACE") != nullptr;
  if (const char* e = std::getenv("VDO_BA_TILE_EPT")) o.tile_ept = std::max(1, std::atoi(e));
  o.no_hubs = std::getenv("VDO_BA_NO_HUBS") != nullptr;
  o.wide_partials = std::getenv("VDO_BA_WIDE_PARTIALS") != nullptr;
  o.no_twist = std::getenv("VDO_BA_NO_TWIST") != nullptr;
  return o;
}

int link_tracks(const vdo_ba_graph& g, TrackLinks& lk) {
  lk.next_e.assign(g.n_point, -1);
  lk.prev_e.assign(g.n_point, -1);
  for (int e = 0; e < g.n_et; ++e) {
    if (lk.next_e[g.et_p1[e]] != -1 || lk.prev_e[g.et_p2[e]] != -1)
      return set_error(VDO_ERR_UNSUPPORTED, "ternary edge %d: landmark tracks must be simple chains", e);
    lk.next_e[g.et_p1[e]] = e;
    lk.prev_e[g.et_p2[e]] = e;
  }
  return VDO_OK;
}

namespace {

constexpr int kSoftSlots = 64;     // normal tiles stay below this many pose slots
constexpr int kHardSlots = 512;    // a single long DYNAMIC track may use up to this many (a chain of n points touches n cameras + n - 1 motion vertices: n <= 256 = VDO_TILE_PTS): the tile kernels
                                   // stage slots in rounds of 256.  Reachable: 511 (<= 256 cameras - one per-pose piece each - and <= 255 motions), ~140 KB of LDS at 16 sums per partial row
                                   // (ONE workgroup per CU - paid only by graphs that hold such a track); at 32 sums per row the sweep's LDS caps a tile lower - vdo_ba_create checks
                                   // every tile kernel's LDS against the plan and refuses beyond
constexpr int kStaticSlots = 256;  // a STATIC point beyond this many pose vertices is a hub landmark (ba_hub.hip: no LDS at all) instead of a tile of its own
// a graph of a few tiles - the 20-frame windows: 8 k edges - is launch-bound whatever its bank conflicts are, and the placement was half of its 0.9 ms of tile building:
// below this many incidences the edges of a tile keep their pose-sorted order
constexpr int64_t kPlaceMinInc = 32768;
constexpr int kTwistMin = 16;      // pose chains from this length on are stored twisted (pose_chains)

// CSR of items 0 .. n - 1 by key: idx[off[k] .. off[k + 1]) are the items of key k, in ascending order
template <class KeyOf>
void csr_fill(int n_keys, int n, KeyOf key_of, std::vector<int32_t>& off, std::vector<int32_t>& idx) {
  off.assign((size_t)n_keys + 1, 0);
  idx.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) off[key_of(i) + 1]++;
  for (int k = 0; k < n_keys; ++k) off[k + 1] += off[k];
  std::vector<int32_t> fill(off.begin(), off.end() - 1);
  for (int i = 0; i < n; ++i) idx[fill[key_of(i)]++] = i;
}

// Threads the EdgeSE3PointXYZ edges of a SORTED pose list need: every thread of a tile kernel takes <= ept edges of ONE pose, so every run of equal poses is cut
// into pieces of <= ept
template <class PoseOf>
int pieces(int n, PoseOf pose_of, int ept) {
  int need = 0;
  for (int j = 0; j < n;) {
    int k = j;
    while (k < n && pose_of(k) == pose_of(j)) ++k;
    need += (k - j + ept - 1) / ept;
    j = k;
  }
  return need;
}

int validate(const vdo_ba_graph& g) {
  const unsigned P = g.n_pose, L = g.n_point;
  for (int e = 0; e < g.n_eb; ++e)
    if ((unsigned)g.eb_pose[e] >= P || (unsigned)g.eb_point[e] >= L) return set_error(VDO_ERR_INVALID, "binary edge %d: index out of range", e);
  for (int e = 0; e < g.n_et; ++e)
    if ((unsigned)g.et_pose[e] >= P || (unsigned)g.et_p1[e] >= L || (unsigned)g.et_p2[e] >= L || g.et_p1[e] == g.et_p2[e])
      return set_error(VDO_ERR_INVALID, "ternary edge %d: index out of range", e);
  for (int e = 0; e < g.n_ep; ++e)
    if ((unsigned)g.ep_i[e] >= P || (unsigned)g.ep_j[e] >= P || g.ep_i[e] == g.ep_j[e]) return set_error(VDO_ERR_INVALID, "pose-pose edge %d: index out of range", e);
  for (int e = 0; e < g.n_prior; ++e)
    if ((unsigned)g.pr_pose[e] >= P) return set_error(VDO_ERR_INVALID, "prior %d: index out of range", e);
  // robust-kernel widths: g2o keeps delta^2 in a FLOAT member (robust_kernel_impl.h:84); the tile kernels' Huber weight (se3_dev.hpp huber_dev) takes its
  // square root without range scaling and relies on e > dsqr being a NORMAL number: a positive delta whose float square underflows (delta below ~1.1e-19) is
  // refused - no camera, depth or motion residual is measured in units where that is a width
  for (const double hd : {g.huber_eb, g.huber_et, g.huber_ep})
    if (hd > 0 && !((double)(float)(hd * hd) >= 1.1754943508222875e-38))
      return set_error(VDO_ERR_INVALID, "vdo_ba_create: Huber width %.3g: its square is not a normal float (RobustKernelHuber keeps it in one)", hd);
  return VDO_OK;
}

// ---- tracks
struct Track { int32_t head, npts, ninc, key; };      // first point, points, incidences (EdgeSE3PointXYZ + 2 per ternary edge), first pose that observes it

struct Tracks {
  TrackLinks links;
  std::vector<int32_t> pb_off, pb_idx;      // point -> its EdgeSE3PointXYZ edges
  std::vector<Track> list;
};

// Order of the tracks = order of the tiles' contents: the DYNAMIC tracks (chains of several points) first, among themselves by first observing frame, then the
// static points by first observing frame.  A dynamic track of n points brings 2 n - 1 pose vertices (its cameras and its motions) - more than the 64 slots a tile
// is closed at - and its neighbours in time on the same object share nearly all of them; interleaved with the static points every such track would close its tile
// behind itself and sit there alone: one lane of 256 walking its chain in the solver's kernels.
int find_and_order_tracks(const vdo_ba_graph& g, Tracks& tr) {
  csr_fill(g.n_point, g.n_eb, [&](int e) { return g.eb_point[e]; }, tr.pb_off, tr.pb_idx);
  tr.list.reserve(g.n_point);
  const int rc = find_tracks(g, tr.links, Track{0, 0, 0, g.n_pose}, [&](Track& t, int c, int e) {
    ++t.npts;
    t.ninc += tr.pb_off[c + 1] - tr.pb_off[c] + (e == -1 ? 0 : 2);
    for (int k = tr.pb_off[c]; k < tr.pb_off[c + 1]; ++k) t.key = std::min(t.key, g.eb_pose[tr.pb_idx[k]]);
  }, tr.list);
  if (rc != VDO_OK) return rc;
  std::stable_sort(tr.list.begin(), tr.list.end(), [](const Track& a, const Track& b) {
    const bool da = a.npts > 1, db = b.npts > 1;
    if (da != db) return da;
    return a.key < b.key;
  });
  return VDO_OK;
}

// the pose vertices of a track's edges, in chain order: all of them, and those of its EdgeSE3PointXYZ edges alone (a static point has no others)
struct TrackPoses {
  std::vector<int32_t> all, eb_only;
  bool is_static = true;
  const std::vector<int32_t>& eb() const { return is_static ? all : eb_only; }
  void of(const vdo_ba_graph& g, const Tracks& tr, const Track& t) {
    all.clear(); eb_only.clear();
    is_static = t.npts == 1;
    tr.links.walk(g, t.head, [&](int c, int e) {
      for (int k = tr.pb_off[c]; k < tr.pb_off[c + 1]; ++k) {
        all.push_back(g.eb_pose[tr.pb_idx[k]]);
        if (!is_static) eb_only.push_back(all.back());
      }
      if (e != -1) all.push_back(g.et_pose[e]);
    });
  }
};

int distinct_count(std::vector<int32_t> v) {
  std::sort(v.begin(), v.end());
  return (int)(std::unique(v.begin(), v.end()) - v.begin());
}

int pieces_of(std::vector<int32_t> poses) {
  std::sort(poses.begin(), poses.end());
  return pieces((int)poses.size(), [&](int k) { return poses[k]; }, VDO_TILE_EPT);
}

// ---- tiles
// The open tile: tracks are added while they fit, close() writes the tile's slots, its edge block and its descriptor into the plan.
struct OpenTile {
  const vdo_ba_graph& g;
  const Tracks& tr;
  BaPlan& plan;
  const bool trace;
  const bool place;       // bank-aware placement of the edges (else pose-sorted order)
  int soft_inc;           // incidences a tile is closed at
  int dyn_slot_cap = 0;   // distinct pose vertices of the graph's largest dynamic track
  Tile cur{};
  int id = 0, npts = 0, ninc = 0;
  int need = 0;           // threads the open tile needs: sum over its poses of ceil(EdgeSE3PointXYZ edges / VDO_TILE_EPT)
  bool dyn_only = true;   // it holds dynamic tracks only
  int inc_total = 0;
  bool thr_overflow = false;
  std::vector<int32_t> poses, eb, et;                     // its distinct pose vertices, the original ids of its edges
  std::vector<int32_t> pose_stamp, pose_cnt, cnt_stamp;   // per pose: the tile that took it last; its EdgeSE3PointXYZ edges in the open tile (valid where cnt_stamp == id)
  std::vector<int32_t> et_new_of_old;
  std::vector<int32_t> slot_lut, sort_cnt, sort_slot, sort_tmp;      // close: slot of a pose of the tile, scratch of its counting sorts

  OpenTile(const vdo_ba_graph& g_, const Tracks& tr_, const BaPlanOptions& opt, BaPlan& plan_)
      : g(g_), tr(tr_), plan(plan_), trace(opt.trace), place((int64_t)g_.n_eb + 2 * (int64_t)g_.n_et >= kPlaceMinInc),
        pose_stamp(g_.n_pose, -1), pose_cnt(g_.n_pose, 0), cnt_stamp(g_.n_pose, -1), et_new_of_old(g_.n_et, -1), slot_lut(g_.n_pose, 0) {
    // Incidences a tile is CLOSED at (soft; a single track may still take up to VDO_TILE_INC): VDO_TILE_EPT per thread spreads what a tile costs
    // apart from its edges over more edges - right for graphs of many tiles; a small graph (the 60-frame window: 0.25 M incidences) would be left
    // with fewer tiles than the device has CUs, so it gets smaller tiles: about four tiles per CU of a 256-CU device, not fewer than 2 edges per thread.
    const int ept = opt.tile_ept ? opt.tile_ept : std::max((int)std::ceil(((double)g.n_eb + 2.0 * (double)g.n_et) / (VDO_TILE_THREADS * 1024.0)), 2);
    soft_inc = VDO_TILE_THREADS * std::min(ept, VDO_TILE_EPT);
  }

  // threads the tile needs with the track's EdgeSE3PointXYZ edges (at the poses `eb_poses`) in it
  int need_with(const std::vector<int32_t>& eb_poses, bool commit) {
    int n = need;
    for (int32_t p : eb_poses) {
      if (cnt_stamp[p] != id) { cnt_stamp[p] = id; pose_cnt[p] = 0; }
      if (pose_cnt[p] % VDO_TILE_EPT == 0) ++n;
      ++pose_cnt[p];
    }
    if (commit) need = n;
    else for (int32_t p : eb_poses) --pose_cnt[p];
    return n;
  }

  bool fits(const Track& t, const TrackPoses& tp) {
    if (npts == 0) return true;
    int newp = 0;
    for (int32_t p : tp.all) if (pose_stamp[p] != id) ++newp;      // upper bound (a pose the track touches twice counts twice)
    // slots a tile is closed at: kSoftSlots - but dynamic tracks are packed together up to the slot count the graph's largest track forces on every tile kernel's
    // LDS anyway (the tile kernels' LDS is sized by the largest tile, so packing up to it costs no occupancy; a tile that holds a static point keeps the soft
    // limit).  Packing beyond the largest track's slot count gains nothing on a graph of many dynamic tracks and costs the sweep of a static graph 6 %.
    const int slot_cap = (t.npts > 1 && dyn_only) ? std::max(kSoftSlots, dyn_slot_cap) : kSoftSlots;
    return !(npts + t.npts > VDO_TILE_PTS || ninc + t.ninc > soft_inc || (int)poses.size() + newp > slot_cap || need_with(tp.eb(), false) > VDO_TILE_THREADS);
  }

  int add(const Track& t, const TrackPoses& tp) {
    if (npts == 0) {
      dyn_only = true;
      cur = Tile{};
      cur.pt_begin = (int32_t)plan.pt_old_of_new.size();
      cur.chain_begin = (int32_t)plan.chain_off.size() - 1;
    }
    dyn_only = dyn_only && t.npts > 1;
    for (int32_t p : tp.all)
      if (pose_stamp[p] != id) { pose_stamp[p] = id; poses.push_back(p); }
    if ((int)poses.size() > kHardSlots) return set_error(VDO_ERR_UNSUPPORTED, "landmark track touches %zu pose vertices (limit %d)", poses.size(), kHardSlots);
    tr.links.walk(g, t.head, [&](int c, int e) {
      plan.pt_new_of_old[c] = (int32_t)plan.pt_old_of_new.size();
      plan.pt_old_of_new.push_back(c);
      plan.pt_prev_edge.push_back(tr.links.prev_e[c]);      // original ternary id for now; build_tiles remaps it
      for (int k = tr.pb_off[c]; k < tr.pb_off[c + 1]; ++k) eb.push_back(tr.pb_idx[k]);
      if (e != -1) et.push_back(e);
    });
    plan.chain_off.push_back((int32_t)plan.pt_old_of_new.size());
    npts += t.npts; ninc += t.ninc;
    need_with(tp.eb(), true);
    return VDO_OK;
  }

  int32_t local_point(int32_t old_point) const { return plan.pt_new_of_old[old_point] - cur.pt_begin; }

  // ids in slot order, ties in the order they came (= std::stable_sort by pose, as a counting sort: a comparator's two random reads into the pose array per
  // comparison made the sort 0.7 of the 0.9 s of planning a 1 M-point graph)
  void sort_by_slot(std::vector<int32_t>& ids, const int32_t* pose_of) {
    if (ids.size() < 2) return;
    const int ns = (int)poses.size();
    sort_cnt.assign((size_t)ns + 1, 0);
    sort_slot.resize(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) { sort_slot[k] = slot_lut[pose_of[ids[k]]]; ++sort_cnt[(size_t)sort_slot[k] + 1]; }
    for (int k = 0; k < ns; ++k) sort_cnt[(size_t)k + 1] += sort_cnt[k];
    sort_tmp.resize(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) sort_tmp[(size_t)sort_cnt[sort_slot[k]]++] = ids[k];
    ids.swap(sort_tmp);
  }

  // Fills the tile's block of 256 x ept entries from its pose-sorted edges `eb`.  false: the runs need more than 256 threads.
  // Which edge of a slot's run goes to which (thread, row) is free - a thread needs <= ept edges of ONE slot in rows 0 .. count - 1, nothing else -
  // and it decides the LDS bank conflicts of every tile kernel: row i of a wave is one LDS instruction per operand, 64 lanes at the local point
  // ids of their edges (point reads, the four landmark ds_add_f64 of the sweep, the factor reads of the solver's kernels).  The LDS serves
  // a wave in lane groups - 16 contiguous lanes for 64-bit stores / atomics (32 banks: point id mod 16), 32 for 64-bit reads (64 banks: id mod 32)
  // - and every extra distinct address on a bank costs a cycle: with the edges in pose-sorted order the ids of a group are random (2.5 .. 3 addresses
  // on the busiest bank, the LDS pipe busy ~85 % of the sweep).  So: rows are filled one after the other (thread counts stay balanced: ceil or
  // floor of run / threads), and every (thread, row) takes, of its slot's remaining edges, one whose point id collides with the fewest lanes
  // already placed in its 16-lane group and 32-lane half of that row.  Without `place` the cost is zero everywhere: the edges keep their order.
  bool place_edges(int ept) {
    const int nb_real = (int)eb.size();
    int32_t* const old_of_new = plan.eb_old_of_new.data() + cur.eb_begin;
    int32_t* const key_of = plan.eb_key.data() + cur.eb_begin;
    int32_t* const inc_of = plan.inc_key.data() + inc_total;
    static thread_local std::vector<int> bucket[32];
    int occ16[VDO_TILE_THREADS / 64][VDO_TILE_EPT][4][16], occ32[VDO_TILE_THREADS / 64][VDO_TILE_EPT][2][32];
    std::memset(occ16, 0, sizeof occ16); std::memset(occ32, 0, sizeof occ32);
    int t = 0;
    for (int j = 0; j < nb_real;) {
      int k = j;
      while (k < nb_real && g.eb_pose[eb[k]] == g.eb_pose[eb[j]]) ++k;
      const int len = k - j, nthr = (len + ept - 1) / ept;
      if (t + nthr > VDO_TILE_THREADS) return false;
      for (int r = 0; r < 32; ++r) bucket[r].clear();
      uint32_t nonempty = 0;                               // (buckets that still hold an edge: a run of a dozen edges touches a dozen of the 32)
      for (int q = k - 1; q >= j; --q) { const int r = local_point(g.eb_point[eb[q]]) & 31; bucket[r].push_back(eb[q]); nonempty |= 1u << r; }     // (popped from the back: pose-sorted order among equals)
      const int32_t slot = slot_lut[g.eb_pose[eb[j]]];
      int left = len;
      for (int i = 0; i < ept && left > 0; ++i)
        for (int tau = 0; tau < nthr && left > 0; ++tau, --left) {
          const int T = t + tau, w = T >> 6, g16 = (T >> 4) & 3, h = (T >> 5) & 1;
          int best = -1, best_cost = 1 << 30;
          for (uint32_t m = nonempty; m; m &= m - 1) {    // (ascending bucket index, the first minimum wins)
            const int r = __builtin_ctz(m);
            const int cost = place ? 2 * occ16[w][i][g16][r & 15] + occ32[w][i][h][r] : 0;
            if (cost < best_cost) { best_cost = cost; best = r; if (cost == 0) break; }
          }
          const int e = bucket[best].back(); bucket[best].pop_back();
          if (bucket[best].empty()) nonempty &= ~(1u << best);
          ++occ16[w][i][g16][best & 15]; ++occ32[w][i][h][best];
          const int pos = i * VDO_TILE_THREADS + T;
          const int32_t key = (slot << 16) | local_point(g.eb_point[e]);
          old_of_new[pos] = e;
          key_of[pos] = key;
          inc_of[pos] = key;
        }
      t += nthr;
      j = k;
    }
    if (!place) return true;
    // refinement: the rows of ONE thread can be exchanged freely (same slot, same count) - a few passes of pairwise exchanges wherever that lowers
    // the collisions of the two group-rows involved
    const int nthr_used = t;
    auto lp_at = [&](int T, int i) { const int32_t key = key_of[i * VDO_TILE_THREADS + T]; return key < 0 ? -1 : (key & 0xffff); };
    for (int pass = 0; pass < 3; ++pass) {
      int moved = 0;
      for (int T = 0; T < nthr_used; ++T) {
        const int w = T >> 6, g16 = (T >> 4) & 3, h = (T >> 5) & 1;
        int cnt = 0;
        while (cnt < ept && lp_at(T, cnt) >= 0) ++cnt;
        for (int a = 0; a < cnt; ++a) for (int b = a + 1; b < cnt; ++b) {
          const int la = lp_at(T, a), lb = lp_at(T, b);
          if ((la & 31) == (lb & 31)) continue;
          // cost of this thread's two entries where they are, and exchanged (occupancies without this thread's own entries)
          auto c16 = [&](int i, int l) { return occ16[w][i][g16][l & 15]; };
          auto c32 = [&](int i, int l) { return occ32[w][i][h][l & 31]; };
          const int now = 2 * (c16(a, la) - 1) + (c32(a, la) - 1) + 2 * (c16(b, lb) - 1) + (c32(b, lb) - 1);
          const int then = 2 * (c16(a, lb) - ((la & 15) == (lb & 15) ? 1 : 0)) + c32(a, lb) + 2 * (c16(b, la) - ((la & 15) == (lb & 15) ? 1 : 0)) + c32(b, la);
          if (then < now) {
            --occ16[w][a][g16][la & 15]; --occ32[w][a][h][la & 31]; --occ16[w][b][g16][lb & 15]; --occ32[w][b][h][lb & 31];
            ++occ16[w][a][g16][lb & 15]; ++occ32[w][a][h][lb & 31]; ++occ16[w][b][g16][la & 15]; ++occ32[w][b][h][la & 31];
            const int pa = a * VDO_TILE_THREADS + T, pb = b * VDO_TILE_THREADS + T;
            std::swap(old_of_new[pa], old_of_new[pb]); std::swap(key_of[pa], key_of[pb]); std::swap(inc_of[pa], inc_of[pb]);
            ++moved;
          }
        }
      }
      if (!moved) break;
    }
    return true;
  }

  void close() {
    if (npts == 0) return;
    const auto t_close0 = std::chrono::steady_clock::now();
    // slots: the tile's distinct poses, sorted
    std::sort(poses.begin(), poses.end());
    cur.slot_begin = (int32_t)plan.tile_pose.size();
    plan.tile_pose.insert(plan.tile_pose.end(), poses.begin(), poses.end());
    cur.slot_end = (int32_t)plan.tile_pose.size();
    plan.max_slots = std::max(plan.max_slots, cur.slot_end - cur.slot_begin);
    for (int k = 0; k < (int)poses.size(); ++k) slot_lut[poses[k]] = k;
    sort_by_slot(eb, g.eb_pose);
    sort_by_slot(et, g.et_pose);
    // EdgeSE3PointXYZ edges of the tile: a PADDED block of 256 x ept entries in thread-transposed order - entry j * 256 + t is the j-th edge of
    // thread t - so that the tile kernels need no thread table and every load of theirs is one contiguous 256-lane row (with the edges in
    // pose-sorted order and a table of first-edge indices, the six loads of a thread's edges touched the same 12 cache lines six times).
    // Every thread takes <= ept edges of ONE pose slot, ept the smallest of 1 .. VDO_TILE_EPT that fits 256 threads; unused entries carry key -1.
    cur.eb_begin = (int32_t)plan.eb_old_of_new.size();
    cur.et_begin = (int32_t)plan.et_old_of_new.size();
    cur.inc_begin = inc_total;
    const int nb_real = (int)eb.size(), nt = (int)et.size();
    int ept = 1;
    while (ept < VDO_TILE_EPT && pieces(nb_real, [&](int k) { return g.eb_pose[eb[k]]; }, ept) > VDO_TILE_THREADS) ++ept;
    const int nb = nb_real ? VDO_TILE_THREADS * ept : 0;     // entries of the block
    cur.ept = nb_real ? ept : 0;
    plan.eb_old_of_new.resize((size_t)cur.eb_begin + nb, -1);
    plan.eb_key.resize((size_t)cur.eb_begin + nb, -1);
    plan.inc_key.resize((size_t)inc_total + nb + 2 * (size_t)nt, -1);
    if (!place_edges(ept)) thr_overflow = true;
    for (int j = 0; j < nt; ++j) {
      const int e = et[j];
      const int en = (int)plan.et_old_of_new.size();
      plan.et_old_of_new.push_back(e);
      et_new_of_old[e] = en;
      const int32_t sl = slot_lut[g.et_pose[e]];
      const int32_t l1 = local_point(g.et_p1[e]), l2 = local_point(g.et_p2[e]);
      plan.et_key[en] = l1 | (l2 << 16);
      plan.et_slot[en] = sl;
      plan.inc_key[inc_total + nb + j] = (sl << 16) | l1;
      plan.inc_key[inc_total + nb + nt + j] = (sl << 16) | l2;
    }
    inc_total += nb + 2 * nt;
    if (nb + 2 * nt > VDO_TILE_THREADS * (VDO_TILE_EPT + 2)) plan.dense_tiles_ok = false;      // (the dense assembly keeps VDO_TILE_EPT + 2 incidences per thread - cannot happen: nb <= 1536, nt < 256)
    cur.eb_end = (int32_t)plan.eb_old_of_new.size();
    cur.et_end = (int32_t)plan.et_old_of_new.size();
    cur.pt_end = (int32_t)plan.pt_old_of_new.size();
    cur.chain_end = (int32_t)plan.chain_off.size() - 1;
    plan.tiles.push_back(cur);
    ++id;
    npts = 0; ninc = 0; need = 0;
    poses.clear(); eb.clear(); et.clear();
    if (trace) plan.t_close_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_close0).count();
  }
};

// Packs the tracks, in their order, into tiles; `hubs` receives the static points that stay out of them.
// HUB landmarks (ba_hub.hip): a STATIC point (no LandmarkMotionTernaryEdge) whose observations do not fit a tile - more than kStaticSlots distinct pose vertices,
// more than 256 per-pose pieces or more than VDO_TILE_INC edges - stays out of the tiles; a workgroup of its own walks its edges.  A dynamic track beyond the
// envelope is refused, with a message that names the track.
int build_tiles(const vdo_ba_graph& g, const BaPlanOptions& opt, const Tracks& tr, BaPlan& plan, std::vector<int32_t>& hubs) {
  const int L = g.n_point, Eb = g.n_eb, Et = g.n_et;
  plan.chain_off.assign(1, 0);
  plan.pt_old_of_new.reserve(L); plan.pt_prev_edge.reserve(L);
  plan.pt_new_of_old.assign(L, -1);
  plan.eb_old_of_new.reserve(Eb); plan.et_old_of_new.reserve(Et);
  plan.et_key.assign(Et, 0); plan.et_slot.assign(Et, 0);
  plan.eb_key.reserve((size_t)Eb + Eb / 8); plan.inc_key.reserve((size_t)Eb + Eb / 8 + 2 * (size_t)Et);      // (they grow with the padded edge blocks of the tiles)
  OpenTile tile(g, tr, opt, plan);
  TrackPoses tp;
  for (const Track& t : tr.list) {
    if (t.npts <= 1) break;                     // (dynamic tracks come first)
    tp.of(g, tr, t);
    tile.dyn_slot_cap = std::max(tile.dyn_slot_cap, distinct_count(tp.all));
  }
  for (const Track& t : tr.list) {
    tp.of(g, tr, t);
    const bool is_static = t.npts == 1;
    // (a static point of at most min(kStaticSlots, 256 threads) observations - nearly every point of every graph - passes all of the checks below by its count alone)
    const bool plain_static = is_static && t.ninc <= std::min(kStaticSlots, VDO_TILE_THREADS);
    int distinct = 0, n_pieces = 0;
    if (!plain_static) {
      distinct = distinct_count(tp.all);
      n_pieces = pieces_of(tp.eb());
      if (is_static && !opt.no_hubs && (distinct > kStaticSlots || n_pieces > VDO_TILE_THREADS || t.ninc > VDO_TILE_INC)) { hubs.push_back(t.head); continue; }
    }
    if (t.npts > VDO_TILE_PTS || t.ninc > VDO_TILE_INC)
      return set_error(VDO_ERR_UNSUPPORTED, "landmark track with %d points / %d incidences exceeds the tile capacity (%d / %d)", t.npts, t.ninc, VDO_TILE_PTS, VDO_TILE_INC);
    if (!plain_static) {
      // the track on its own must fit a tile: distinct pose vertices <= kHardSlots (LDS slots), and its EdgeSE3PointXYZ edges cut per pose into pieces of
      // <= VDO_TILE_EPT must fit the 256 threads of the sweep
      const int slot_limit = is_static ? kStaticSlots : kHardSlots;      // (a static point gets here only with VDO_BA_NO_HUBS)
      if (distinct > slot_limit)
        return set_error(VDO_ERR_UNSUPPORTED, "landmark track of %d point(s) / %d incidences touches %d distinct pose vertices (limit %d per track)",
                         t.npts, t.ninc, distinct, slot_limit);
      if (n_pieces > VDO_TILE_THREADS)
        return set_error(VDO_ERR_UNSUPPORTED, "landmark track of %d point(s) with %zu EdgeSE3PointXYZ observations needs %d per-pose pieces (limit %d per track)",
                         t.npts, tp.eb().size(), n_pieces, VDO_TILE_THREADS);
    }
    if (!tile.fits(t, tp)) tile.close();
    const int rc = tile.add(t, tp);
    if (rc != VDO_OK) return rc;
  }
  tile.close();
  if (tile.thr_overflow) return set_error(VDO_ERR_UNSUPPORTED, "a tile has more pose-slot pieces than threads");
  for (auto& pe : plan.pt_prev_edge) if (pe >= 0) pe = tile.et_new_of_old[pe];
  // incidence index of every (new) edge, for the un-permuting download
  plan.inc_of_eb.resize(plan.eb_old_of_new.size()); plan.inc1_of_et.resize(Et); plan.inc2_of_et.resize(Et);
  for (const Tile& T : plan.tiles) {
    const int nb = T.eb_end - T.eb_begin, nt = T.et_end - T.et_begin;
    for (int j = 0; j < nb; ++j) plan.inc_of_eb[T.eb_begin + j] = T.inc_begin + j;
    for (int j = 0; j < nt; ++j) { plan.inc1_of_et[T.et_begin + j] = T.inc_begin + nb + j; plan.inc2_of_et[T.et_begin + j] = T.inc_begin + nb + nt + j; }
  }
  plan.eb_key.resize(std::max<size_t>(plan.eb_key.size(), VDO_TILE_THREADS), -1);     // (>= one row: the tile kernels load a thread's edges unconditionally - entry `thread` of the first block for a tile without edges)
  return VDO_OK;
}

// hub landmarks: device points behind every tile's (each a chain of its own), one pose-major partial row ("slot") per edge behind every tile's slots
void add_hubs(const vdo_ba_graph& g, const Tracks& tr, const std::vector<int32_t>& hubs, BaPlan& plan) {
  plan.NPS_tiles = (int)plan.tile_pose.size();
  plan.hub_off.assign(1, 0);
  for (int32_t c : hubs) {
    plan.pt_new_of_old[c] = (int32_t)plan.pt_old_of_new.size();
    plan.hub_point.push_back((int32_t)plan.pt_old_of_new.size());
    plan.pt_old_of_new.push_back(c);
    plan.pt_prev_edge.push_back(-1);
    plan.chain_off.push_back((int32_t)plan.pt_old_of_new.size());
    for (int k = tr.pb_off[c]; k < tr.pb_off[c + 1]; ++k) { const int o = tr.pb_idx[k]; plan.hub_eb_old.push_back(o); plan.hub_pose.push_back(g.eb_pose[o]); plan.tile_pose.push_back(g.eb_pose[o]); }
    plan.hub_off.push_back((int32_t)plan.hub_pose.size());
  }
  if (!hubs.empty()) plan.dense_tiles_ok = false;      // (the dense assembly walks tiles only: graphs with hubs are solved by the PCG)
  plan.NPS = (int)plan.tile_pose.size();
  plan.tile_pose.push_back(0);                         // (one entry of padding: the tile kernels read slot min(thread, slots - 1) unconditionally, also for a tile without slots)
  plan.pt_single.assign(std::max(g.n_point, 1), 0);
  for (int c = 0; c < plan.n_chains(); ++c) if (plan.chain_off[c + 1] - plan.chain_off[c] == 1) plan.pt_single[plan.chain_off[c]] = 1;
}

// ---- points, measurements and weights in the device's order, and the compact edge inputs where they are lossless (ba_dev.hpp): one information scalar per edge
// class, fp32 measurements
void permute_data(const vdo_ba_graph& g, BaPlan& plan) {
  // (Ebp: entries of the padded edge blocks; entries without an edge keep zeros)
  const int L = g.n_point, Eb = g.n_eb, Et = g.n_et, Ebp = plan.Ebp();
  plan.point.resize(3 * (size_t)L);
  plan.eb_z.assign(3 * (size_t)Ebp, 0.0); plan.eb_w.assign(Ebp, 0.0);
  plan.et_z.resize(3 * (size_t)Et); plan.et_w.resize(Et);
  for (int l = 0; l < L; ++l) for (int k = 0; k < 3; ++k) plan.point[3 * (size_t)l + k] = g.point[3 * (size_t)plan.pt_old_of_new[l] + k];
  for (int e = 0; e < Ebp; ++e) {
    const int o = plan.eb_old_of_new[e];
    if (o < 0) continue;
    for (int k = 0; k < 3; ++k) plan.eb_z[(size_t)k * Ebp + e] = g.eb_z[(size_t)k * Eb + o];
    plan.eb_w[e] = g.eb_w[o];
  }
  for (int e = 0; e < Et; ++e) {
    const int o = plan.et_old_of_new[e];
    for (int k = 0; k < 3; ++k) plan.et_z[(size_t)k * Et + e] = g.et_z[(size_t)k * Et + o];
    plan.et_w[e] = g.et_w[o];
  }
  const int n_hub_edges = plan.n_hub_edges();
  plan.hub_z.assign(3 * (size_t)std::max(n_hub_edges, 1), 0.0); plan.hub_w.assign(std::max(n_hub_edges, 1), 0.0);
  for (int e = 0; e < n_hub_edges; ++e) {
    const int o = plan.hub_eb_old[e];
    for (int k = 0; k < 3; ++k) plan.hub_z[(size_t)k * n_hub_edges + e] = g.eb_z[(size_t)k * Eb + o];
    plan.hub_w[e] = g.eb_w[o];
  }
  bool wb_uni = Eb > 0, wt_uni = Et > 0, zb_f32 = Eb > 0, zt_zero = Et > 0;
  for (int e = 1; e < Eb && wb_uni; ++e) wb_uni = g.eb_w[e] == g.eb_w[0];
  for (int e = 1; e < Et && wt_uni; ++e) wt_uni = plan.et_w[e] == plan.et_w[0];
  for (size_t i = 0; i < 3 * (size_t)Ebp && zb_f32; ++i) zb_f32 = plan.eb_z[i] == (double)(float)plan.eb_z[i];
  for (size_t i = 0; i < 3 * (size_t)Et && zt_zero; ++i) zt_zero = plan.et_z[i] == 0.0;
  if (zb_f32) plan.eb_zf.assign(plan.eb_z.begin(), plan.eb_z.end());
  plan.compact_edges = (wb_uni ? 1 : 0) | (zb_f32 ? 2 : 0) | (wt_uni ? 4 : 0) | (zt_zero ? 8 : 0);
}

// ---- pose -> slots, pose -> EdgeSE3 (edge << 1 | side), pose -> priors
void pose_tables(const vdo_ba_graph& g, const BaPlanOptions& opt, BaPlan& plan) {
  const int P = g.n_pose, NPS = plan.NPS;
  csr_fill(P, NPS, [&](int k) { return plan.tile_pose[k]; }, plan.ps_off, plan.ps_idx);
  // pose-major rows of the sweep partials (ba_dev.hpp): slot s -> row slot_dst[s]; 16 sums per row unless a pose carries both edge kinds
  plan.slot_dst.assign((size_t)NPS + 1, 0);
  for (int k = 0; k < NPS; ++k) plan.slot_dst[plan.ps_idx[k]] = k;
  plan.hub_row.assign(std::max(plan.n_hub_edges(), 1), 0);
  for (int e = 0; e < plan.n_hub_edges(); ++e) plan.hub_row[e] = plan.slot_dst[(size_t)plan.NPS_tiles + e];
  plan.pose_kind.assign(std::max(P, 1), 0);
  std::vector<char> has_b(P, 0), has_t(P, 0);
  for (int e = 0; e < g.n_eb; ++e) has_b[g.eb_pose[e]] = 1;
  for (int e = 0; e < g.n_et; ++e) has_t[g.et_pose[e]] = 1;
  plan.ps_stride = opt.wide_partials ? 32 : 16;
  for (int p = 0; p < P; ++p) { plan.pose_kind[p] = has_t[p] ? 1 : 0; if (has_b[p] && has_t[p]) plan.ps_stride = 32; }
  csr_fill(P, 2 * g.n_ep, [&](int s) { return (s & 1) ? g.ep_j[s >> 1] : g.ep_i[s >> 1]; }, plan.pe_off, plan.pe_idx);
  csr_fill(P, g.n_prior, [&](int q) { return g.pr_pose[q]; }, plan.pr_off, plan.pr_idx);
  plan.pr_idx.resize(std::max(g.n_prior, 1), 0);
}

// ---- pose chains for the block-tridiagonal preconditioner: connected components of the pose-pose (EdgeSE3) graph that are simple paths - the odometry chain of
// the cameras, the smoothness chain of every object's motions - in path order; every other pose (isolated, or part of a branching / cyclic component) is a chain
// of length 1 (plain block-Jacobi).
// A path of >= kTwistMin poses is stored in TWISTED order - first half p_0 .. p_{m-1}, then the second half BACKWARDS p_{n-1} .. p_{m+1}, then p_m (the joint) -
// so that its block LDL^T is two independent recurrences of half the depth that meet in one step (k_pchain_factor runs them on two waves).  In that order
// position m (p_{n-1}) has no predecessor (pc_edge = -1: L = 0, the substitutions restart there by themselves) and the joint has two: position n-2 (the ordinary
// link) and position m-1 - the chain's one FAR link (pc_far_pos / pc_far_edge, -1 for an untwisted chain).  No fill-in: an exact factorisation of the same
// block-tridiagonal matrix, reordered.
void pose_chains(const vdo_ba_graph& g, const BaPlanOptions& opt, BaPlan& plan) {
  const int P = g.n_pose;
  const std::vector<int32_t>&pe_off = plan.pe_off, &pe_idx = plan.pe_idx;
  auto other_end = [&](int k) { const int e = pe_idx[k] >> 1; return (pe_idx[k] & 1) ? g.ep_i[e] : g.ep_j[e]; };
  auto single = [&](int p) { plan.pc_pose.push_back(p); plan.pc_edge.push_back(-1); plan.pc_off.push_back((int32_t)plan.pc_pose.size()); plan.pc_far_pos.push_back(-1); plan.pc_far_edge.push_back(-1); };
  plan.pc_off.assign(1, 0);
  std::vector<int> deg(P, 0);
  for (int e = 0; e < g.n_ep; ++e) { deg[g.ep_i[e]]++; deg[g.ep_j[e]]++; }
  std::vector<int> comp(P, -1);
  std::vector<char> comp_ok;
  std::vector<int> stack;
  for (int p0 = 0; p0 < P; ++p0) {
    if (comp[p0] != -1) continue;
    const int c = (int)comp_ok.size();
    int nodes = 0, degsum = 0; bool ok = true;
    stack.assign(1, p0); comp[p0] = c;
    while (!stack.empty()) {
      const int p = stack.back(); stack.pop_back();
      ++nodes; degsum += deg[p];
      if (deg[p] > 2) ok = false;
      for (int k = pe_off[p]; k < pe_off[p + 1]; ++k) {
        const int q = other_end(k);
        if (comp[q] == -1) { comp[q] = c; stack.push_back(q); }
      }
    }
    if (degsum / 2 != nodes - 1) ok = false;        // a tree with max degree 2 is a path; anything else has a cycle or a double edge
    comp_ok.push_back(ok ? 1 : 0);
    plan.pose_graph_is_paths = plan.pose_graph_is_paths && ok;      // (else the auto solver choice goes to the dense Cholesky, ba_lm.hip)
  }
  std::vector<char> done(P, 0);
  std::vector<int32_t> nodes, via_of;               // a path, and for t >= 1 the link nodes[t-1] -> nodes[t] (edge << 1 | side)
  for (int p0 = 0; p0 < P; ++p0) {
    if (done[p0]) continue;
    if (!comp_ok[comp[p0]] || deg[p0] == 0) { done[p0] = 1; single(p0); continue; }
    if (deg[p0] != 1) continue;                       // start paths at their lower-numbered end point
    nodes.clear(); via_of.clear();
    int prev = -1, cur = p0, via = -1;
    while (cur != -1) {
      done[cur] = 1; nodes.push_back(cur); via_of.push_back(via);
      int nxt = -1, nvia = -1;
      for (int k = pe_off[cur]; k < pe_off[cur + 1]; ++k) {
        const int q = other_end(k);
        if (q != prev && !done[q]) { nxt = q; nvia = pe_idx[k]; }     // side 0: cur is i of the edge -> E(cur,next) = block(i,j); 1: transposed
      }
      prev = cur; cur = nxt; via = nvia;
    }
    const int n = (int)nodes.size(), base = (int)plan.pc_pose.size();
    if (n < kTwistMin || opt.no_twist) {
      for (int t = 0; t < n; ++t) { plan.pc_pose.push_back(nodes[t]); plan.pc_edge.push_back(via_of[t]); }
      plan.pc_far_pos.push_back(-1); plan.pc_far_edge.push_back(-1);
    } else {
      const int m = n / 2;
      for (int t = 0; t < m; ++t) { plan.pc_pose.push_back(nodes[t]); plan.pc_edge.push_back(via_of[t]); }
      // second half backwards: position m + u holds nodes[n-1-u]; its predecessor position holds nodes[n-u], the link between them is via_of[n-u] walked the other way
      for (int u = 0; n - 1 - u > m; ++u) { plan.pc_pose.push_back(nodes[n - 1 - u]); plan.pc_edge.push_back(u == 0 ? -1 : (via_of[n - u] ^ 1)); }
      plan.pc_pose.push_back(nodes[m]); plan.pc_edge.push_back(via_of[m + 1] ^ 1);      // the joint: ordinary link from nodes[m+1] (position n-2) ...
      plan.pc_far_pos.push_back(base + m - 1); plan.pc_far_edge.push_back(via_of[m]);    // ... and the far link from nodes[m-1] (position m-1)
    }
    plan.pc_off.push_back((int32_t)plan.pc_pose.size());
  }
  for (int p = 0; p < P; ++p) if (!done[p]) single(p);      // unreachable, defensive
  for (int c = 0; c < plan.n_pchains(); ++c) plan.pc_maxlen = std::max(plan.pc_maxlen, (int)(plan.pc_off[c + 1] - plan.pc_off[c]));
}

// The device holds the tile descriptors in LAUNCH order (tiles with the longest landmark chain first: their serial solves would be the tail of a launch; they
// are also the ones with ternary edges, ~1.5x the work in the sweep): workgroup b reads descriptor b straight from its block id - no order array in front of it
// (the chain of dependent loads at the head of a tile was a quarter of its time).  The dynamic tiles come first: n_dyn_tiles of them.
void launch_order(BaPlan& plan) {
  const int n_tiles = plan.n_tiles();
  std::vector<int32_t> longest(std::max(n_tiles, 1), 0);
  plan.tile_order.assign(std::max(n_tiles, 1), 0);
  for (int t = 0; t < n_tiles; ++t) {
    const Tile& T = plan.tiles[t];
    plan.tile_order[t] = t;
    for (int c = T.chain_begin; c < T.chain_end; ++c) longest[t] = std::max(longest[t], plan.chain_off[c + 1] - plan.chain_off[c]);
    if (longest[t] > 1 || T.et_end > T.et_begin) ++plan.n_dyn_tiles;
  }
  std::stable_sort(plan.tile_order.begin(), plan.tile_order.begin() + n_tiles, [&](int a, int b) { return longest[a] > longest[b]; });
  plan.tiles_launch.assign(std::max(n_tiles, 1), Tile{});
  for (int b = 0; b < n_tiles; ++b) plan.tiles_launch[b] = plan.tiles[plan.tile_order[b]];
}

}  // namespace

int plan_graph(const vdo_ba_graph& g, const BaPlanOptions& opt, BaPlan& plan) {
  const auto t0 = std::chrono::steady_clock::now();
  auto mark = [&](int k) { if (opt.trace) plan.t_mark[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  plan.P = g.n_pose; plan.L = g.n_point; plan.Eb = g.n_eb; plan.Et = g.n_et; plan.Ep = g.n_ep; plan.Npr = g.n_prior;
  int rc = validate(g);
  if (rc != VDO_OK) return rc;
  mark(0);
  Tracks tr;
  rc = find_and_order_tracks(g, tr);
  if (rc != VDO_OK) return rc;
  mark(1);
  std::vector<int32_t> hubs;
  rc = build_tiles(g, opt, tr, plan, hubs);
  if (rc != VDO_OK) return rc;
  mark(2);
  add_hubs(g, tr, hubs, plan);
  mark(3);
  permute_data(g, plan);
  pose_tables(g, opt, plan);
  mark(4);
  pose_chains(g, opt, plan);
  launch_order(plan);
  return VDO_OK;
}

}  // namespace vdo

// ---- the plan behind a C handle, for the tests (include/vdo_slam_hip.h)
struct vdo_ba_plan {
  vdo::BaPlan plan;
  int64_t dims[13];
};

extern "C" int vdo_ba_plan_create(const vdo_ba_graph* g, vdo_ba_plan** out) {
  using namespace vdo;
  if (!g || !out) return set_error(VDO_ERR_INVALID, "vdo_ba_plan_create: null argument");
  if (g->n_pose <= 0 || g->n_point < 0 || g->n_eb < 0 || g->n_et < 0 || g->n_ep < 0 || g->n_prior < 0)
    return set_error(VDO_ERR_INVALID, "vdo_ba_create: negative/empty sizes");
  vdo_ba_plan* p = new vdo_ba_plan();
  const int rc = plan_graph(*g, BaPlanOptions::from_env(), p->plan);
  if (rc != VDO_OK) { delete p; return rc; }
  const BaPlan& q = p->plan;
  const int64_t dims[13] = {q.n_tiles(), q.NPS, q.max_slots, q.ps_stride, q.n_hubs(), q.n_hub_edges(), q.Ebp(), q.n_dyn_tiles, q.n_pchains(), q.pc_maxlen,
                            q.pose_graph_is_paths ? 1 : 0, q.dense_tiles_ok ? 1 : 0, q.compact_edges};
  std::memcpy(p->dims, dims, sizeof dims);
  *out = p;
  return VDO_OK;
}

extern "C" int vdo_ba_plan_array(const vdo_ba_plan* p, const char* name, const void** data, int64_t* count, int32_t* elem_bytes) {
  using namespace vdo;
  if (!p || !name || !data || !count || !elem_bytes) return set_error(VDO_ERR_INVALID, "vdo_ba_plan_array: null argument");
  const BaPlan& q = p->plan;
  auto give = [&](const void* ptr, size_t n, size_t bytes) { *data = ptr; *count = (int64_t)n; *elem_bytes = (int32_t)bytes; return VDO_OK; };
  if (!std::strcmp(name, "dims")) return give(p->dims, 13, sizeof(int64_t));
  // (a tile descriptor goes out as its 12 int32 fields)
  if (!std::strcmp(name, "tiles")) return give(q.tiles.data(), q.tiles.size() * (sizeof(Tile) / 4), 4);
  if (!std::strcmp(name, "tiles_launch")) return give(q.tiles_launch.data(), q.tiles_launch.size() * (sizeof(Tile) / 4), 4);
#define VDO_PLAN_FIELD(f) if (!std::strcmp(name, #f)) return give(q.f.data(), q.f.size(), sizeof(q.f[0]));
  VDO_PLAN_FIELD(tile_order) VDO_PLAN_FIELD(tile_pose) VDO_PLAN_FIELD(chain_off) VDO_PLAN_FIELD(pt_prev_edge) VDO_PLAN_FIELD(pt_single)
  VDO_PLAN_FIELD(eb_key) VDO_PLAN_FIELD(et_key) VDO_PLAN_FIELD(et_slot) VDO_PLAN_FIELD(inc_key)
  VDO_PLAN_FIELD(pt_old_of_new) VDO_PLAN_FIELD(pt_new_of_old) VDO_PLAN_FIELD(eb_old_of_new) VDO_PLAN_FIELD(et_old_of_new)
  VDO_PLAN_FIELD(inc_of_eb) VDO_PLAN_FIELD(inc1_of_et) VDO_PLAN_FIELD(inc2_of_et)
  VDO_PLAN_FIELD(ps_off) VDO_PLAN_FIELD(ps_idx) VDO_PLAN_FIELD(slot_dst) VDO_PLAN_FIELD(pose_kind)
  VDO_PLAN_FIELD(pe_off) VDO_PLAN_FIELD(pe_idx) VDO_PLAN_FIELD(pr_off) VDO_PLAN_FIELD(pr_idx)
  VDO_PLAN_FIELD(pc_off) VDO_PLAN_FIELD(pc_pose) VDO_PLAN_FIELD(pc_edge) VDO_PLAN_FIELD(pc_far_pos) VDO_PLAN_FIELD(pc_far_edge)
  VDO_PLAN_FIELD(hub_off) VDO_PLAN_FIELD(hub_point) VDO_PLAN_FIELD(hub_pose) VDO_PLAN_FIELD(hub_eb_old) VDO_PLAN_FIELD(hub_row) VDO_PLAN_FIELD(hub_z) VDO_PLAN_FIELD(hub_w)
  VDO_PLAN_FIELD(point) VDO_PLAN_FIELD(eb_z) VDO_PLAN_FIELD(eb_w) VDO_PLAN_FIELD(et_z) VDO_PLAN_FIELD(et_w) VDO_PLAN_FIELD(eb_zf)
#undef VDO_PLAN_FIELD
  return set_error(VDO_ERR_INVALID, "vdo_ba_plan_array: no array named '%s'", name);
}

extern "C" int vdo_ba_plan_destroy(vdo_ba_plan* p) {
  delete p;
  return VDO_OK;
}
