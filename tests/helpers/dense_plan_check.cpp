// Exhaustive host-only check of vdo_slam_amd/csrc/dense_plan.hpp (dn_move, dn_clip) against brute force; tests/test_dense_plan.py builds and runs it.
// Prints one line and returns 0, or the first failing case and 1.
#include <climits>
#include <cstdint>
#include <cstdio>

#include "../../vdo_slam_amd/csrc/dense_plan.hpp"

using namespace vdo;

static long long g_cases = 0;

// the global voxel that slot s of an axis of size n holds when the origin is o: the g in [o, o + n) with g mod n == s
static int64_t global_of(int s, int64_t o, int n) { return o + ((s - o) % n + n) % n; }

// a slot keeps its word iff its global voxel is the same before and after; the slots that `m` clears must be exactly the others
static bool move_ok(const int n[3], const int from[3], const int to[3]) {
  ++g_cases;
  const DnMove m = dn_move(n, from, to);
  bool ok = m.slabs >= 0 && m.slabs <= 3 && !(m.all && m.slabs);
  for (int i = 0; ok && i < m.slabs; ++i) {
    const int k = m.slab[i].axis;
    ok = k >= 0 && k < 3 && (i == 0 || k > m.slab[i - 1].axis) && m.slab[i].s0 >= 0 && m.slab[i].s0 < n[k] && m.slab[i].len >= 1 && m.slab[i].len < n[k];
  }
  for (int z = 0; ok && z < n[2]; ++z)
    for (int y = 0; y < n[1]; ++y)
      for (int x = 0; x < n[0]; ++x) {
        const int s[3] = {x, y, z};
        bool keep = true, cleared = m.all;
        for (int k = 0; k < 3; ++k) keep = keep && global_of(s[k], from[k], n[k]) == global_of(s[k], to[k], n[k]);
        for (int i = 0; i < m.slabs; ++i) {
          const int k = m.slab[i].axis;
          cleared = cleared || ((s[k] - m.slab[i].s0) % n[k] + n[k]) % n[k] < m.slab[i].len;
        }
        ok = ok && keep == !cleared;
      }
  if (!ok) std::printf("dn_move: n %d %d %d from %d %d %d to %d %d %d\n", n[0], n[1], n[2], from[0], from[1], from[2], to[0], to[1], to[2]);
  return ok;
}

// the clipped box must be the set of the volume's voxels with lo <= g < hi on every axis; empty is all zeros
static bool clip_ok(const int n[3], const int o[3], const int32_t lo[3], const int32_t hi[3]) {
  ++g_cases;
  const DnClip c = dn_clip(n, o, lo, hi);
  long long count = 0;
  int64_t mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, mx[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
  for (int z = 0; z < n[2]; ++z)
    for (int y = 0; y < n[1]; ++y)
      for (int x = 0; x < n[0]; ++x) {
        const int64_t g[3] = {(int64_t)o[0] + x, (int64_t)o[1] + y, (int64_t)o[2] + z};
        bool in = true;
        for (int k = 0; k < 3; ++k) in = in && lo[k] <= g[k] && g[k] < hi[k];
        if (!in) continue;
        ++count;
        for (int k = 0; k < 3; ++k) { mn[k] = g[k] < mn[k] ? g[k] : mn[k]; mx[k] = g[k] > mx[k] ? g[k] : mx[k]; }
      }
  bool ok = c.empty == (count == 0) && c.voxels() == count;
  for (int k = 0; k < 3; ++k) ok = ok && (count ? c.box.lo[k] == mn[k] && c.box.b[k] == mx[k] - mn[k] + 1 : c.box.lo[k] == 0 && c.box.b[k] == 0);
  if (!ok) std::printf("dn_clip: n %d %d %d o %d %d %d lo %d %d %d hi %d %d %d\n", n[0], n[1], n[2], o[0], o[1], o[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
  return ok;
}

int main() {
  const int kMax = (1 << 22) - 1;
  // the three origin triples of the joint loops: every axis away from 0, both signs, a multiple of no size
  const int O3[3][3] = {{-7, 3, 7}, {4, -7, -1}, {7, 6, -5}};

  // THE MOVE, per axis: every size 1..5, every origin -7..7, every move -12..12 on axis k; every size on the other two, which stand still
  for (int k = 0; k < 3; ++k)
    for (int nk = 1; nk <= 5; ++nk) for (int ok = -7; ok <= 7; ++ok) for (int dk = -12; dk <= 12; ++dk)
      for (int na = 1; na <= 5; ++na) for (int nb = 1; nb <= 5; ++nb) {
        int n[3], from[3], to[3];
        n[k] = nk; n[(k + 1) % 3] = na; n[(k + 2) % 3] = nb;
        from[k] = ok; from[(k + 1) % 3] = 4; from[(k + 2) % 3] = -3;
        for (int a = 0; a < 3; ++a) to[a] = from[a];
        to[k] += dk;
        if (!move_ok(n, from, to)) return 1;
      }
  // the axes together (what couples them is `all`): every size and every move -12..12 on every axis at once
  for (int nx = 1; nx <= 5; ++nx) for (int ny = 1; ny <= 5; ++ny) for (int nz = 1; nz <= 5; ++nz)
    for (int dx = -12; dx <= 12; ++dx) for (int dy = -12; dy <= 12; ++dy) for (int dz = -12; dz <= 12; ++dz) {
      const int n[3] = {nx, ny, nz}, *from = O3[(dx + dy + dz + 36) % 3], to[3] = {from[0] + dx, from[1] + dy, from[2] + dz};
      if (!move_ok(n, from, to)) return 1;
    }
  // at the edge of the origin's range, +-(2^22 - 1): towards the inside and along the edge
  for (int nn = 1; nn <= 5; ++nn) for (int d = -12; d <= 12; ++d) for (int k = 0; k < 3; ++k) {
    const int n[3] = {nn, 6 - nn, 3};
    int lo_o[3] = {-kMax, -kMax, -kMax}, hi_o[3] = {kMax + 1 - n[0], kMax + 1 - n[1], kMax + 1 - n[2]}, to[3];
    for (int a = 0; a < 3; ++a) to[a] = lo_o[a];
    to[k] += d < 0 ? -d : d;
    if (!move_ok(n, lo_o, to) || !move_ok(n, to, lo_o)) return 1;
    for (int a = 0; a < 3; ++a) to[a] = hi_o[a];
    to[k] -= d < 0 ? -d : d;
    if (!move_ok(n, hi_o, to) || !move_ok(n, to, hi_o)) return 1;
    if (!move_ok(n, lo_o, hi_o) || !move_ok(n, hi_o, lo_o)) return 1;
  }

  // THE BOX, per axis: the same sizes and origins, lo and hi from -9..9, INT32_MIN and INT32_MAX on axis k; the other two axes whole, or one of them empty
  int32_t V[21];
  for (int i = 0; i < 19; ++i) V[i] = i - 9;
  V[19] = INT32_MIN; V[20] = INT32_MAX;
  for (int k = 0; k < 3; ++k)
    for (int nk = 1; nk <= 5; ++nk) for (int ok = -7; ok <= 7; ++ok) for (int il = 0; il < 21; ++il) for (int ih = 0; ih < 21; ++ih)
      for (int other = 0; other < 3; ++other) {
        int n[3], o[3];
        int32_t lo[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, hi[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
        n[k] = nk; n[(k + 1) % 3] = 1 + (nk + ok + 7) % 5; n[(k + 2) % 3] = 1 + (il + ih) % 5;
        o[k] = ok; o[(k + 1) % 3] = -6; o[(k + 2) % 3] = 5;
        lo[k] = V[il]; hi[k] = V[ih];
        if (other == 1) { lo[(k + 1) % 3] = -5; hi[(k + 1) % 3] = -5; }                 // empty there: everything is 0
        if (other == 2) { lo[(k + 2) % 3] = 6; hi[(k + 2) % 3] = 7; }                   // one voxel thick there
        if (!clip_ok(n, o, lo, hi)) return 1;
      }
  // the axes together (what couples them is `empty`): every size, bounds on every axis at once
  const int32_t LO[4] = {INT32_MIN, -9, 1, 9}, HI[4] = {-9, 2, 9, INT32_MAX};
  for (int nx = 1; nx <= 5; ++nx) for (int ny = 1; ny <= 5; ++ny) for (int nz = 1; nz <= 5; ++nz)
    for (int q = 0; q < 4096; ++q) {
      const int n[3] = {nx, ny, nz}, *o = O3[q % 3];
      const int32_t lo[3] = {LO[q & 3], LO[q >> 2 & 3], LO[q >> 4 & 3]}, hi[3] = {HI[q >> 6 & 3], HI[q >> 8 & 3], HI[q >> 10 & 3]};
      if (!clip_ok(n, o, lo, hi)) return 1;
    }
  // a volume at the edge of the origin's range against the widest box
  {
    const int n[3] = {5, 3, 4}, o[3] = {-kMax, kMax + 1 - 3, 0};
    const int32_t lo[3] = {INT32_MIN, INT32_MIN, 2}, hi[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
    if (!clip_ok(n, o, lo, hi)) return 1;
  }
  std::printf("dense_plan ok: %lld cases\n", g_cases);
  return 0;
}
