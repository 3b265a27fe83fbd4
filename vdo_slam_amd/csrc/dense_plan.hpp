// The integer decisions about a cyclic volume: where an origin sits in the slots, what a box leaves of the volume, what a move of the origin makes
// stale.  No HIP type: dense.hpp includes it for the library, tests/helpers/dense_plan_check.cpp for an exhaustive host-only check.
#pragma once
#include <cstdint>

namespace vdo {

inline int dn_mod(int g, int n) { const int m = g % n; return m < 0 ? m + n : m; }      // g mod n in [0, n), n > 0

struct DnBox { int lo[3], b[3]; };                                         // a box's first global voxel and its size; k_dn_extract takes it by value

// [lo, hi) clipped against the volume [o, o + n): every size > 0, or `empty` with every field 0
struct DnClip { DnBox box; bool empty; long long voxels() const { return (long long)box.b[0] * box.b[1] * box.b[2]; } };

inline DnClip dn_clip(const int n[3], const int o[3], const int32_t lo[3], const int32_t hi[3]) {
  DnClip c{};
  for (int k = 0; k < 3; ++k) {
    const int64_t end = (int64_t)o[k] + n[k], a0 = lo[k] > o[k] ? lo[k] : o[k], a1 = hi[k] < end ? hi[k] : end;
    if (a1 <= a0) { c = DnClip{}; c.empty = true; return c; }
    c.box.lo[k] = (int)a0; c.box.b[k] = (int)(a1 - a0);
  }
  return c;
}

// What a move of the origin makes stale: everything (`all`: an axis moved by n or more), or per moved axis ONE leaving slab - `len` slots from slot
// `s0` on (cyclic) on `axis`, whole on the other two: the first d voxels of the axis when the volume moves up by d, the last -d when it moves down.
// A slot outside every slab holds the same global voxel before and after.
struct DnMove { bool all; int slabs; struct { int axis, s0, len; } slab[3]; };

inline DnMove dn_move(const int n[3], const int from[3], const int to[3]) {
  DnMove m{};
  int64_t d[3];
  for (int k = 0; k < 3; ++k) { d[k] = (int64_t)to[k] - from[k]; m.all = m.all || d[k] >= n[k] || -d[k] >= n[k]; }
  for (int k = 0; k < 3 && !m.all; ++k) {
    if (d[k] == 0) continue;
    const int len = (int)(d[k] > 0 ? d[k] : -d[k]), g0 = d[k] > 0 ? from[k] : from[k] + n[k] - len;
    m.slab[m.slabs].axis = k; m.slab[m.slabs].s0 = dn_mod(g0, n[k]); m.slab[m.slabs++].len = len;
  }
  return m;
}

}  // namespace vdo
